from .ensemble import DecoderEnsemble  # noqa: F401
from .search_options import SearchOptions  # noqa: F401
