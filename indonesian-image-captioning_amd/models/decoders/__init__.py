from .ensemble import DecoderEnsemble  # noqa: F401
