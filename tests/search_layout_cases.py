"""The workspace queries of the search and rollout drivers (csrc/beam_search.cpp) over a small table: byte count and
result offsets of every form.  They launch nothing and load without a GPU.

    python tests/search_layout_cases.py --record     writes tests/golden/search_layouts.json from the library in the tree

The stored file was recorded once, on a build of the commit BEFORE the four search drivers became one, so
tests/test_search_layout.py pins the layouts of that commit: a workspace laid out differently would leave every kernel's
tests passing and break a caller that kept offsets."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "indonesian-image-captioning_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "search_layouts.json")

# dims in scnattn_dims order (B, P, E, A, D, F, M, S, V, T, L, has_att): the attention decoder of
# test_c_entry_points_refuse_without_a_gpu, and one without attention and with another D
DIMS = {"att": (3, 49, 256, 128, 128, 128, 64, 40, 1003, 51, 51, 1),
        "noatt": (3, 49, 256, 128, 96, 128, 64, 40, 1003, 51, 51, 0)}
KT = ((1, 1), (5, 51), (8, 7))
ENSEMBLES = (("att",), ("noatt",), ("att", "noatt"), ("noatt", "att"), ("att", "noatt", "noatt", "att"))
ALPHA_MEMBERS = (-1, 0, 1)


def _options():
    from scnattn import _lib as L
    return L.SearchOpts(min_length=0, no_repeat_ngram=2, n_banned=1, banned=(C.c_int32 * L.MAX_BANNED)(7))


def _query(workspace, layout, noff, *args):
    """(bytes, [offsets]) of one form; args: what the two calls take before their output pointer"""
    from scnattn import _lib as L
    h = L.lib()
    n, off = C.c_size_t(), (C.c_long * noff)()
    assert getattr(h, workspace)(*args, C.byref(n)) == 0, h.scnattn_last_error()
    assert getattr(h, layout)(*args, off) == 0, h.scnattn_last_error()
    return [n.value, list(off)]


def single(name, K, T, options):
    from scnattn import _lib as L
    d = L.Dims(*DIMS[name])
    if options:
        return _query("scnattn_beam_workspace_opt", "scnattn_beam_layout_opt", L.BEAM_NOFF_OPT, C.byref(d), K, T,
                      C.byref(_options()))
    return _query("scnattn_beam_workspace", "scnattn_beam_layout", L.BEAM_NOFF, C.byref(d), K, T)


def ensemble(names, K, T, alpha_member, options):
    from scnattn import _lib as L
    d = (L.Dims * len(names))(*[L.Dims(*DIMS[x]) for x in names])
    if options:
        return _query("scnattn_ensemble_workspace_opt", "scnattn_ensemble_layout_opt", L.BEAM_NOFF_OPT, len(names), d, K, T,
                      alpha_member, C.byref(_options()))
    return _query("scnattn_ensemble_workspace", "scnattn_ensemble_layout", L.BEAM_NOFF, len(names), d, K, T, alpha_member)


def rollout(name, K, T, want_alpha):
    from scnattn import _lib as L
    d = L.Dims(*DIMS[name])
    return _query("scnattn_rollout_workspace", "scnattn_rollout_layout", L.ROLLOUT_NOFF, C.byref(d), K, T, want_alpha)


def cases():
    """{case id: (function, arguments)} -- every form at every (K, T) of the table"""
    out = {}
    for K, T in KT:
        at = "K%d-T%d" % (K, T)
        for name in DIMS:
            for opt in (0, 1):
                out["single-%s-%s-opt%d" % (name, at, opt)] = (single, (name, K, T, opt))
            for wa in (0, 1):
                out["rollout-%s-%s-alpha%d" % (name, at, wa)] = (rollout, (name, K, T, wa))
        for names in ENSEMBLES:
            for am in ALPHA_MEMBERS:
                if am >= len(names):
                    continue
                for opt in (0, 1):
                    out["ens-%s-%s-am%d-opt%d" % ("+".join(names), at, am, opt)] = (ensemble, (names, K, T, am, opt))
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    rec = {k: fn(*args) for k, (fn, args) in cases().items()}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d layouts -> %s" % (len(rec), GOLDEN))
