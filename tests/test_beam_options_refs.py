"""tests/beam_options_refs.py (the restatement the search options are judged against on the GPU) pinned on the CPU: with
default options it IS beam_refs.search; rule 3 against a brute-force statement; the length-normalised pick; the refusals of
models.decoders.SearchOptions; and the caps of tests/test_gpu_beam_options_search.py, from the restatement alone."""
import random

import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
from helpers import params_from, t

A, B_, C_, D_, E_ = 0, 1, 2, 3, 4       # the alphabet of the rule tests; <end> = 5
END, V = 5, 6


# ---- default options: the search of beam_refs -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_default_options_are_beam_refs_search(name, kind):
    """sequences, fp64 scores and alphas EQUAL (==), k in {1, 3, 5}"""
    d, Vf = BR.sharpened(name)
    wm = BR.word_map(Vf)
    P64 = params_from(d, dtype=torch.float64)
    enc = t(d["enc"]).double()
    tags = t(d["tags"]).double() if kind != "pure_attention" else None
    for k in BR.BEAMS:
        want = BR.search(kind, P64, k, wm, enc, tags)
        got, traces = OR.search_one(kind, P64, k, wm, enc, tags)
        assert got == want, k
        assert len(traces) == enc.shape[0] and all(tr and len(tr[0]) == 3 for tr in traces)


# ---- rule 3 against brute force --------------------------------------------------------------------------------------------
def _brute_ngram(hist, t, g, alphabet):
    """v is excluded iff, after appending v, an n-gram of g words that ends at the last position occurs earlier too"""
    out = set()
    for v in alphabet:
        s = list(hist[:t]) + [v]
        grams = [tuple(s[i:i + g]) for i in range(len(s) - g + 1)]
        if grams and grams[-1] in grams[:-1]:
            out.add(v)
    return out


def test_ngram_rule_vs_brute_force():
    rnd = random.Random(7)
    checked = fired = 0
    for _ in range(600):
        t_ = rnd.randint(0, 12)
        hist = [rnd.randrange(5) for _ in range(t_)]
        for g in (1, 2, 3, 4):
            got = OR.excluded(hist, t_, V, END, OR.Opts(no_repeat_ngram=g))
            assert got == _brute_ngram(hist, t_, g, range(5)), (hist, g)
            assert END not in got
            checked += 1
            fired += bool(got)
            if t_ < g:
                assert not got
    assert checked == 2400 and fired >= 600
    # a history longer than t: only the first t words count
    assert OR.excluded([A, B_] + [C_], 2, V, END, OR.Opts(no_repeat_ngram=1)) == {A, B_}


def test_rules_by_hand():
    o2 = OR.Opts(no_repeat_ngram=2)
    assert OR.excluded([A, B_, A], 3, V, END, o2) == {B_}                    # a b a: b would repeat "a b"
    assert OR.excluded([A, B_, A, B_], 4, V, END, o2) == {A}
    assert OR.excluded([A, A], 2, V, END, o2) == {A}                         # the window i = t - g overlaps the tail
    for g in (1, 2, 3, 4, 8):                                               # t = g - 1: nothing yet; t = g: the first window
        hist = [A] * g
        assert OR.excluded(hist, g - 1, V, END, OR.Opts(no_repeat_ngram=g)) == set()
        assert OR.excluded(hist, g, V, END, OR.Opts(no_repeat_ngram=g)) == {A}
    o = OR.Opts(min_length=4)
    assert OR.excluded([A, B_, C_], 3, V, END, o) == {END} and OR.excluded([A, B_, C_, D_], 4, V, END, o) == set()
    assert OR.excluded([], 0, V, END, OR.Opts()) == set()
    all3 = OR.Opts(min_length=2, no_repeat_ngram=1, banned_tokens=(E_,))
    assert OR.excluded([C_], 1, V, END, all3) == {E_, END, C_}


def test_selection_skips_excluded_and_keeps_the_tie_rule():
    val = torch.tensor([[1.0, 3.0, 3.0, 3.0, 0.5, 2.0], [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]], dtype=torch.float64)
    v, i = OR.row_topk_excl(val, [{1}, {5, 3}], 3)
    assert i.tolist() == [[2, 3, 5], [4, 2, 1]] and v.tolist() == [[3.0, 3.0, 2.0], [4.0, 2.0, 1.0]]
    v0, i0 = OR.row_topk_excl(val, [set(), set()], 3)
    assert i0.tolist() == [[1, 2, 3], [5, 4, 3]]
    assert torch.equal(val, torch.tensor([[1.0, 3.0, 3.0, 3.0, 0.5, 2.0], [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]], dtype=torch.float64))
    with pytest.raises(AssertionError):
        OR.row_topk_excl(val, [{0, 1, 2, 3}, set()], 3)


# ---- the length-normalised pick --------------------------------------------------------------------------------------------
def test_length_penalty_picks():
    s = BR.word_map(12)["<start>"]
    done = [([s, 1, 11], -1.0), ([s, 1, 2, 3, 11], -1.4), ([s] + [1] * 9 + [11], -3.05)]       # L = 2, 4, 10
    assert OR.pick(done, 0.0) == 0          # -1.0, -1.4, -3.05
    assert OR.pick(done, 0.7) == 1          # -0.616, -0.530, -0.609
    assert OR.pick(done, 1.0) == 2          # -0.5, -0.35, -0.305
    tie = [([s, 1, 2, 11], -1.5), ([s, 4, 5, 11], -1.5), ([s, 1, 11], -1.5)]
    assert OR.pick(tie, 0.0) == 0 and OR.pick(tie, 1.0) == 0                # equal: the earlier completion
    # the project's own pick is the same rule
    from models.decoders import _common
    for alpha in (0.0, 0.7, 1.0, -0.5):
        for d_ in (done, tie):
            assert _common.pick_best([x[1] for x in d_], [len(x[0]) - 1 for x in d_], alpha) == OR.pick(d_, alpha)


def test_trace_back_applies_the_penalty():
    """hand-made device results of ONE image, K = 3: three beams completed at steps 1, 3 and 4"""
    from models.decoders import _common
    K, T, start, end = 3, 5, 10, 11
    token = torch.zeros(T, K, dtype=torch.int32)
    parent = torch.zeros(T, K, dtype=torch.int32)
    for t_ in range(T):
        token[t_] = torch.tensor([1 + t_, 1 + t_, 1 + t_])
    res = {"token": token, "parent": parent, "alpha": None, "ncomp": torch.tensor([3]), "nsrc": torch.tensor([0]),
           "comp_step": torch.tensor([1, 3, 4]), "comp_parent": torch.tensor([0, 0, 0]),
           "comp_score": torch.tensor([-1.0, -1.4, -1.7]), "best_idx": torch.tensor([0]), "scores": torch.zeros(K)}
    seqs = [[start, 1, end], [start, 1, 2, 3, end], [start, 1, 2, 3, 4, end]]      # L = 2, 4, 5
    for alpha, want in ((0.0, 0), (0.7, 1), (1.0, 2)):
        (one, done), = _common.trace_back(res, T, 1, K, start, end, (1, 1), False, return_all=True, length_penalty=alpha)
        assert one == seqs[want], alpha
        assert [s_ for s_, _ in done] == seqs and [round(x, 6) for _, x in done] == [-1.0, -1.4, -1.7]     # raw, in order


# ---- SearchOptions -----------------------------------------------------------------------------------------------------------
def test_search_options_refusals():
    from models.decoders import SearchOptions
    o = SearchOptions()
    assert (o.min_length, o.no_repeat_ngram, o.banned_tokens, o.length_penalty) == (0, 0, (), 0.0) and not o.on_device
    assert SearchOptions(length_penalty=0.7).on_device is False and SearchOptions(min_length=1).on_device
    for kw in (dict(no_repeat_ngram=9), dict(no_repeat_ngram=-1), dict(min_length=-1), dict(banned_tokens=range(65)),
               dict(banned_tokens=(-1,)), dict(length_penalty=float("inf")), dict(length_penalty=float("nan")),
               dict(min_length=1.5)):
        with pytest.raises(ValueError):
            SearchOptions(**kw)
    assert SearchOptions(banned_tokens=[3, 3, 1]).banned_tokens == (1, 3) and len(SearchOptions(banned_tokens=range(64)).banned_tokens) == 64
    Vw, K, T = 1003, 5, 51
    end = Vw - 1
    SearchOptions(min_length=50, no_repeat_ngram=8, banned_tokens=range(64)).check(Vw, K, T, end)
    for opt in (SearchOptions(banned_tokens=(end,)), SearchOptions(banned_tokens=(Vw,)), SearchOptions(min_length=51)):
        with pytest.raises(ValueError):
            opt.check(Vw, K, T, end)
    # the candidate-count rule: V - |B| - 1 - (g >= 1 ? max_steps : 0) >= K, on the boundary
    SearchOptions(no_repeat_ngram=1).check(57, 5, 51, 56)
    with pytest.raises(ValueError, match="candidates"):
        SearchOptions(no_repeat_ngram=1).check(56, 5, 51, 55)
    SearchOptions(banned_tokens=(1, 2)).check(8, 5, 51, 7)
    with pytest.raises(ValueError, match="candidates"):
        SearchOptions(banned_tokens=(1, 2, 3)).check(8, 5, 51, 7)
    # ... and the restatement refuses the same
    for opts, args in ((OR.Opts(no_repeat_ngram=1), (56, 5, 51, 55)), (OR.Opts(banned_tokens=(1, 2, 3)), (8, 5, 51, 7)),
                       (OR.Opts(banned_tokens=(7,)), (8, 5, 51, 7)), (OR.Opts(no_repeat_ngram=9), (1003, 5, 51, 1002))):
        assert OR.refusal(opts, *args) is not None
    assert OR.refusal(OR.Opts(no_repeat_ngram=1), 57, 5, 51, 56) is None
    wm = BR.word_map(30)
    o = SearchOptions.from_words(wm, min_length=2)
    assert o.banned_tokens == (wm["<unk>"],) and o.min_length == 2
    assert SearchOptions.from_words(wm, ban=("w1", "w2"), no_repeat_ngram=3).banned_tokens == (1, 2)
    with pytest.raises(ValueError):
        SearchOptions.from_words(wm, ban=("<end>",))
    with pytest.raises(ValueError):
        SearchOptions.from_words(wm, ban=("no such word",))


def test_sample_batch_refuses_before_the_gpu():
    """a refused option set raises ValueError on CPU tensors; a valid one reaches the 'no CPU fallback' refusal"""
    from models.decoders import DecoderEnsemble, SearchOptions
    from test_beam_host import _args, _decoders
    wm = BR.word_map(12)
    for m, has_tags in _decoders():
        with pytest.raises(ValueError, match="candidates"):
            m.sample_batch(3, wm, *_args(m, has_tags), options=SearchOptions(no_repeat_ngram=2))     # 12 - 1 - 51 < 3
        with pytest.raises(ValueError, match="<end>"):
            m.sample_batch(3, wm, *_args(m, has_tags), options=SearchOptions(banned_tokens=(11,)))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.sample_batch(3, wm, *_args(m, has_tags), options=SearchOptions(min_length=2))
    ens = DecoderEnsemble([m for m, _ in _decoders()])
    enc, tags = _args(None, True)
    with pytest.raises(ValueError, match="candidates"):
        ens.sample_batch(3, wm, enc, tags, options=SearchOptions(no_repeat_ngram=2))


def test_c_entry_points_refuse_without_a_gpu():
    import ctypes as C
    from scnattn import _lib as L
    h = L.lib()
    n = C.c_size_t()
    good = L.Dims(3, 49, 256, 128, 128, 128, 64, 40, 1003, 51, 51, 1)

    def opts(min_length=0, g=0, banned=()):
        o = L.SearchOpts(min_length=min_length, no_repeat_ngram=g, n_banned=len(banned))
        for i, b in enumerate(banned[:L.MAX_BANNED]):
            o.banned[i] = b
        return o

    plain = C.c_size_t()
    assert h.scnattn_beam_workspace(C.byref(good), 5, 51, C.byref(plain)) == 0
    assert h.scnattn_beam_workspace_opt(C.byref(good), 5, 51, C.byref(opts(8, 2, (1000,))), C.byref(n)) == 0
    hist_bytes = 4 * ((2 * 15 * 51 + 63) // 64 * 64)
    assert n.value == plain.value + hist_bytes           # the history int32 [2][N*K][max_steps], in 256-byte granules
    off = (C.c_long * L.BEAM_NOFF_OPT)()
    off13 = (C.c_long * L.BEAM_NOFF)()
    assert h.scnattn_beam_layout_opt(C.byref(good), 5, 51, C.byref(opts()), off) == 0
    assert h.scnattn_beam_layout(C.byref(good), 5, 51, off13) == 0
    assert list(off)[:L.BEAM_NOFF] == list(off13) and 0 <= off[13] < n.value // 4 and off[13] not in list(off13)
    small = L.Dims(3, 49, 256, 128, 128, 128, 64, 40, 56, 51, 51, 1)
    for dims, o, word in ((good, opts(g=9), b"no_repeat_ngram"), (good, opts(min_length=51), b"min_length"),
                          (good, opts(min_length=-1), b"min_length"), (good, opts(banned=(1003,)), b"outside"),
                          (small, opts(g=1), b"candidates")):
        assert h.scnattn_beam_workspace_opt(C.byref(dims), 5, 51, C.byref(o), C.byref(n)) == -1
        assert word in h.scnattn_last_error(), h.scnattn_last_error()
    o65 = opts()
    o65.n_banned = 65
    assert h.scnattn_beam_workspace_opt(C.byref(good), 5, 51, C.byref(o65), C.byref(n)) == -1
    assert h.scnattn_beam_workspace_opt(C.byref(good), 5, 51, None, C.byref(n)) == -1
    d2 = (L.Dims * 2)(good, good)
    assert h.scnattn_ensemble_workspace_opt(2, d2, 5, 51, 0, C.byref(opts(g=9)), C.byref(n)) == -1
    assert h.scnattn_ensemble_workspace_opt(2, d2, 5, 51, 0, C.byref(opts(8, 2)), C.byref(n)) == 0
    # a banned <end> is refused where the call knows <end>: before anything is launched (null operands are never reached)
    assert h.scnattn_beam_steps_opt(None, C.byref(good), 5, 51, C.byref(opts(banned=(1002,))), None, None, 1002, 0, 1, None) == -1
    assert b"end token" in h.scnattn_last_error()
    assert h.scnattn_version() == 109


# ---- the caps of tests/test_gpu_beam_options_search.py, from the restatement alone -----------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_ensemble_table_caps(mode):
    cs = OR.ensemble_cases(mode)
    left = sum(1 for _, ok, _ in cs.values() if not ok)
    changed = sum(1 for _, ok, differs in cs.values() if ok and differs)
    print("two-member ensemble, mode %d: %d cases, %d left out, the n-gram rule changes %d" % (mode, len(cs), left, changed))
    assert len(cs) == 9 and 4 * left <= len(cs) and changed >= 3


@pytest.mark.parametrize("name", sorted(OR.TABLES))
def test_table_caps(name):
    """at most 1/4 of a table's cases left out; rule 3 changes the caption of at least 3 compared cases (a kernel that
    ignored the history would otherwise pass)"""
    total, left, changed = OR.table_counts(name)
    print("%s: %d cases, %d left out, the n-gram rule changes %d compared captions" % (name, total, left, changed))
    assert total == 27 and 4 * left <= total
    assert changed >= 3
    for kind, seed, options in OR.TABLES[name]:
        for (one, done), _, _ in OR.cases(kind, seed, options).values():
            seq = OR._seq(one, kind)
            words = seq[1:-1] if seq[-1] == 1002 else seq[1:]
            g = options.no_repeat_ngram
            grams = [tuple(words[i:i + g]) for i in range(len(words) - g + 1)]
            assert len(grams) == len(set(grams)), "a repeated n-gram in the restatement's own caption"
            assert not set(words) & set(options.banned_tokens)
            assert all(len(s_) - 2 >= options.min_length for s_, _ in done if s_[-1] == 1002)
