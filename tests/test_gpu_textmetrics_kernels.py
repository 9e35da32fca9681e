"""GPU tests (``-m gpu``) of csrc/textmetrics.hip through the C ABI, against the restatements of tests/textmetrics_refs.py.

Bars.  Integers -- the n-gram statistics, lcs, the keys of scnattn_text_ref_keys and the document-frequency tables made of
them -- equal the restatement, no case excepted.  The fp64 ROUGE-L and CIDEr-D per-image scores and their corpus means:
|got - ref| <= 1e-12 * max(1, |ref|).  That bar is derived, not measured: every sum has at most a few hundred non-negative
terms (the idf weights are >= 0, nothing cancels), which bounds the rounding error near 3e-14; log, exp and sqrt are good to
a few ulp; the margin is about 30x.  A failure means a wrong term, not rounding.

Cases, the smallest at which these kernels can go wrong: all pairs of the lengths 0, 1, 3, 4, 63, 64, 65, 127, 128 (81 images,
two waves of tokens, both words of the 128-bit LCS recurrence); R = 1, 2 and 5; an absent slot in the middle and all slots
absent; clipping (2 2 2 2 2 against 1 2 2 2 3); a closest-length tie; hypotheses longer / shorter than every reference; skip
ids at the start, middle and end and sequences of skipped ids only; N = 1 (CIDEr exactly 0), 2, 70 and 81; an n-gram in
several references of one image (df counts it once), in every image (idf 0), in no reference; the 4-gram of four times the
largest admitted id next to the sentinel; a token one above the admitted range and a negative one (flag); a memory length
larger than the padded width (clamped, no fault); a padded width of 129 (refused); random corpora at V = 12 and V = 10 000."""
import ctypes as C
import math

import pytest
import torch

import textmetrics_refs as T

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _close(got, want):
    return abs(got - want) <= TOL * max(1.0, abs(want))


def _skip(ids):
    return (C.c_int32 * max(1, len(ids)))(*ids), len(ids)


def _run(dev, hyps, refs, skip_h=(), skip_r=(), hyp_len=None, ref_len=None):
    """every kernel on one corpus through the C ABI; tables as CaptionScorer builds them (sort, run lengths)"""
    from scnattn import _lib as L
    from scnattn import textmetrics as TM
    hyp, hl = TM.pack_captions(hyps, dev)
    ref, rl = TM.pack_references(refs, dev)
    if hyp_len is not None:
        hl = torch.tensor(hyp_len, dtype=torch.int32, device=dev)
    if ref_len is not None:
        rl = torch.tensor(ref_len, dtype=torch.int32, device=dev)
    N, Lh = hyp.shape
    _, R, Lr = ref.shape
    st = L.stream_of(hyp)
    sh, nh = _skip(skip_h)
    sr, nr = _skip(skip_r)
    stats = torch.full((N, 10), -7, dtype=torch.int32, device=dev)
    lcs = torch.full((N, R), -7, dtype=torch.int32, device=dev)
    rouge = torch.full((N,), -7.0, dtype=torch.float64, device=dev)
    cider = torch.full((N,), -7.0, dtype=torch.float64, device=dev)
    means = torch.full((2,), -7.0, dtype=torch.float64, device=dev)
    flags = torch.full((5,), -7, dtype=torch.int32, device=dev)
    keys = torch.full((4, N, R, Lr), -7, dtype=torch.int64, device=dev)
    common = (N, R, L.ptr(hyp), Lh, L.ptr(hl), L.ptr(ref), Lr, L.ptr(rl), sh, nh, sr, nr)
    L.call("scnattn_text_ngram_stats", st, *common, L.ptr(stats))
    L.call("scnattn_text_lcs", st, *common, L.ptr(lcs), L.ptr(rouge), C.c_void_p(means.data_ptr()))
    tk, td, off = [], [], [0]
    for n in range(1, 5):
        L.call("scnattn_text_ref_keys", st, n, N, R, L.ptr(ref), Lr, L.ptr(rl), sr, nr, L.ptr(keys[n - 1]),
               C.c_void_p(flags.data_ptr() + 4 * (n - 1)))
        k = keys[n - 1].reshape(-1)
        u, c = torch.unique_consecutive(torch.sort(k[k != -1])[0], return_counts=True)
        tk.append(u)
        td.append(c.to(torch.int32))
        off.append(off[-1] + u.numel())
    table_keys, table_df = torch.cat(tk).contiguous(), torch.cat(td).contiguous()
    L.call("scnattn_text_cider", st, *common, L.ptr(table_keys), L.ptr(table_df), (C.c_long * 5)(*off), N, L.ptr(cider),
           C.c_void_p(means.data_ptr() + 8), C.c_void_p(flags.data_ptr() + 16))
    torch.cuda.synchronize()
    return dict(stats=stats.tolist(), lcs=lcs.tolist(), rouge=rouge.tolist(), cider=cider.tolist(), means=means.tolist(),
                flags=flags.tolist(), keys=keys.tolist(), tables=[(a.tolist(), b.tolist()) for a, b in zip(tk, td)], Lr=Lr)


def _check(out, hyps, refs, flags=(0, 0, 0, 0, 0)):
    """every output of _run against the restatement applied to the (already stripped) corpus"""
    N = len(hyps)
    assert out["flags"] == list(flags)
    want_rouge = []
    for i, (h, r) in enumerate(zip(hyps, refs)):
        assert out["stats"][i] == T.ngram_stats(h, r), ("stats", i)
        ls, sc = T.rouge_l(h, r)
        ls = ls + [0] * (len(out["lcs"][i]) - len(ls))
        assert out["lcs"][i] == ls, ("lcs", i)
        assert _close(out["rouge"][i], sc), ("rouge", i, out["rouge"][i], sc)
        want_rouge.append(sc)
    assert _close(out["means"][0], T.mean(want_rouge))
    if any(flags):
        return
    tables = T.df_tables(refs)
    for n in range(1, 5):
        assert out["tables"][n - 1] == tables[n - 1], ("df table", n)
        for i, per in enumerate(refs):
            R = len(out["keys"][n - 1][i])
            want = T.ref_keys(list(per) + [None] * (R - len(per)), n, out["Lr"])
            assert out["keys"][n - 1][i] == want, ("keys", n, i)
    want_cider = T.cider_scores(hyps, refs)
    for i in range(N):
        assert _close(out["cider"][i], want_cider[i]), ("cider", i, out["cider"][i], want_cider[i])
    assert _close(out["means"][1], T.mean(want_cider))


def test_every_length_pair(dev):
    hyps, refs = T.length_corpus()
    _check(_run(dev, hyps, refs), hyps, refs)


def test_corner_cases(dev):
    hyps, refs = T.corner_corpus()
    out = _run(dev, hyps, refs)
    _check(out, hyps, refs)
    assert out["stats"][0][0:4] == [3, 2, 1, 0] and out["stats"][1][9] == 4 and out["stats"][5][9] == 0
    assert out["cider"][5] == 0.0 and out["rouge"][5] == 0.0 and out["lcs"][5] == [0, 0, 0, 0, 0]
    assert T.key_of((T.CIDER_MAX_TOKEN,) * 4) in out["tables"][3][0] and T.SENTINEL not in out["tables"][3][0]
    assert out["tables"][2][1][out["tables"][2][0].index(T.key_of((7, 1, 2)))] == 3
    n_with_7 = out["tables"][0][1][out["tables"][0][0].index(T.key_of((7,)))]
    assert n_with_7 == 8                             # every image with a present reference holds token 7: its idf is log(9/8)


def test_unigram_in_every_image_has_idf_zero(dev):
    hyps, refs = [[7, 1], [7, 2], [7, 3]], [[[7, 1, 4]], [[7, 2, 5]], [[6, 7]]]
    out = _run(dev, hyps, refs)
    _check(out, hyps, refs)
    only7 = _run(dev, [[7], [7], [7]], refs)
    assert only7["cider"] == [0.0, 0.0, 0.0]         # the only shared n-gram has idf log 3 - log 3 = 0 exactly: norms 0, no NaN


def test_skip_lists(dev):
    hyps, refs, sh, sr = T.skip_corpus()
    sh_, sr_ = T.stripped(hyps, refs, sh, sr)
    _check(_run(dev, hyps, refs, sh, sr), sh_, sr_)
    four = _run(dev, hyps, refs, (90, 91, 0, 6), (90, 0, 91, 6))
    _check(four, *T.stripped(hyps, refs, (90, 91, 0, 6), (90, 0, 91, 6)))


@pytest.mark.parametrize("n_img", (1, 2))
def test_one_and_two_images(dev, n_img):
    hyps, refs = [[1, 2], [3]][:n_img], [[[1, 2]], [[1, 3]]][:n_img]
    out = _run(dev, hyps, refs)
    _check(out, hyps, refs)
    if n_img == 1:
        assert out["cider"] == [0.0] and out["means"][1] == 0.0             # exactly 0, not NaN
    else:
        assert abs(out["cider"][0] - 5.0) <= 1e-12 and abs(out["cider"][1] - 2.5 * math.exp(-1 / 72)) <= 1e-12


@pytest.mark.parametrize("vocab,cpi", ((12, 5), (10000, 5), (12, 1)))
def test_random_corpora(dev, vocab, cpi):
    hyps, refs = T.random_corpus(7 + vocab + cpi, 70, vocab, cpi=cpi)
    _check(_run(dev, hyps, refs), hyps, refs)


def test_token_range_flag_and_unlimited_bleu_rouge(dev):
    big = T.CIDER_MAX_TOKEN + 1
    hyps, refs = [[1, 2, 3], [4, 5]], [[[1, 2, 3], [2, 3]], [[4, 5, 6], [5]]]
    h_bad = [[1, big, 3], [4, 5]]
    out = _run(dev, h_bad, refs)
    _check(out, h_bad, refs, flags=(0, 0, 0, 0, 1))                          # references fine, the hypothesis is not
    r_bad = [[[1, 2, 3], [2, -3]], [[4, 5, 6], [2 ** 31 - 1]]]
    out = _run(dev, hyps, r_bad)
    _check(out, hyps, r_bad, flags=(1, 1, 1, 1, 1))                          # integers and ROUGE-L still exact
    ok = _run(dev, [[T.CIDER_MAX_TOKEN, 0]], [[[T.CIDER_MAX_TOKEN, 0]]])
    assert ok["flags"] == [0, 0, 0, 0, 0]


def test_scorer_raises_on_the_flag(dev):
    from scnattn import textmetrics as TM
    with pytest.raises(ValueError):
        TM.CaptionScorer([[[1, 70000]]], device=dev)
    s = TM.CaptionScorer([[[1, 2]]], device=dev)
    with pytest.raises(ValueError):
        s.score([[1, 65535]])


def test_memory_lengths_are_clamped(dev):
    hyps, refs = [[1, 2, 3, 4, 5, 6], [1, 2, 3, 0, 0, 0]], [[[1, 2, 3, 4], [2, 3, 4, 5]], [[1, 2, 0, 0], [3, 0, 0, 0]]]
    out = _run(dev, hyps, refs, hyp_len=[1000, 2 ** 31 - 1], ref_len=[[4, 77], [129, 4]])
    _check(out, hyps, refs)                          # every row counts in full: lengths clamp to the padded widths 6 and 4
    out = _run(dev, hyps, refs, hyp_len=[-5, 3], ref_len=[[4, 4], [2, 1]])
    _check(out, [[], [1, 2, 3]], [refs[0], [[1, 2], [3]]])                  # a negative hypothesis length is an empty one


def test_width_129_is_refused_with_device_pointers(dev):
    from scnattn import _lib as L
    t = torch.zeros(2, 129, dtype=torch.int32, device=dev)
    n = torch.zeros(2, dtype=torch.int32, device=dev)
    out = torch.full((2, 10), -7, dtype=torch.int32, device=dev)
    h = L.lib()
    assert h.scnattn_text_ngram_stats(L.stream_of(t), 2, 1, L.ptr(t), 129, L.ptr(n), L.ptr(t), 128, L.ptr(n), None, 0, None, 0,
                                      L.ptr(out)) == -1
    assert h.scnattn_text_ngram_stats(L.stream_of(t), 2, 1, L.ptr(t), 128, L.ptr(n), L.ptr(t), 129, L.ptr(n), None, 0, None, 0,
                                      L.ptr(out)) == -1
    assert "padded width" in h.scnattn_last_error().decode()
    assert int((out != -7).sum()) == 0               # nothing ran
