"""GPU tests (``-m gpu``) of csrc/tagmetrics.hip through the C ABI, against the exact restatement of tests/tagmetrics_refs.py.

Bars (derived in tagmetrics_refs, no case exempt).  Integers -- npos, hits@k, tp / fp / fn, agree, the n_* counts -- equal the
restatement.  An AP over m positives lies within (m + 2) * 2^-53 of the exact rational value; a mean over c values within
(c + 2) * 2^-53 on top of its inputs' bounds; binary_accuracy has the bits of 100.0 * agree / (n * S).  Every case is run
twice, and once more in ONE batch when it comes in several: result arrays, summary and the tag-major store must be the same
bits each time.  The arrays are allocated three rows / columns longer than needed and pre-filled: what lies beyond n must
keep its filling.

Cases (tagmetrics_refs.cases): S = 1, 2, 63, 64, 65, 127, 256 | 257 and 1024 | 1025 (the row kernel's register counts), 1000,
1001, 4096; B = 1, 3; batches 3 + 3 + 1, 17 + 16 + 7 (the 16-image tile); n = 1, 255, 256, 257, 1025 (the column kernel's
chunk of 256 and its 512 staged positives); scores in quarters, all equal, saturated 0 / 1; scores exactly at 0.5 and at
fp32(0.3) with those thresholds; rows / tags without and with only positives; k = 1, npos, > npos, >= S and a tie at the cut;
uint8 and fp32 targets (0.49 | 0.5); a row stride above S; eight thresholds, none, no k.  Then the sklearn-recorded cases of
tests/golden/tagmetrics_sklearn.json, and bad scores (NaN, 1.5, inf, a negative one) raising the flag."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import tagmetrics_refs as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.cases()
PAD = 3
NAMES = ("row_ap", "row_npos", "row_hits", "col_ap", "col_npos", "col_counts", "col_agree", "summary", "store_scores", "store_labels")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def run_abi(dev, probs, targets, batches, ks, thresholds, ld=None):
    """the three kernels over one case; everything downloaded as numpy arrays (the padding included)"""
    from scnattn import _lib as L
    n, S = probs.shape
    cap = n + PAD
    nk, nt = len(ks), len(thresholds)
    ks_c = (C.c_int32 * max(1, nk))(*ks)
    th_c = (C.c_float * max(1, nt))(*thresholds)
    sb, lb = C.c_size_t(), C.c_size_t()
    L.call("scnattn_tag_store_size", S, cap, C.byref(sb), C.byref(lb))
    assert (sb.value, lb.value) == (4 * S * cap, S * cap)
    t = dict(store_scores=torch.full((S, cap), -3.0, device=dev), store_labels=torch.full((S, cap), 9, dtype=torch.uint8, device=dev),
             row_ap=torch.full((cap,), -3.0, dtype=torch.float64, device=dev),
             row_npos=torch.full((cap,), -3, dtype=torch.int32, device=dev),
             row_hits=torch.full((cap, max(1, nk)), -3, dtype=torch.int32, device=dev),
             col_ap=torch.full((S + PAD,), -3.0, dtype=torch.float64, device=dev),
             col_npos=torch.full((S + PAD,), -3, dtype=torch.int32, device=dev),
             col_counts=torch.full((S + PAD, max(1, nt), 3), -3, dtype=torch.int32, device=dev),
             col_agree=torch.full((S + PAD,), -3, dtype=torch.int32, device=dev),
             summary=torch.full((T.SUMMARY_LEN + PAD,), -3.0, dtype=torch.float64, device=dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = L.stream_of(flag)
    row0 = 0
    for B in batches:
        p, g = probs[row0:row0 + B], targets[row0:row0 + B]
        if ld is not None:      # a column slice of a wider tensor; what lies beside it would raise the flag if it were read
            wide_p = np.full((B, ld), 7.0, dtype=np.float32)
            wide_g = np.full((B, ld), 1, dtype=targets.dtype)
            wide_p[:, :S], wide_g[:, :S] = p, g
            p, g = wide_p, wide_g
        pd, gd = torch.from_numpy(np.ascontiguousarray(p)).to(dev), torch.from_numpy(np.ascontiguousarray(g)).to(dev)
        L.call("scnattn_tag_rows", st, B, S, L.ptr(pd), pd.stride(0), L.ptr(gd), int(gd.dtype == torch.uint8), gd.stride(0), row0,
               cap, ks_c, nk, L.ptr(t["store_scores"]), L.ptr(t["store_labels"]), L.ptr(t["row_ap"]), L.ptr(t["row_npos"]),
               L.ptr(t["row_hits"]), L.ptr(flag))
        row0 += B
    assert row0 == n
    L.call("scnattn_tag_cols", st, S, n, cap, L.ptr(t["store_scores"]), L.ptr(t["store_labels"]), th_c, nt, L.ptr(t["col_ap"]),
           L.ptr(t["col_npos"]), L.ptr(t["col_counts"]), L.ptr(t["col_agree"]))
    L.call("scnattn_tag_finalize", st, S, n, ks_c, nk, nt, L.ptr(t["row_ap"]), L.ptr(t["row_npos"]), L.ptr(t["row_hits"]),
           L.ptr(t["col_ap"]), L.ptr(t["col_npos"]), L.ptr(t["col_counts"]), L.ptr(t["col_agree"]), L.ptr(flag),
           L.ptr(t["summary"]))
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["flag"] = int(flag.item())
    return out


def same_bits(a, b):
    return [k for k in NAMES if a[k].tobytes() != b[k].tobytes()]


def check(out, probs, targets, ks, thresholds):
    """padding untouched, the store holds the inputs tag-major, everything else as the restatement says"""
    n, S = probs.shape
    nk, nt = len(ks), len(thresholds)
    assert out["flag"] == 0
    assert (out["row_ap"][n:] == -3).all() and (out["row_npos"][n:] == -3).all() and (out["row_hits"][n:] == -3).all()
    assert (out["col_ap"][S:] == -3).all() and (out["col_npos"][S:] == -3).all() and (out["col_counts"][S:] == -3).all()
    assert (out["col_agree"][S:] == -3).all() and (out["summary"][T.SUMMARY_LEN:] == -3).all()
    assert (out["store_scores"][:, n:] == -3).all() and (out["store_labels"][:, n:] == 9).all()
    assert out["store_scores"][:, :n].tobytes() == np.ascontiguousarray(probs.T).tobytes()
    assert np.array_equal(out["store_labels"][:, :n], T.positives(targets).T.astype(np.uint8))
    ref = T.reference(probs, targets, ks, thresholds)
    got = dict(row_ap=out["row_ap"][:n], row_npos=out["row_npos"][:n], row_hits=out["row_hits"][:n, :nk], col_ap=out["col_ap"][:S],
               col_npos=out["col_npos"][:S], col_counts=out["col_counts"][:S, :nt], col_agree=out["col_agree"][:S],
               summary=out["summary"][:T.SUMMARY_LEN])
    bad = T.judge(got, ref, nk, nt)
    assert not bad, bad[:8]
    return ref


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_against_the_exact_restatement(dev, case):
    args = (case["probs"], case["targets"], case["batches"], case["ks"], case["thresholds"])
    out = run_abi(dev, *args, ld=case["ld"])
    check(out, case["probs"], case["targets"], case["ks"], case["thresholds"])
    again = run_abi(dev, *args, ld=case["ld"])
    assert not same_bits(out, again), "two runs differ"
    if len(case["batches"]) > 1:
        whole = run_abi(dev, case["probs"], case["targets"], [case["probs"].shape[0]], case["ks"], case["thresholds"], ld=case["ld"])
        assert not same_bits(out, whole), "one batch and %s differ" % (case["batches"],)


def test_uint8_and_fp32_targets_give_the_same_bits(dev):
    cs = {c["name"]: c for c in CASES}
    f, u = cs["targets_fp32"], cs["targets_u8_of_the_same"]
    a = run_abi(dev, f["probs"], f["targets"], f["batches"], f["ks"], f["thresholds"])
    b = run_abi(dev, u["probs"], u["targets"], u["batches"], u["ks"], u["thresholds"])
    assert not same_bits(a, b)


def test_recorded_sklearn_cases_through_the_kernels(dev):
    with open(os.path.join(ROOT, "tests", "golden", "tagmetrics_sklearn.json")) as fh:
        cases = json.load(fh)["cases"]
    assert len(cases) == 5
    for c in cases:
        p, t = T.decode_golden(c)
        n, S = p.shape
        out = run_abi(dev, p, t, T.split(n), (1, 5, 10, 20), (0.5,))
        check(out, p, t, (1, 5, 10, 20), (0.5,))
        v = out["summary"]
        assert np.abs(out["col_ap"][:S] - np.array(c["ap_per_tag"])).max() <= 1e-12, c["name"]
        assert abs(v[0] - c["ap_macro"]) <= 1e-12 and abs(v[1] - c["lrap"]) <= 1e-12, c["name"]
        assert np.abs(v[10:13] - np.array(c["prf_micro"])).max() <= 1e-12 and np.abs(v[13:16] - np.array(c["prf_macro"])).max() <= 1e-12


@pytest.mark.parametrize("value", (float("nan"), 1.5, float("inf"), -0.25), ids=("nan", "1.5", "inf", "negative"))
def test_a_score_outside_0_1_raises_the_flag(dev, value):
    rng = np.random.default_rng(3)
    p, t = T._random(rng, 5, 130, rate=0.2)
    assert run_abi(dev, p, t, [3, 2], (1, 5), (0.5,))["flag"] == 0
    p[3, 129] = value
    out = run_abi(dev, p, t, [3, 2], (1, 5), (0.5,))
    assert out["flag"] == 1 and out["summary"][62] == 1.0
    p[3, 129] = 1.0                                                     # -0.0, 0.0 and 1.0 are scores
    p[0, 0] = -0.0
    assert run_abi(dev, p, t, [3, 2], (1, 5), (0.5,))["flag"] == 0


def test_refusals_launch_nothing(dev):
    """capacity overflow, 5 k's, 9 thresholds, S = 4097: -1, a message, and the caller's arrays untouched"""
    from scnattn import _lib as L
    h = L.lib()
    S, cap = 8, 4
    p = torch.rand(3, S, device=dev)
    g = torch.zeros(3, S, dtype=torch.uint8, device=dev)
    store_s, store_l = torch.full((S, cap), -3.0, device=dev), torch.full((S, cap), 9, dtype=torch.uint8, device=dev)
    row_ap = torch.full((cap,), -3.0, dtype=torch.float64, device=dev)
    row_i = torch.full((cap, 8), -3, dtype=torch.int32, device=dev)
    col_d = torch.full((4100,), -3.0, dtype=torch.float64, device=dev)
    col_i = torch.full((4100 * 27,), -3, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    summary = torch.full((64,), -3.0, dtype=torch.float64, device=dev)
    st = L.stream_of(p)
    ks = (C.c_int32 * 5)(1, 2, 3, 4, 5)
    th = (C.c_float * 9)(*([0.5] * 9))

    def rows(B=3, S_=S, row0=0, nk=2):
        return h.scnattn_tag_rows(st, B, S_, L.ptr(p), max(S, S_), L.ptr(g), 1, max(S, S_), row0, cap, ks, nk, L.ptr(store_s),
                                  L.ptr(store_l), L.ptr(row_ap), L.ptr(row_i), L.ptr(row_i), L.ptr(flag))

    def cols(S_=S, n=3, nt=1):
        return h.scnattn_tag_cols(st, S_, n, cap, L.ptr(store_s), L.ptr(store_l), th, nt, L.ptr(col_d), L.ptr(col_i), L.ptr(col_i),
                                  L.ptr(col_i))

    def fin(S_=S, nk=2, nt=1):
        return h.scnattn_tag_finalize(st, S_, 3, ks, nk, nt, L.ptr(row_ap), L.ptr(row_i), L.ptr(row_i), L.ptr(col_d), L.ptr(col_i),
                                      L.ptr(col_i), L.ptr(col_i), L.ptr(flag), L.ptr(summary))

    for call, text in ((lambda: rows(row0=2), "exceeds the capacity"), (lambda: rows(nk=5), "values of k"),
                       (lambda: rows(S_=4097), "S outside"), (lambda: cols(nt=9), "thresholds"), (lambda: cols(S_=4097), "S outside"),
                       (lambda: cols(n=5), "more images"), (lambda: fin(nk=5), "values of k"), (lambda: fin(nt=9), "thresholds"),
                       (lambda: fin(S_=4097), "S outside")):
        assert call() == -1
        assert text in h.scnattn_last_error().decode()
    torch.cuda.synchronize()
    for x, fill in ((store_s, -3), (store_l, 9), (row_ap, -3), (row_i, -3), (col_d, -3), (col_i, -3), (summary, -3), (flag, 0)):
        assert bool((x == fill).all())
