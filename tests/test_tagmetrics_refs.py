"""CPU-only tests of the tagger-evaluation restatement (tests/tagmetrics_refs.py) and of the host side of csrc/tagmetrics.hip.

1. The restatement reproduces tests/golden/tagmetrics_sklearn.json (scikit-learn 1.7.2, tools/make_tagmetrics_golden.py) within
   1e-12: average_precision_score per tag and macro, label_ranking_average_precision_score, micro / macro precision, recall and
   F1 at 0.5.  Where scikit-learn is installed, the same on fresh random cases with heavy ties.
2. The exact (Fraction) form and the fp64 form of AP agree within the derived bound (m + 2) * 2^-53; AP does not depend on the
   order of ties; hits@k by sorting equals hits@k by the rank definition.
3. Examples small enough for paper.
4. The library: the four new symbols are declared, exported and bound; the header's limits equal scnattn._lib's; every refusal
   the issue names returns -1 with its message before anything reaches a GPU; TagScorer refuses its arguments likewise."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import tagmetrics_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("scnattn_tag_store_size", "scnattn_tag_rows", "scnattn_tag_cols", "scnattn_tag_finalize")


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "tagmetrics_sklearn.json")) as fh:
        return json.load(fh)["cases"]


def _f(pair):
    return float(pair[0])


def test_restatement_reproduces_the_recorded_sklearn_values():
    cases = _golden()
    assert len(cases) == 5 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "tagmetrics_sklearn.json")) < 64 * 1024
    for c in cases:
        p, t = T.decode_golden(c)
        assert p.shape == (c["n"], c["S"]) and c["n"] * c["S"] <= 64 * 65
        assert all(0 < x < c["n"] for x in t.sum(0)) and all(0 < x < c["S"] for x in t.sum(1))
        ref = T.reference(p, t)
        for s, want in enumerate(c["ap_per_tag"]):
            assert abs(float(ref["col_ap"][s]) - want) <= 1e-12, (c["name"], s)
        sm = ref["summary"]
        assert abs(_f(sm["map_tags"]) - c["ap_macro"]) <= 1e-12 and abs(_f(sm["ap_images"]) - c["lrap"]) <= 1e-12
        for r in range(3):
            assert abs(_f(sm["micro", 0][r]) - c["prf_micro"][r]) <= 1e-12, (c["name"], "micro", r)
            assert abs(_f(sm["macro", 0][r]) - c["prf_macro"][r]) <= 1e-12, (c["name"], "macro", r)


def test_restatement_reproduces_sklearn_on_fresh_cases():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(7)
    for n, S, quant in ((6, 9, 3), (15, 8, 0), (31, 40, 5), (40, 13, 2)):
        while True:
            p, t = T._random(rng, n, S, rate=0.3, quant=quant)
            if all(0 < x < n for x in t.sum(0)) and all(0 < x < S for x in t.sum(1)):
                break
        ref = T.reference(p, t)
        want = sk.average_precision_score(t, p, average=None)
        assert max(abs(float(ref["col_ap"][s]) - want[s]) for s in range(S)) <= 1e-12
        assert abs(_f(ref["summary"]["ap_images"]) - sk.label_ranking_average_precision_score(t, p)) <= 1e-12
        pred = (p >= np.float32(0.5)).astype(np.uint8)
        for avg in ("micro", "macro"):
            got = [_f(x) for x in ref["summary"][avg, 0]]
            assert np.allclose(got, sk.precision_recall_fscore_support(t, pred, average=avg, zero_division=0)[:3], rtol=0, atol=1e-12)


def test_fraction_and_fp64_forms_agree_within_the_derived_bound():
    rng = np.random.default_rng(11)
    for S, rate, quant in ((1, 1.0, 0), (65, 0.3, 4), (1000, 0.01, 0), (1000, 0.5, 8), (300, 1.0, 2)):
        p, t = T._random(rng, 1, S, rate=rate, quant=quant)
        pos = T.positives(t[0])
        m = int(pos.sum())
        if m == 0:
            assert T.ap_exact(p[0], pos) is None and T.ap_float(p[0], pos) is None
            continue
        assert T.close(T.ap_float(p[0], pos), T.ap_exact(p[0], pos), (m + 2) * T.U)
        perm = rng.permutation(S)                                       # tie-invariant: any order of the entries
        assert T.ap_exact(p[0][perm], pos[perm]) == T.ap_exact(p[0], pos)
        for k in (1, 3, m, S, S + 3):
            assert T.hits_at(p[0], pos, k) == T.hits_at_by_definition(p[0], pos, k)


def test_by_hand():
    s = np.array([0.9, 0.5, 0.5, 0.1], dtype=np.float32)
    pos = np.array([0, 0, 1, 0], dtype=bool)
    assert T.ap_counts(s, pos) == [(1, 3)] and T.ap_exact(s, pos) == Fraction(1, 3)
    assert T.hits_at(s, pos, 2) == 0 and T.hits_at(s, pos, 3) == 1                      # the tie goes to index 1
    assert T.hits_at(s, np.array([0, 1, 0, 0], dtype=bool), 2) == 1
    pos = np.array([1, 0, 1, 1], dtype=bool)
    # terms: index 0: 1/1; index 2: 2 of the 3 entries >= 0.5; index 3: 3/4
    assert T.ap_exact(s, pos) == (Fraction(1) + Fraction(2, 3) + Fraction(3, 4)) / 3
    ref = T.reference(np.array([[0.9, 0.2], [0.5, 0.6], [0.4, 0.7]], dtype=np.float32),
                      np.array([[1.0, 0.49], [0.5, 0.0], [0.0, 0.2]], dtype=np.float32), ks=(1, 5), thresholds=(0.5, 0.45))
    assert ref["row_npos"].tolist() == [1, 1, 0] and ref["col_npos"].tolist() == [2, 0]
    assert ref["row_ap"] == [Fraction(1), Fraction(1, 2), None] and ref["col_ap"] == [Fraction(1), None]
    assert ref["row_hits"].tolist() == [[1, 1], [0, 1], [0, 0]]                         # k = 5 is clamped to S = 2
    assert ref["col_counts"].tolist() == [[[2, 0, 0], [2, 0, 0]], [[0, 2, 0], [0, 2, 0]]]
    assert ref["n_images_empty"] == 1 and ref["n_tags_empty"] == 1 and ref["binary_accuracy"] == 100.0 * 4 / 6
    sm = ref["summary"]
    assert sm["map_tags"][0] == 1 and sm["ap_images"][0] == Fraction(3, 4)
    assert sm["precision_at", 1][0] == Fraction(1, 2) and sm["recall_at", 0][0] == Fraction(1, 2)
    assert [x for x, _ in sm["micro", 0]] == [Fraction(1, 2), Fraction(1), Fraction(2, 3)]
    assert [x for x, _ in sm["macro", 0]] == [Fraction(1), Fraction(1), Fraction(1)]     # over the one tag with a positive
    empty = T.reference(np.zeros((2, 3), dtype=np.float32), np.zeros((2, 3), dtype=np.uint8))
    assert empty["summary"]["map_tags"] == (None, None) and empty["binary_accuracy"] == 100.0


def test_fp64_restatement_agrees_with_the_exact_one():
    cs = {c["name"]: c for c in T.cases()}
    for name in ("n257", "ties_quarters_rows", "degenerate_none", "k_values", "threshold_boundary", "eight_thresholds"):
        c = cs[name]
        ref = T.reference(c["probs"], c["targets"], c["ks"], c["thresholds"])
        got = T.reference_fp64(c["probs"], c["targets"], c["ks"], c["thresholds"])
        sm = ref["summary"]
        assert T.close(got["map_tags"], *sm["map_tags"]) and T.close(got["ap_images"], *sm["ap_images"])
        for q, k in enumerate(c["ks"]):
            assert T.close(got["precision_at"][k], *sm["precision_at", q]) and T.close(got["recall_at"][k], *sm["recall_at", q])
        for t, th in enumerate(c["thresholds"]):
            d = got["threshold_%g" % th]
            for r, key in enumerate(("precision", "recall", "f1")):
                assert T.close(d["micro_" + key], *sm["micro", t][r]) and T.close(d["macro_" + key], *sm["macro", t][r])
        assert got["binary_accuracy"] == ref["binary_accuracy"]
        assert (got["n_images_empty"], got["n_tags_empty"]) == (ref["n_images_empty"], ref["n_tags_empty"])
    nothing = T.reference_fp64(np.zeros((2, 3), dtype=np.float32), np.zeros((2, 3), dtype=np.uint8))
    assert nothing["map_tags"] != nothing["map_tags"] and nothing["n_images_empty"] == 2 and nothing["n_tags_empty"] == 3


def test_case_list_covers_what_it_names():
    cs = {c["name"]: c for c in T.cases()}
    assert len(cs) == len(T.cases())
    assert {c["probs"].shape[1] for c in cs.values()} >= {1, 2, 63, 64, 65, 127, 256, 257, 1000, 1001, 1024, 1025, 4096}
    assert {c["probs"].shape[0] for c in cs.values()} >= {1, 3, 7, 255, 256, 257, 1025}
    assert cs["n7"]["batches"] == [3, 3, 1] and cs["n1025"]["batches"] == [512, 512, 1]
    assert T.positives(cs["n1025"]["targets"])[:, 3].all() and not T.positives(cs["n1025"]["targets"])[:, 4].any()
    d = T.positives(cs["degenerate_none"]["targets"])
    assert not d[1].any() and not d[:, 7].any()
    d = T.positives(cs["degenerate_full"]["targets"])
    assert d[4].all() and d[:, 9].all()
    assert len(np.unique(cs["ties_all_equal"]["probs"])) == 1 and set(np.unique(cs["ties_saturated"]["probs"])) == {0.0, 1.0}
    assert set(np.unique(cs["ties_quarters_rows"]["probs"])) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    b = cs["threshold_boundary"]
    assert (b["probs"] == np.float32(0.5)).any() and (b["probs"] == np.float32(0.3)).any()
    f, u = cs["targets_fp32"], cs["targets_u8_of_the_same"]
    assert f["targets"].dtype == np.float32 and u["targets"].dtype == np.uint8 and np.array_equal(f["probs"], u["probs"])
    assert T.positives(f["targets"])[0, :4].tolist() == [True, True, False, False]
    assert np.array_equal(T.positives(f["targets"]), u["targets"] != 0)
    k = cs["k_values"]
    assert k["ks"] == (1, 3, 6, 25) and T.positives(k["targets"]).sum(1).tolist() == [3, 3, 3] and k["probs"].shape[1] == 20
    r = T.reference(cs["k_tie_at_the_cut"]["probs"], cs["k_tie_at_the_cut"]["targets"], ks=(2, 1, 3))
    assert r["row_hits"].tolist() == [[0, 0, 1], [1, 0, 1]]
    assert cs["row_stride"]["ld"] > cs["row_stride"]["probs"].shape[1]
    assert len(cs["eight_thresholds"]["thresholds"]) == 8 and cs["no_thresholds"]["thresholds"] == ()


def test_new_symbols_are_exported_and_declared():
    from scnattn import _lib as L
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    declared = set(re.findall(r"\b(scnattn_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and name in L._SIGS and hasattr(L.lib(), name), name
    for macro, value in (("MAX_S", L.TAG_MAX_S), ("MAX_K", L.TAG_MAX_K), ("MAX_THRESHOLDS", L.TAG_MAX_THRESHOLDS),
                         ("MAX_IMAGES", L.TAG_MAX_IMAGES), ("SUMMARY_LEN", L.TAG_SUMMARY_LEN)):
        assert int(re.search(r"#define SCNATTN_TAG_%s (\d+)" % macro, header).group(1)) == value
    assert (L.TAG_MAX_S, L.TAG_MAX_K, L.TAG_MAX_THRESHOLDS, L.TAG_SUMMARY_LEN) == (T.MAX_S, T.MAX_K, T.MAX_T, T.SUMMARY_LEN)
    sb, lb = C.c_size_t(), C.c_size_t()
    assert L.lib().scnattn_tag_store_size(1000, 40000, C.byref(sb), C.byref(lb)) == 0
    assert (sb.value, lb.value) == (1000 * 40000 * 4, 1000 * 40000)


def test_argument_validation_returns_error_codes_without_a_gpu():
    """nothing below reaches a launch: every call is refused on its arguments, the buffers are host dummies"""
    from scnattn import _lib as L
    h = L.lib()
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)
    ks = (C.c_int32 * 8)(1, 2, 3, 4, 5, 6, 7, 8)
    th = (C.c_float * 9)(*([0.5] * 9))
    sb = C.c_size_t()

    def rows(B=2, S=8, probs=p, ldp=8, ldt=8, row0=0, cap=4, ks_=ks, nk=4, flag=p):
        return h.scnattn_tag_rows(None, B, S, probs, ldp, p, 0, ldt, row0, cap, ks_, nk, p, p, p, p, p, flag)

    def cols(S=8, n=2, cap=4, nt=1, th_=th, out=p):
        return h.scnattn_tag_cols(None, S, n, cap, p, p, th_, nt, out, p, p, p)

    def fin(S=8, n=2, nk=4, nt=1, out=p):
        return h.scnattn_tag_finalize(None, S, n, ks, nk, nt, p, p, p, p, p, p, p, p, out)

    cases = [
        (lambda: rows(S=4097, ldp=4097, ldt=4097), "S outside"), (lambda: rows(S=0), "S outside"),
        (lambda: rows(nk=5), "values of k"), (lambda: rows(ks_=(C.c_int32 * 4)(1, 0, 2, 3)), "k < 1"),
        (lambda: rows(row0=3, B=2), "exceeds the capacity"), (lambda: rows(B=5), "exceeds the capacity"),
        (lambda: rows(cap=0), "capacity outside"), (lambda: rows(ldp=7), "leading dimension"),
        (lambda: rows(ldt=7), "leading dimension"), (lambda: rows(probs=None), "null pointer"),
        (lambda: rows(flag=None), "null pointer"), (lambda: rows(B=-1), "B < 0"),
        (lambda: cols(nt=9), "thresholds"), (lambda: cols(S=4097), "S outside"), (lambda: cols(n=5), "more images"),
        (lambda: cols(n=0), "no images"), (lambda: cols(out=None), "null pointer"), (lambda: cols(nt=1, th_=None), "thresholds"),
        (lambda: fin(nk=5), "values of k"), (lambda: fin(nt=9), "thresholds"), (lambda: fin(S=4097), "S outside"),
        (lambda: fin(n=0), "no images"), (lambda: fin(out=None), "null pointer"),
        (lambda: h.scnattn_tag_store_size(4097, 10, C.byref(sb), C.byref(sb)), "S outside"),
        (lambda: h.scnattn_tag_store_size(10, (1 << 30) + 1, C.byref(sb), C.byref(sb)), "capacity outside"),
        (lambda: h.scnattn_tag_store_size(10, 10, None, C.byref(sb)), "null pointer"),
    ]
    for call, text in cases:
        assert call() == -1, text
        msg = h.scnattn_last_error().decode()
        assert text in msg and "invalid argument" in msg, (text, msg)


def test_tagscorer_refuses_its_arguments_before_touching_a_device():
    from scnattn.tagmetrics import TagScorer
    for kw in (dict(semantic_size=4097, capacity=4), dict(semantic_size=0, capacity=4), dict(semantic_size=8, capacity=0),
               dict(semantic_size=8, capacity=4, ks=(1, 2, 3, 4, 5)), dict(semantic_size=8, capacity=4, ks=(0,)),
               dict(semantic_size=8, capacity=4, thresholds=(0.1,) * 9)):
        with pytest.raises(ValueError):
            TagScorer(device="cpu", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TagScorer(8, 4, device="cpu")
