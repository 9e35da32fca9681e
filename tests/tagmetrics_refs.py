"""numpy / Fraction restatement of the tagger-evaluation definitions of include/scnattn.h, the case list shared by the CPU and
GPU test modules, and the judges.

Definitions.  probs fp32 [n, S], targets fp32 or uint8 [n, S]; an entry is positive iff target >= 0.5.  Every comparison is
a comparison of the stored fp32 values.
  AP of a score vector s with labels t, m = #positives >= 1:
      AP = (1/m) * sum over positive i of TP(i) / N(i),  N(i) = #{j : s_j >= s_i},  TP(i) = #{j positive : s_j >= s_i}.
  It does not depend on the order of ties; it is sklearn's average_precision_score of a column and, for 0 < m < S,
  label_ranking_average_precision_score of a row.  m = 0: the row / tag is left out of every mean and counted as empty.
  hits@k of a row: positives among the top k, entry i being in the top k iff #{j : s_j > s_i} + #{j < i : s_j == s_i} < k (ties
  to the lower index); k clamped to S; precision@k = hits / k, recall@k = hits / npos.
  Per tag and threshold: tp, fp, fn with the prediction p >= fp32(threshold); P = tp / (tp + fp), R = tp / (tp + fn),
  F1 = 2 tp / (2 tp + fp + fn), 0 / 0 = 0.  Micro: from the counts summed over tags.  Macro: the mean of the per-tag values
  over the tags with a positive.  binary_accuracy = 100 * agree / (n * S) at 0.5.

`reference` computes every AP and every mean EXACTLY (fractions.Fraction).  Bounds of the judges, derived, not tuned:
  integers                        equal;
  an AP over m positives          (m + 2) * 2^-53: every term is <= 1 and correctly rounded (2^-53 each), a fixed-order sum of m
                                  such terms adds at most (m - 1) * 2^-53 * m, the division by m brings both to <= (m - 1) * 2^-53
                                  + 2^-53, and the division rounds once more;
  a mean over c values            (c + 2) * 2^-53 on top of the mean of its inputs' bounds (the same argument; a quotient
                                  hits / npos, tp / (tp + fp), ... is one correctly rounded value <= 1: 2^-53);
  micro P / R / F1                one correctly rounded quotient of exact integers: 2^-53;
  binary_accuracy                 the bits of the Python expression 100.0 * agree / (n * S).
No case is exempt."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
MAX_S, MAX_K, MAX_T, SUMMARY_LEN = 4096, 4, 8, 64


def positives(targets):
    t = np.asarray(targets)
    return (t != 0) if t.dtype == np.uint8 or t.dtype == np.bool_ else (t.astype(np.float32) >= np.float32(0.5))


def ap_counts(s, pos):
    """[(TP(i), N(i))] for the positives i in ascending index"""
    s = np.asarray(s, dtype=np.float32)
    idx = np.flatnonzero(pos)
    if idx.size == 0:
        return []
    ge = s[None, :] >= s[idx][:, None]
    N = ge.sum(1)
    TP = (ge & pos[None, :]).sum(1)
    return list(zip(TP.tolist(), N.tolist()))


def ap_exact(s, pos):
    c = ap_counts(s, pos)
    if not c:
        return None
    by_n = {}
    for tp, n in c:
        by_n[(tp, n)] = by_n.get((tp, n), 0) + 1
    return sum(Fraction(tp * k, n) for (tp, n), k in by_n.items()) / len(c)


def ap_float(s, pos):
    """the fp64 form of the kernels: one division per term, summed in ascending index, one division by m"""
    c = ap_counts(s, pos)
    if not c:
        return None
    acc = 0.0
    for tp, n in c:
        acc += float(tp) / float(n)
    return acc / float(len(c))


def hits_at(s, pos, k):
    s = np.asarray(s, dtype=np.float32)
    k = min(int(k), s.size)
    order = np.lexsort((np.arange(s.size), -s.astype(np.float64)))      # descending score, ascending index among equals
    return int(pos[order[:k]].sum())


def hits_at_by_definition(s, pos, k):
    s = np.asarray(s, dtype=np.float32)
    k = min(int(k), s.size)
    h = 0
    for i in np.flatnonzero(pos):
        rank = int((s > s[i]).sum()) + int((s[:i] == s[i]).sum())
        h += rank < k
    return h


def _q(a, b):
    return Fraction(a, b) if b else Fraction(0)


def _mean(vals, bounds):
    """exact mean and its bound; (None, None) over nothing"""
    c = len(vals)
    if c == 0:
        return None, None
    return sum(vals, Fraction(0)) / c, sum(bounds, Fraction(0)) / c + (c + 2) * U


def reference(probs, targets, ks=(1, 5, 10, 20), thresholds=(0.5,)):
    probs = np.asarray(probs, dtype=np.float32)
    n, S = probs.shape
    pos = positives(targets)
    ks_c = [min(int(k), S) for k in ks]
    out = {"n": n, "S": S}
    out["row_npos"] = pos.sum(1).astype(np.int64)
    out["row_ap"] = [ap_exact(probs[i], pos[i]) for i in range(n)]
    out["row_hits"] = np.array([[hits_at(probs[i], pos[i], k) for k in ks_c] for i in range(n)], dtype=np.int64).reshape(n, len(ks))
    out["col_npos"] = pos.sum(0).astype(np.int64)
    out["col_ap"] = [ap_exact(probs[:, s], pos[:, s]) for s in range(S)]
    counts = np.zeros((S, len(thresholds), 3), dtype=np.int64)
    for t, th in enumerate(thresholds):
        pred = probs >= np.float32(th)
        counts[:, t, 0] = (pred & pos).sum(0)
        counts[:, t, 1] = (pred & ~pos).sum(0)
        counts[:, t, 2] = (~pred & pos).sum(0)
    out["col_counts"] = counts
    agree = int(((probs >= np.float32(0.5)) == pos).sum())
    out["col_agree"] = ((probs >= np.float32(0.5)) == pos).sum(0).astype(np.int64)
    rows = [i for i in range(n) if out["row_npos"][i] > 0]
    tags = [s for s in range(S) if out["col_npos"][s] > 0]
    summ = {}
    summ["map_tags"] = _mean([out["col_ap"][s] for s in tags], [(int(out["col_npos"][s]) + 2) * U for s in tags])
    summ["ap_images"] = _mean([out["row_ap"][i] for i in rows], [(int(out["row_npos"][i]) + 2) * U for i in rows])
    for q, k in enumerate(ks_c):
        summ["precision_at", q] = _mean([Fraction(int(out["row_hits"][i, q]), k) for i in rows], [U] * len(rows))
        summ["recall_at", q] = _mean([Fraction(int(out["row_hits"][i, q]), int(out["row_npos"][i])) for i in rows],
                                     [U] * len(rows))
    for t in range(len(thresholds)):
        tp, fp, fn = (int(x) for x in counts[:, t].sum(0))
        summ["micro", t] = [(_q(tp, tp + fp), U), (_q(tp, tp + fn), U), (_q(2 * tp, 2 * tp + fp + fn), U)]
        per = [[_q(a, a + b), _q(a, a + c), _q(2 * a, 2 * a + b + c)] for a, b, c in
               ([int(x) for x in counts[s, t]] for s in tags)]
        summ["macro", t] = [_mean([p[r] for p in per], [U] * len(per)) for r in range(3)]
    out["summary"] = summ
    out["binary_accuracy"] = 100.0 * agree / (n * S)
    out["n_images_empty"] = n - len(rows)
    out["n_tags_empty"] = S - len(tags)
    return out


def reference_fp64(probs, targets, ks=(1, 5, 10, 20), thresholds=(0.5,)):
    """The same definitions in numpy and fp64 with the kernels' summation order, without the exact rationals: the host side of
    tools/tagmetrics_bench.py, and the shape of the dict TagScorer.result() returns."""
    probs = np.asarray(probs, dtype=np.float32)
    n, S = probs.shape
    pos = positives(targets)
    ks_c = [min(int(k), S) for k in ks]

    def mean(vals):
        acc = 0.0
        for v in vals:
            acc += v
        return acc / len(vals) if vals else float("nan")

    rows = [i for i in range(n) if pos[i].any()]
    tags = [s for s in range(S) if pos[:, s].any()]
    hits = np.zeros((n, len(ks_c)), dtype=np.int64)
    idx = np.arange(S)
    for i in rows:
        order = np.lexsort((idx, -probs[i].astype(np.float64)))
        top = np.cumsum(pos[i][order])
        hits[i] = [top[k - 1] for k in ks_c]
    npos = pos.sum(1)
    out = {"map_tags": mean([ap_float(probs[:, s], pos[:, s]) for s in tags]),
           "ap_images": mean([ap_float(probs[i], pos[i]) for i in rows]),
           "precision_at": {k: mean([float(hits[i, q]) / kc for i in rows]) for q, (k, kc) in enumerate(zip(ks, ks_c))},
           "recall_at": {k: mean([float(hits[i, q]) / float(npos[i]) for i in rows]) for q, k in enumerate(ks)}}

    def div(a, b):
        return float(a) / float(b) if b else 0.0

    for th in thresholds:
        pred = probs >= np.float32(th)
        tp, fp, fn = (pred & pos).sum(0), (pred & ~pos).sum(0), (~pred & pos).sum(0)
        a, b, c = int(tp.sum()), int(fp.sum()), int(fn.sum())
        out["threshold_%g" % th] = {
            "micro_precision": div(a, a + b), "micro_recall": div(a, a + c), "micro_f1": div(2 * a, 2 * a + b + c),
            "macro_precision": mean([div(tp[s], tp[s] + fp[s]) for s in tags]),
            "macro_recall": mean([div(tp[s], tp[s] + fn[s]) for s in tags]),
            "macro_f1": mean([div(2 * tp[s], 2 * tp[s] + fp[s] + fn[s]) for s in tags])}
    agree = int(((probs >= np.float32(0.5)) == pos).sum())
    out.update(binary_accuracy=100.0 * agree / (n * S), n_images=n, n_images_empty=n - len(rows), n_tags_empty=S - len(tags))
    return out


def close(got, exact, bound):
    """|got - exact| <= bound, in exact arithmetic; a mean over nothing must be NaN"""
    if exact is None:
        return got != got
    got = float(got)
    return got == got and abs(Fraction(got) - exact) <= bound


def judge(got, ref, nk, nt):
    """`got`: dict of numpy arrays row_ap [n], row_npos, row_hits [n, nk], col_ap [S], col_npos, col_counts [S, nt, 3],
    col_agree [S], summary [64].  Returns the list of failures (empty: passed)."""
    bad = []
    n, S = ref["n"], ref["S"]
    for name in ("row_npos", "row_hits", "col_npos", "col_counts", "col_agree"):
        if not np.array_equal(np.asarray(got[name], dtype=np.int64).reshape(ref[name].shape), ref[name]):
            bad.append(name)
    for name, npos in (("row_ap", ref["row_npos"]), ("col_ap", ref["col_npos"])):
        for i, ex in enumerate(ref[name]):
            g = float(got[name][i])
            if ex is None:
                if g != 0.0:
                    bad.append("%s[%d] of an empty one is %r" % (name, i, g))
            elif not close(g, ex, (int(npos[i]) + 2) * U):
                bad.append("%s[%d]: %r vs %r" % (name, i, g, float(ex)))
    v, sm = got["summary"], ref["summary"]
    checks = [("map_tags", v[0], sm["map_tags"]), ("ap_images", v[1], sm["ap_images"])]
    for q in range(nk):
        checks.append(("precision_at[%d]" % q, v[2 + q], sm["precision_at", q]))
        checks.append(("recall_at[%d]" % q, v[6 + q], sm["recall_at", q]))
    for t in range(nt):
        for r in range(3):
            checks.append(("micro[%d][%d]" % (t, r), v[10 + 6 * t + r], sm["micro", t][r]))
            checks.append(("macro[%d][%d]" % (t, r), v[13 + 6 * t + r], sm["macro", t][r]))
    for name, g, (ex, bound) in checks:
        if not close(g, ex, bound):
            bad.append("%s: %r vs %r" % (name, float(g), None if ex is None else float(ex)))
    if float(v[58]) != ref["binary_accuracy"]:
        bad.append("binary_accuracy: %r vs %r" % (float(v[58]), ref["binary_accuracy"]))
    if (int(v[59]), int(v[60]), int(v[61])) != (n, ref["n_images_empty"], ref["n_tags_empty"]):
        bad.append("n_images / n_images_empty / n_tags_empty: %r" % ([float(x) for x in v[59:62]],))
    if float(v[62]) != 0.0 or any(float(x) != 0.0 for x in v[63:]) or any(
            float(x) != 0.0 for q in range(nk, MAX_K) for x in (v[2 + q], v[6 + q])) or any(
            float(x) != 0.0 for x in v[10 + 6 * nt:58]):
        bad.append("flag or an unused summary entry is not 0")
    return bad


# ---- cases: the smallest shapes at which the kernels can go wrong -------------------------------------------------------------

def _case(name, probs, targets, batches=None, ks=(1, 5, 10, 20), thresholds=(0.5,), ld=None):
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    targets = np.ascontiguousarray(targets)
    assert probs.ndim == 2 and targets.shape == probs.shape and targets.dtype in (np.float32, np.uint8)
    n = probs.shape[0]
    batches = [n] if batches is None else list(batches)
    assert sum(batches) == n
    return dict(name=name, probs=probs, targets=targets, batches=batches, ks=tuple(ks), thresholds=tuple(thresholds), ld=ld)


def _random(rng, n, S, rate=0.1, quant=None):
    p = rng.random((n, S), dtype=np.float32)
    if quant:
        p = np.floor(p * (quant + 1)).clip(0, quant).astype(np.float32) / np.float32(quant)
    t = (rng.random((n, S)) < rate).astype(np.uint8)
    return p, t


def split(n):
    """n images as two equal batches and a short last one: 7 -> 3 + 3 + 1"""
    if n < 3:
        return [n]
    b = (n - 1) // 2
    return [b, b, n - 2 * b]


def cases():
    rng = np.random.default_rng(20240531)
    out = []
    # S: one lane, one register, the register-count steps (256 | 257, 1024 | 1025) and the maximum; B = 1 and 3
    for S in (1, 2, 63, 64, 65, 127, 256, 257, 1000, 1001, 1024, 1025, 4096):
        for B in (1, 3):
            p, t = _random(rng, B, S, rate=0.1 if S > 2 else 0.6)
            t[0, S // 2] = 1
            out.append(_case("S%d_B%d" % (S, B), p, t))
    # accumulation: 3 + 3 + 1, and n across the column kernel's chunk of 256
    for n in (1, 7, 255, 256, 257, 1025):
        p, t = _random(rng, n, 5, rate=0.3)
        t[:, 3] = 1                                                      # a tag all positive: 1025 > the 512 staged at a time
        t[:, 4] = 0                                                      # a tag never positive
        out.append(_case("n%d" % n, p, t, batches=split(n), ks=(1, 2, 5), thresholds=(0.5, 0.25)))
    p, t = _random(rng, 40, 65, rate=0.1)
    out.append(_case("n40_S65_tiles", p, t, batches=[17, 16, 7]))       # batches across the 16-image tile
    # ties
    p, t = _random(rng, 3, 127, rate=0.2, quant=4)
    out.append(_case("ties_quarters_rows", p, t))
    p, t = _random(rng, 257, 5, rate=0.3, quant=4)
    out.append(_case("ties_quarters_cols", p, t, batches=split(257), thresholds=(0.5, 0.25, 0.75)))
    p, t = _random(rng, 7, 65, rate=0.3)
    out.append(_case("ties_all_equal", np.full_like(p, 0.375), t, batches=[3, 3, 1]))
    p, t = _random(rng, 7, 65, rate=0.3, quant=1)
    out.append(_case("ties_saturated", p, t, batches=[3, 3, 1], thresholds=(0.5, 1.0, 0.0)))
    # threshold boundary: scores exactly at 0.5 (predicted) and at a second threshold that is not a binary fraction
    p, t = _random(rng, 9, 17, rate=0.4)
    p[::2, ::3] = 0.5
    p[1::2, 1::3] = np.float32(0.3)
    p[0, 1] = np.nextafter(np.float32(0.5), np.float32(0))
    p[0, 2] = np.nextafter(np.float32(0.3), np.float32(1))
    out.append(_case("threshold_boundary", p, t, thresholds=(0.5, 0.3)))
    # degenerate rows and tags
    p, t = _random(rng, 7, 65, rate=0.3)
    t[1, :] = 0
    t[:, 7] = 0
    out.append(_case("degenerate_none", p, t, batches=[3, 3, 1]))        # a row and a tag without a positive
    t = t.copy()
    t[4, :] = 1
    t[:, 9] = 1
    out.append(_case("degenerate_full", p, t, batches=[3, 3, 1]))        # and a row and a tag all positive
    out.append(_case("no_positive_at_all", p, np.zeros_like(t)))
    out.append(_case("all_positive", p, np.ones_like(t)))
    # k: 1, npos, above npos, >= S; and ties at the cut
    p, t = _random(rng, 3, 20, rate=0.0)
    t[:, [2, 5, 11]] = 1
    out.append(_case("k_values", p, t, ks=(1, 3, 6, 25)))
    p = np.array([[0.9, 0.5, 0.5, 0.1], [0.9, 0.5, 0.5, 0.1]], dtype=np.float32)
    t = np.array([[0, 0, 1, 0], [0, 1, 0, 0]], dtype=np.uint8)          # the positive on the higher index loses, on the lower wins
    out.append(_case("k_tie_at_the_cut", p, t, ks=(2, 1, 3)))
    # target types
    p, t = _random(rng, 5, 33, rate=0.3)
    tf = np.where(t != 0, np.float32(0.5), np.float32(0.49)).astype(np.float32)
    tf[0, :4] = [1.0, 0.51, 0.0, np.nextafter(np.float32(0.5), np.float32(0))]
    out.append(_case("targets_fp32", p, tf))
    out.append(_case("targets_u8_of_the_same", p, positives(tf).astype(np.uint8)))
    # a row stride above S
    p, t = _random(rng, 5, 65, rate=0.2)
    out.append(_case("row_stride", p, t, batches=[3, 2], ld=65 + 7))
    # eight thresholds, no k; and no threshold
    p, t = _random(rng, 6, 33, rate=0.3)
    out.append(_case("eight_thresholds", p, t, ks=(), thresholds=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)))
    out.append(_case("no_thresholds", p, t, ks=(3,), thresholds=()))
    return out


def decode_golden(case):
    """a case of tests/golden/tagmetrics_sklearn.json -> (probs fp32 [n, S], targets uint8 [n, S])"""
    n, S = case["n"], case["S"]
    if "probs_bits" in case:
        words = [int(row[8 * j:8 * j + 8], 16) for row in case["probs_bits"] for j in range(S)]
        p = np.array(words, dtype=np.uint32).view(np.float32).reshape(n, S)
    else:
        p = (np.array(case["probs_num"], dtype=np.float64) / case["probs_den"]).astype(np.float32).reshape(n, S)
    t = np.array([[int(c) for c in row] for row in case["targets"]], dtype=np.uint8).reshape(n, S)
    return p, t
