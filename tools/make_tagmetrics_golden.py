"""Writes tests/golden/tagmetrics_sklearn.json: tagger-evaluation cases scored by scikit-learn.

    python tools/make_tagmetrics_golden.py            (needs scikit-learn; recorded with 1.7.2)

Every row and every column of a case holds 0 < positives < size: only there do sklearn's conventions and the project's
coincide (sklearn counts a row without a positive as 1.0 in label_ranking_average_precision_score and gives a tag without a
positive 0 with a warning; the project leaves both out of its means).  The inputs are stored as exact values -- the fp32 bit
patterns, or small numerators over a power of two -- so that nothing depends on a random generator's version.  Recorded per
case: average_precision_score per tag and its macro mean, label_ranking_average_precision_score, and
precision_recall_fscore_support(average = 'micro' | 'macro', zero_division = 0) at the threshold 0.5."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tagmetrics_sklearn.json")


def draw(seed, n, S, rate, den):
    """the first draw from `seed` on whose rows and columns 0 < positives < size"""
    rng = np.random.default_rng(seed)
    while True:
        t = (rng.random((n, S)) < rate).astype(np.uint8)
        if den:
            p = (rng.integers(0, den + 1, size=(n, S)).astype(np.float64) / den).astype(np.float32)
        else:
            p = rng.random((n, S), dtype=np.float32)
        if all(0 < c < n for c in t.sum(0)) and all(0 < c < S for c in t.sum(1)):
            return p, t


def main():
    import sklearn
    from sklearn.metrics import average_precision_score, label_ranking_average_precision_score, precision_recall_fscore_support
    cases = []
    for name, seed, n, S, rate, den in (("quarters_7x5", 1, 7, 5, 0.4, 4), ("random_12x17", 2, 12, 17, 0.3, 0),
                                        ("random_20x33", 3, 20, 33, 0.2, 0), ("sixtyfourths_64x65", 4, 64, 65, 0.1, 64),
                                        ("halves_9x6", 5, 9, 6, 0.5, 2)):
        p, t = draw(seed, n, S, rate, den)
        c = {"name": name, "n": n, "S": S, "targets": ["".join(str(int(x)) for x in row) for row in t]}
        if den:
            c["probs_den"] = den
            c["probs_num"] = [[int(round(float(x) * den)) for x in row] for row in p]
        else:
            c["probs_bits"] = ["".join("%08x" % int(w) for w in row.view(np.uint32)) for row in p]
        pred = (p >= np.float32(0.5)).astype(np.uint8)
        c["ap_per_tag"] = [float(x) for x in average_precision_score(t, p, average=None)]
        c["ap_macro"] = float(average_precision_score(t, p, average="macro"))
        c["lrap"] = float(label_ranking_average_precision_score(t, p))
        for avg in ("micro", "macro"):
            pr, rc, f1, _ = precision_recall_fscore_support(t, pred, average=avg, zero_division=0)
            c["prf_" + avg] = [float(pr), float(rc), float(f1)]
        cases.append(c)
    with open(OUT, "w") as fh:
        json.dump({"sklearn": sklearn.__version__, "cases": cases}, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
