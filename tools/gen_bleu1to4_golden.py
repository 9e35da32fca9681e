"""Golden BLEU-1..4 values and the integer statistics behind them, from NLTK itself:

    /opt/conda/bin/python3.9 tools/gen_bleu1to4_golden.py        # -> tests/golden/bleu_nltk_1to4.json

NLTK is not importable by the project interpreter; the second interpreter of the image (nltk 3.6.5) has it.  Per case the
file holds the corpus, ``corpus_bleu`` at the uniform weights of orders 1..4 (no smoothing), and per hypothesis NLTK's
``modified_precision`` numerators and denominators of orders 1..4 and ``closest_ref_length`` -- what
tests/test_textmetrics_refs.py holds the restatements of tests/textmetrics_refs.py to."""
import json
import os
import random
import sys
import warnings

import nltk
from nltk.translate.bleu_score import closest_ref_length, corpus_bleu, modified_precision

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from textmetrics_refs import make_case  # noqa: E402

WEIGHTS = [(1.0,), (0.5, 0.5), (1.0 / 3, 1.0 / 3, 1.0 / 3), (0.25, 0.25, 0.25, 0.25)]


def main():
    rng = random.Random(20261019)
    corpora = [make_case(rng, *spec) for spec in
               [(1, 12, 1, 8, 8, 0.0), (5, 30, 5, 4, 14, 0.2), (20, 50, 5, 3, 20, 0.4), (30, 12, 5, 8, 22, 0.25),
                (8, 10, 3, 1, 5, 0.5), (3, 1000, 5, 6, 9, 1.0), (10, 20, 5, 1, 3, 0.3), (40, 10000, 5, 8, 22, 0.25)]]
    corpora += [([[[1, 2, 3, 4, 5, 6, 7, 8]]], [[1, 2, 3, 4, 5, 6, 7, 8]]),
                ([[[1, 2, 3, 4, 5, 6, 7, 8]]], [[9, 9, 9, 9]]),
                ([[[1, 2, 3, 4], [1, 2, 3, 4, 5, 6]]], [[1, 2, 3, 4, 5]]),
                ([[[1, 2, 3, 4, 5, 6, 7]]], [[1, 2, 3]]),
                ([[[1, 2, 2, 2, 3]], [[4, 5, 6, 7, 8, 9]]], [[2, 2, 2, 2, 2], [4, 5, 6, 7, 8, 9]])]
    cases = []
    for refs, hyps in corpora:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bleu = [float(corpus_bleu(refs, hyps, weights=w)) for w in WEIGHTS]
        num, den, closest = [], [], []
        for r, h in zip(refs, hyps):
            p = [modified_precision(r, h, n) for n in range(1, 5)]
            num.append([int(x.numerator) for x in p])
            den.append([int(x.denominator) for x in p])
            closest.append(int(closest_ref_length(r, len(h))))
        cases.append({"references": refs, "hypotheses": hyps, "bleu": bleu, "numerators": num, "denominators": den,
                      "closest_ref_length": closest})
    out = {"generator": "nltk %s corpus_bleu / modified_precision / closest_ref_length, no smoothing" % nltk.__version__,
           "cases": cases}
    with open(os.path.join(ROOT, "tests", "golden", "bleu_nltk_1to4.json"), "w") as fh:
        json.dump(out, fh)
    print("wrote %d cases" % len(cases), [[round(b, 6) for b in c["bleu"]] for c in cases])


if __name__ == "__main__":
    main()
