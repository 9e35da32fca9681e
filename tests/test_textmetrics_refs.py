"""CPU-only tests of the caption text metrics' host side and of the restatements the GPU tests compare against.

1. tests/textmetrics_refs.py against what is already pinned: its NLTK-form BLEU-4 / BLEU-2 equal utils.metric.corpus_bleu and
   every case of tests/golden/bleu_nltk.json to 1e-12; against tests/golden/bleu_nltk_1to4.json (tools/gen_bleu1to4_golden.py,
   NLTK 3.6.5) the tail holds at the four uniform weights to 1e-12 and the integer statistics equal NLTK's modified_precision
   numerators / denominators and closest_ref_length exactly.
2. Examples small enough for paper.
   ROUGE-L: hyp 1 2 3 4 against 1 3 4 5 6 and 2 4.  LCS = 3 (1 3 4) and 2 (2 4); P = max(3/4, 2/4) = 3/4, Rc = max(3/5, 2/2) = 1;
   score = 2.44 * 0.75 / (1 + 1.44 * 0.75) = 1.83 / 2.08.
   CIDEr-D: two images, so log N = ln 2.  Image A: reference 1 2, hypothesis 1 2; image B: reference 1 3, hypothesis 3.
   df: unigram 1 -> 2 (idf 0), 2 -> 1, 3 -> 1 (idf ln 2); bigrams (1 2), (1 3) -> 1 (idf ln 2).
   A: order 1: both vectors {1: 0, 2: ln 2}: dot = ln^2 2, norms ln 2 each -> 1; order 2: {(1 2): ln 2} both -> 1; orders 3, 4
   empty -> 0; equal lengths, penalty 1: score = (1 + 1 + 0 + 0) / 4 * 10 = 5.
   B: order 1: hyp {3: ln 2}, ref {1: 0, 3: ln 2}: dot = ln^2 2, norms ln 2 each -> 1, lengths 1 and 2: penalty exp(-1/72);
   no bigram in the hypothesis: score = exp(-1/72) / 4 * 10.  CIDEr = (5 + 2.5 exp(-1/72)) / 2.
   With image A alone N = 1, every idf is 0 and the score is exactly 0.
3. The library: the five new symbols are exported and declared, scnattn_text_max_len() == 128, the header's limits equal
   scnattn._lib's, and every argument-validation path returns -1 with its message without a GPU.  utils.metric.bleu_from_totals
   and scnattn.textmetrics.bleu_coco (the production tails) equal the restatements on the recorded corpora."""
import ctypes as C
import json
import math
import os
import random
import re

import pytest

import textmetrics_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("scnattn_text_max_len", "scnattn_text_ngram_stats", "scnattn_text_lcs", "scnattn_text_ref_keys", "scnattn_text_cider")
WEIGHTS = [(1.0,), (0.5, 0.5), (1.0 / 3, 1.0 / 3, 1.0 / 3), (0.25, 0.25, 0.25, 0.25)]


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)["cases"]


def test_nltk_form_equals_corpus_bleu_and_the_recorded_nltk_values():
    from utils.metric import corpus_bleu
    cases = _golden("bleu_nltk.json")
    assert len(cases) == 15
    for c in cases:
        refs, hyps = c["references"], c["hypotheses"]
        tot, den = T.corpus_totals(hyps, refs)
        b4 = T.bleu_nltk_tail(tot[0:4], den, tot[8], tot[9])
        b2 = T.bleu_nltk_tail(tot[0:2], den[0:2], tot[8], tot[9], weights=(0.5, 0.5))
        assert abs(b4 - c["bleu4"]) <= 1e-12 and abs(b2 - c["bleu2"]) <= 1e-12
        assert abs(b4 - corpus_bleu(refs, hyps)) <= 1e-12 and abs(b2 - corpus_bleu(refs, hyps, weights=(0.5, 0.5))) <= 1e-12


def test_statistics_and_tails_equal_nltk_1to4():
    from utils.metric import bleu_from_totals, corpus_bleu
    from scnattn.textmetrics import bleu_coco
    cases = _golden("bleu_nltk_1to4.json")
    assert len(cases) == 13
    for c in cases:
        refs, hyps = c["references"], c["hypotheses"]
        for h, r, num, den, closest in zip(hyps, refs, c["numerators"], c["denominators"], c["closest_ref_length"]):
            s = T.ngram_stats(h, r)
            assert s[0:4] == num and [max(1, g) for g in s[4:8]] == den and s[8] == len(h) and s[9] == closest
        tot, den = T.corpus_totals(hyps, refs)
        for w, want in zip(WEIGHTS, c["bleu"]):
            n = len(w)
            assert abs(T.bleu_nltk_tail(tot[0:n], den[0:n], tot[8], tot[9], weights=w) - want) <= 1e-12
            assert abs(bleu_from_totals(tot[0:n], den[0:n], tot[8], tot[9], w) - want) <= 1e-12
        assert bleu_from_totals(tot[0:4], den, tot[8], tot[9]) == corpus_bleu(refs, hyps)       # one tail: the same bits
        for a, b in zip(bleu_coco(tot[0:4], tot[4:8], tot[8], tot[9]), T.bleu_coco_tail(tot[0:4], tot[4:8], tot[8], tot[9])):
            assert a == b


def test_coco_form_by_hand():
    # hyp 1 2 3 4 5 against 1 2 3 9 5 6: correct 4, 2, 1, 0 of 5, 4, 3, 2 guesses; ratio 5/6 < 1
    tot, _ = T.corpus_totals([[1, 2, 3, 4, 5]], [[[1, 2, 3, 9, 5, 6]]])
    assert tot == [4, 2, 1, 0, 5, 4, 3, 2, 5, 6]
    b = T.bleu_coco_tail(tot[0:4], tot[4:8], tot[8], tot[9])
    bp = math.exp(1 - 6 / 5)
    assert abs(b[0] - 0.8 * bp) <= 1e-9 and abs(b[1] - math.sqrt(0.8 * 0.5) * bp) <= 1e-9
    assert abs(b[2] - (0.8 * 0.5 / 3) ** (1 / 3) * bp) <= 1e-9 and 0 < b[3] < 1e-3


def test_rouge_l_and_lcs_by_hand():
    ls, score = T.rouge_l([1, 2, 3, 4], [[1, 3, 4, 5, 6], [2, 4]])
    assert ls == [3, 2] and abs(score - 1.83 / 2.08) <= 1e-15
    assert T.lcs([], [1, 2]) == 0 and T.lcs([1, 2, 3], [3, 2, 1]) == 1 and T.lcs([1, 2, 1, 2], [2, 1, 2, 1]) == 3
    assert T.rouge_l([], [[1, 2]]) == ([0], 0.0) and T.rouge_l([1], [None, []]) == ([0, 0], 0.0)
    assert T.rouge_l([5, 6], [None, [5, 6]]) == ([0, 2], 1.0)


def test_cider_d_by_hand():
    hyps, refs = [[1, 2], [3]], [[[1, 2]], [[1, 3]]]
    df = T.cider_df(refs)
    assert df[0] == {(1,): 2, (2,): 1, (3,): 1} and df[1] == {(1, 2): 1, (1, 3): 1} and df[2] == {} and df[3] == {}
    a, b = T.cider_scores(hyps, refs)
    assert abs(a - 5.0) <= 1e-14 and abs(b - 2.5 * math.exp(-1 / 72)) <= 1e-14
    assert abs(T.score_all(hyps, refs)["CIDEr"] - (5 + 2.5 * math.exp(-1 / 72)) / 2) <= 1e-14
    assert T.cider_scores(hyps[:1], refs[:1]) == [0.0]                      # N = 1: exactly 0
    assert T.cider_scores([[]], [[[1, 2]]]) == [0.0] and T.cider_scores([[1]], [[None]]) == [0.0]


def test_keys_and_tables_of_the_restatement_agree():
    hyps, refs = T.corner_corpus()
    tables = T.df_tables(refs)
    for n in range(1, 5):
        flat = sorted(k for per in refs for row in T.ref_keys(per, n, 9) for k in row if k != T.SENTINEL)
        keys, df = tables[n - 1]
        assert sorted(set(flat)) == keys and [flat.count(k) for k in keys] == df
    big = T.key_of((T.CIDER_MAX_TOKEN,) * 4)
    assert big == -0x0001000100010002 and big != T.SENTINEL and big in tables[3][0]
    assert T.cider_df(refs)[0][(7,)] == sum(1 for per in refs if any(r and 7 in r for r in per))
    assert T.cider_df(refs)[2][(7, 1, 2)] == 3                                # images 2, 4, 6; image 6 holds it three times


def test_new_symbols_are_exported_and_declared():
    from scnattn import _lib as L
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    declared = set(re.findall(r"\b(scnattn_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(L.lib(), name), name
    assert L.lib().scnattn_text_max_len() == 128 == L.TEXT_MAX_LEN
    for macro, value in (("MAX_LEN", L.TEXT_MAX_LEN), ("MAX_REFS", L.TEXT_MAX_REFS), ("CIDER_MAX_TOKEN", L.TEXT_CIDER_MAX_TOKEN)):
        assert int(re.search(r"#define SCNATTN_TEXT_%s (\d+)" % macro, header).group(1)) == value
    assert L.lib().scnattn_version() == 109


def test_argument_validation_returns_error_codes_without_a_gpu():
    """nothing below reaches a launch: every call is refused on its arguments, the buffers are host dummies"""
    from scnattn import _lib as L
    h = L.lib()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    off = (C.c_long * 5)(0, 0, 0, 0, 0)
    bad_off = (C.c_long * 5)(0, 3, 2, 2, 2)

    def stats(N=1, R=1, hyp=p, Lh=4, ref=p, Lr=4, nsh=0, nsr=0, sh=p, out=p):
        return h.scnattn_text_ngram_stats(None, N, R, hyp, Lh, p, ref, Lr, p, sh, nsh, p, nsr, out)

    def lcs(N=1, R=1, Lh=4, Lr=4, nsh=0, nsr=0, out=p, score=p):
        return h.scnattn_text_lcs(None, N, R, p, Lh, p, p, Lr, p, p, nsh, p, nsr, out, score, None)

    def keys(n=1, N=1, R=1, Lr=4, nsr=0, out=p, flag=p):
        return h.scnattn_text_ref_keys(None, n, N, R, p, Lr, p, p, nsr, out, flag)

    def cider(N=1, R=1, Lh=4, Lr=4, nsh=0, nsr=0, table=off, n_images=1, score=p, flag=p, tk=p):
        return h.scnattn_text_cider(None, N, R, p, Lh, p, p, Lr, p, p, nsh, p, nsr, tk, p, table, n_images, score, None, flag)

    refused = [
        (stats(hyp=None), "null pointer"), (stats(ref=None), "null pointer"), (stats(out=None), "null pointer"),
        (stats(N=-1), "N < 0"), (stats(Lh=129), "padded width"), (stats(Lr=129), "padded width"), (stats(Lh=0), "padded width"),
        (stats(nsh=5), "skip list"), (stats(nsr=5), "skip list"), (stats(nsr=-1), "skip list"), (stats(nsh=1, sh=None), "skip list"),
        (stats(R=0), "R outside"), (stats(R=33), "R outside"),
        (lcs(out=None), "null pointer"), (lcs(score=None), "null pointer"), (lcs(N=-1), "N < 0"), (lcs(Lh=129), "padded width"),
        (lcs(Lr=129), "padded width"), (lcs(nsh=5), "skip list"), (lcs(R=33), "R outside"),
        (keys(out=None), "null pointer"), (keys(flag=None), "null pointer"), (keys(n=0), "n outside 1..4"),
        (keys(n=5), "n outside 1..4"), (keys(N=-1), "N < 0"), (keys(Lr=129), "padded width"), (keys(nsr=5), "skip list"),
        (keys(R=0), "R outside"),
        (cider(score=None), "null pointer"), (cider(flag=None), "null pointer"), (cider(table=None), "null pointer"),
        (cider(N=-1), "N < 0"), (cider(Lh=129), "padded width"), (cider(Lr=129), "padded width"), (cider(nsh=5), "skip list"),
        (cider(nsr=5), "skip list"), (cider(n_images=0), "n_images"), (cider(table=bad_off), "not ascending"),
        (cider(table=(C.c_long * 5)(0, 1, 2, 3, 4), tk=None), "null table"), (cider(R=33), "R outside"),
    ]
    # each call above overwrote the message of the one before it: repeat one by one for the texts
    assert all(rc == -1 for rc, _ in refused)
    for call, text in ((lambda: stats(Lh=129), "padded width"), (lambda: keys(n=5), "n outside 1..4"),
                       (lambda: cider(nsh=5), "skip list"), (lambda: lcs(N=-1), "N < 0"), (lambda: stats(hyp=None), "null pointer"),
                       (lambda: cider(table=bad_off), "not ascending"), (lambda: stats(R=33), "R outside")):
        assert call() == -1
        msg = h.scnattn_last_error().decode()
        assert text in msg and "invalid argument" in msg, msg


def test_pack_rejects_long_sequences_before_any_upload():
    from scnattn import textmetrics as TM
    with pytest.raises(ValueError):
        TM.pack_captions([[1] * 129], device="cpu")
    with pytest.raises(ValueError):
        TM.pack_references([[[1] * 129]], device="cpu")
    tok, n = TM.pack_captions([[1, 2, 3], [], [4]], device="cpu")
    assert tok.tolist() == [[1, 2, 3], [0, 0, 0], [4, 0, 0]] and n.tolist() == [3, 0, 1]
    ref, n = TM.pack_references([[[1, 2], [3]], [[4]]], device="cpu")
    assert ref.tolist() == [[[1, 2], [3, 0]], [[4, 0], [0, 0]]] and n.tolist() == [[2, 1], [1, -1]]


def test_generators_cover_the_listed_cases():
    hyps, refs = T.length_corpus()
    lens = {0, 1, 3, 4, 63, 64, 65, 127, 128}
    assert {len(h) for h in hyps} == lens and {len(r[0]) for r in refs} == lens and len(hyps) == 81
    hyps, refs = T.corner_corpus()
    assert T.ngram_stats(hyps[0], refs[0])[0:4] == [3, 2, 1, 0]              # 2 2 2 2 2 against 1 2 2 2 3: clipped
    assert T.ngram_stats(hyps[1], refs[1])[9] == 4                           # tie between 4 and 6
    assert all(len(hyps[2]) > len(r) for r in refs[2]) and all(len(hyps[3]) < len(r) for r in refs[3])
    assert refs[4][1] is None and refs[4][2] is not None and not T.present(refs[5])
    assert T.ngram_stats(hyps[5], refs[5]) == [0, 0, 0, 0, 4, 3, 2, 1, 4, 0]
    h, r, sh, sr = T.skip_corpus()
    sh_, sr_ = T.stripped(h, r, sh, sr)
    assert sh_[0] == [1, 2, 3] and sh_[1] == [] and sh_[2] == [1, 2, 3, 4] and sr_[0][1] == [1, 2, 3, 91] and sr_[2][1] == []
    hy, rf = T.random_corpus(1, 6, 12)
    assert len(hy) == 6 and all(len(p) == 5 for p in rf) and random.Random(1).random() == random.Random(1).random()
