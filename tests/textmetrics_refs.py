"""Pure-Python restatements of the caption text metrics (include/scnattn.h), written from the definitions -- dicts
of tuples, the textbook LCS table, math.fsum in fp64 -- and the case generators of the text-metric tests.  Nothing here is a
port of a package and nothing here touches the GPU.

Conventions: a hypothesis is a list of token ids; the references of an image are a list whose entries are lists of token ids
or None (an absent slot).  Special tokens are stripped by `strip` before a sequence gets here."""
import math
import random
from fractions import Fraction

SIGMA = 6.0
BETA = 1.2
SENTINEL = -1
CIDER_MAX_TOKEN = 65534


def strip(seq, skip):
    return [w for w in seq if w not in skip]


def ngram_counts(seq, n):
    out = {}
    for i in range(len(seq) - n + 1):
        g = tuple(seq[i:i + n])
        out[g] = out.get(g, 0) + 1
    return out


def present(refs):
    return [r for r in refs if r is not None]


# ---- integer statistics ----------------------------------------------------------------------------------------------------
def closest_ref_length(hyp, refs):
    lens = [len(r) for r in present(refs)]
    if not lens:
        return 0
    return min(lens, key=lambda l: (abs(l - len(hyp)), l))


def ngram_stats(hyp, refs):
    """[clipped matches n = 1..4, guesses n = 1..4, len(hyp), closest reference length]"""
    clipped, guess = [], []
    for n in range(1, 5):
        h = ngram_counts(hyp, n)
        rc = [ngram_counts(r, n) for r in present(refs)]
        clipped.append(sum(min(c, max([d.get(g, 0) for d in rc], default=0)) for g, c in h.items()))
        guess.append(max(0, len(hyp) - n + 1))
    return clipped + guess + [len(hyp), closest_ref_length(hyp, refs)]


def corpus_totals(hyps, all_refs):
    """(ten COCO totals, four NLTK denominators): column sums of ngram_stats; NLTK's modified_precision counts max(1, guesses)
    per hypothesis."""
    rows = [ngram_stats(h, r) for h, r in zip(hyps, all_refs)]
    tot = [sum(r[k] for r in rows) for k in range(10)]
    den = [sum(max(1, r[4 + k]) for r in rows) for k in range(4)]
    return tot, den


# ---- the two BLEU tails ------------------------------------------------------------------------------------------------------
def bleu_nltk_tail(num, den, hyp_len, ref_len, weights=(0.25, 0.25, 0.25, 0.25)):
    """Papineni et al. as NLTK's corpus_bleu computes it without smoothing: 0 without a unigram match or when an order has
    no match, brevity penalty exp(1 - r/c) for c <= r, geometric mean of the corpus precisions."""
    if num[0] == 0 or hyp_len == 0:
        return 0.0
    bp = 1.0 if hyp_len > ref_len else math.exp(1 - Fraction(ref_len, hyp_len))
    logs = []
    for n, w in enumerate(weights):
        if num[n] == 0:
            return 0.0
        logs.append(w * math.log(Fraction(num[n], den[n])))
    return bp * math.exp(math.fsum(logs))


def bleu_coco_tail(correct, guess, hyp_len, ref_len):
    """[Bleu_1..Bleu_4], COCO form: running product of (correct_k + 1e-15) / (guess_k + 1e-9), n-th root, times
    exp(1 - 1/ratio) when ratio = (hyp_len + 1e-15) / (ref_len + 1e-9) < 1."""
    ratio = (hyp_len + 1e-15) / (ref_len + 1e-9)
    out, prod = [], 1.0
    for n in range(1, 5):
        prod = prod * ((correct[n - 1] + 1e-15) / (guess[n - 1] + 1e-9))
        b = prod ** (1.0 / n)
        if ratio < 1:
            b = b * math.exp(1 - 1 / ratio)
        out.append(b)
    return out


# ---- LCS / ROUGE-L -----------------------------------------------------------------------------------------------------------
def lcs(a, b):
    """textbook dynamic programme: T[i][j] = LCS of a[:i], b[:j]"""
    T = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            T[i][j] = T[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(T[i - 1][j], T[i][j - 1])
    return T[len(a)][len(b)]


def rouge_l(hyp, refs):
    """(lcs per slot, 0 for an absent one; score): P = max lcs/len(hyp), Rc = max lcs/len(ref), zero lengths left out,
    (1 + b^2) P Rc / (Rc + b^2 P), 0 when P or Rc is 0"""
    ls = [0 if r is None else lcs(hyp, r) for r in refs]
    P = max([l / len(hyp) for l, r in zip(ls, refs) if r is not None and len(hyp) > 0], default=0.0)
    Rc = max([l / len(r) for l, r in zip(ls, refs) if r is not None and len(r) > 0], default=0.0)
    b2 = BETA * BETA
    return ls, (((1 + b2) * P * Rc) / (Rc + b2 * P) if P > 0 and Rc > 0 else 0.0)


# ---- CIDEr-D -----------------------------------------------------------------------------------------------------------------
def cider_df(all_refs):
    """df[n-1][g]: the number of IMAGES with the n-gram g in at least one of their references"""
    df = [{} for _ in range(4)]
    for refs in all_refs:
        for n in range(1, 5):
            seen = set()
            for r in present(refs):
                seen.update(ngram_counts(r, n))
            for g in seen:
                df[n - 1][g] = df[n - 1].get(g, 0) + 1
    return df


def key_of(g):
    """the n-gram as a signed 64-bit key: token k in bits 16k..16k+15"""
    k = 0
    for i, t in enumerate(g):
        assert 0 <= t <= CIDER_MAX_TOKEN
        k |= t << (16 * i)
    return k - (1 << 64) if k >= (1 << 63) else k


def df_tables(all_refs):
    """per order: (keys ascending as signed int64, df of each)"""
    out = []
    for d in cider_df(all_refs):
        items = sorted((key_of(g), c) for g, c in d.items())
        out.append(([k for k, _ in items], [c for _, c in items]))
    return out


def ref_keys(refs, n, width):
    """keys[r][j] of scnattn_text_ref_keys for one image: the key at the first occurrence of an n-gram within the image's
    references (slot order, then position), the sentinel everywhere else"""
    seen, out = set(), []
    for r in refs:
        row = [SENTINEL] * width
        if r is not None:
            for j in range(len(r) - n + 1):
                g = tuple(r[j:j + n])
                if g not in seen:
                    seen.add(g)
                    row[j] = key_of(g)
        out.append(row)
    return out


def _weights(seq, n, df, log_n):
    return {g: c * (log_n - math.log(max(1, df[n - 1].get(g, 0)))) for g, c in ngram_counts(seq, n).items()}


def cider_d(hyp, refs, df, n_images):
    """CIDEr-D of one image, n = 1..4, sigma = 6, x10: per order the clipped cosine of the tf-idf vectors times the Gaussian
    length penalty on the token-length difference, summed over the present references; then the mean over the orders, over
    the references, times 10.  0 without a present reference."""
    log_n = math.log(n_images)
    refs = present(refs)
    if not refs:
        return 0.0
    acc = [0.0] * 4
    for r in refs:
        pen = math.exp(-((len(hyp) - len(r)) ** 2) / (2 * SIGMA * SIGMA))
        for n in range(1, 5):
            wh, wr = _weights(hyp, n, df, log_n), _weights(r, n, df, log_n)
            val = math.fsum(min(w, wr.get(g, 0.0)) * wr.get(g, 0.0) for g, w in wh.items())
            den = math.sqrt(math.fsum(w * w for w in wh.values())) * math.sqrt(math.fsum(w * w for w in wr.values()))
            if den != 0:
                val /= den
            acc[n - 1] += val * pen
    return math.fsum(acc) / 4 / len(refs) * 10.0


def cider_scores(hyps, all_refs):
    df = cider_df(all_refs)
    return [cider_d(h, r, df, len(all_refs)) for h, r in zip(hyps, all_refs)]


def mean(xs):
    return math.fsum(xs) / len(xs) if xs else 0.0


def score_all(hyps, all_refs):
    """the seven values of CaptionScorer.score"""
    tot, den = corpus_totals(hyps, all_refs)
    out = {"Bleu_%d" % (n + 1): b for n, b in enumerate(bleu_coco_tail(tot[0:4], tot[4:8], tot[8], tot[9]))}
    out["bleu4_nltk"] = bleu_nltk_tail(tot[0:4], den, tot[8], tot[9])
    out["ROUGE_L"] = mean([rouge_l(h, r)[1] for h, r in zip(hyps, all_refs)])
    out["CIDEr"] = mean(cider_scores(hyps, all_refs))
    return out


# ---- case generators -----------------------------------------------------------------------------------------------------------
def make_case(rng, n_hyp, vocab, cpi, lo, hi, noise):
    """a corpus of noisy copies of random base sentences: cpi references per image, each a copy with 30 % of its words
    replaced and sometimes one word dropped; the hypothesis a copy with `noise` replaced, sometimes truncated"""
    refs_all, hyps = [], []
    for _ in range(n_hyp):
        base = [rng.randrange(1, vocab) for _ in range(rng.randint(lo, hi))]
        refs = []
        for _ in range(cpi):
            r = [w if rng.random() > 0.3 else rng.randrange(1, vocab) for w in base]
            if rng.random() < 0.5 and len(r) > 2:
                del r[rng.randrange(len(r))]
            refs.append(r)
        hyp = [w if rng.random() > noise else rng.randrange(1, vocab) for w in base]
        if rng.random() < 0.4 and len(hyp) > 1:
            hyp = hyp[:rng.randint(1, len(hyp))]
        refs_all.append(refs)
        hyps.append(hyp)
    return refs_all, hyps


def random_corpus(seed, n_img, vocab, cpi=5, lo=8, hi=22, noise=0.25):
    refs, hyps = make_case(random.Random(seed), n_img, vocab, cpi, lo, hi, noise)
    return hyps, refs


def length_corpus(seed=3, vocab=9):
    """every pair of the lengths at which the kernels change path: 0, 1, 3 (no 4-gram), 4, 63, 64, 65, 127, 128; a small
    vocabulary so that long sequences share n-grams and subsequences.  R = 2."""
    rng = random.Random(seed)
    lens = [0, 1, 3, 4, 63, 64, 65, 127, 128]
    hyps, refs = [], []
    for lh in lens:
        for lr in lens:
            hyps.append([rng.randrange(1, vocab) for _ in range(lh)])
            refs.append([[rng.randrange(1, vocab) for _ in range(lr)], [rng.randrange(1, vocab) for _ in range(lens[(lens.index(lr) + 3) % len(lens)])]])
    return hyps, refs


def corner_corpus():
    """hand-made images, R = 5 slots: clipping, a closest-length tie, hypotheses longer / shorter than every reference, an
    absent slot in the middle, all slots absent, one n-gram in several references of an image, one n-gram in every image with
    a reference, a hypothesis n-gram found nowhere, the 4-gram of the largest admitted id next to the sentinel."""
    T = CIDER_MAX_TOKEN
    hyps = [[2, 2, 2, 2, 2],                       # clipping against 1 2 2 2 3
            [1, 2, 3, 4, 5],                       # tie: references of 4 and 6 tokens -> 4
            [7, 1, 2, 3, 4, 5, 6, 7, 8, 9, 7],     # longer than every reference
            [7, 5],                                # shorter than every reference
            [7, 1, 2, 3],                          # absent slot in the middle
            [7, 4, 4, 4],                          # all slots absent
            [7, 40, 41, 42, 43, 40, 41],           # n-grams found in no reference
            [T, T, T, T, 7],                       # largest key
            [7]]
    refs = [[[1, 2, 2, 2, 3, 7], None, None, None, None],
            [[1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [7, 7, 7, 7, 7, 7, 7, 7, 7], None, None],
            [[7, 1, 2, 3], [1, 2, 3, 4, 5], [7, 8, 9], [5, 6, 7, 8], [1, 2]],
            [[7, 5, 6], [7, 5, 6, 1], [5, 7, 5, 6, 2], [7, 1, 1, 5, 1], [1, 2, 3, 7, 5, 3]],
            [[7, 1, 2, 3], None, [1, 2, 3, 7], None, [7, 1, 2]],
            [None, None, None, None, None],
            [[7, 1, 2], [7, 1, 2], [1, 2, 7, 1, 2], None, None],      # 7 1 2 in three references: df counts the image once
            [[T, T, T, T], [T, T, T, T, T, 7], None, None, None],
            [[7], [7, 7], [], None, None]]
    return hyps, refs


def skip_corpus():
    """sequences with the skipped ids 90 / 91 / 0 at the start, in the middle and at the end, and sequences made of them only;
    returns (hyps, refs, skip_hyp, skip_ref)"""
    hyps = [[90, 1, 2, 3, 91, 0, 0], [90, 91, 0], [1, 90, 90, 2, 3, 4, 91], [90, 5, 6, 91]]
    refs = [[[90, 1, 2, 3, 4, 91, 0], [90, 1, 0, 2, 3, 91, 0]],
            [[90, 1, 2, 91, 0, 0, 0], [90, 91, 0, 0, 0, 0, 0]],
            [[90, 91, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]],
            [[90, 5, 91, 6, 0, 0, 0], None]]
    return hyps, refs, (90, 91, 0), (90, 0)


def stripped(hyps, refs, skip_hyp, skip_ref):
    return ([strip(h, set(skip_hyp)) for h in hyps],
            [[None if r is None else strip(r, set(skip_ref)) for r in per] for per in refs])
