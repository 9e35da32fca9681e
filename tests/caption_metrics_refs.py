"""fp64 restatement, cases and judges of the caption loss with metrics (csrc/loss.hip: scnattn_caption_loss_metrics_fwd;
scnattn.functional.caption_loss_metrics), shared by tests/test_caption_metrics_refs.py (CPU: the restatement against the
oracle, utils.metric.accuracy and torch.max on tie-free rows) and tests/test_gpu_caption_metrics_kernels.py /
tests/test_gpu_caption_metrics_step.py (the kernels).  Index arithmetic per row, not the torch ops it is held to.

For a decoded row (b, t < min(dl[b], T)) with logits x[0..V) and target tg, elements ordered by (value descending, index
ascending):
    lse   = m + log(sum_v exp(x[v] - m)), m = max x;   loss = lse - x[tg]
    rank  = #{v : x[v] > x[tg]} + #{v < tg : x[v] == x[tg]}          the target's position in that order; top k <=> rank < k
    pred  = the first index in that order                             the arg-max, the lowest index among equal maxima
A target outside [0, V): loss NaN, rank INT32_MAX (never a hit), pred unchanged.  A row that was not decoded: lse = loss = 0,
rank = -1, pred = 0.  hits = [#{0 <= rank < k}, #{rank == 0}];  total = sum(loss) / n_tokens, n_tokens = sum_b min(dl[b], T).

Bounds: rank, pred and hits are comparisons of the given fp32 numbers: exactly equal, no case excepted.  lse, loss and the
total are held to the 1e-5 relative of tests/test_gpu_parity.py::test_fused_caption_loss_matches_oracle (rows: of the largest
|ref| of the case, the suite's tensor-level rel_err; the total: of |ref|), and to bit equality with scnattn_caption_loss_fwd."""
import torch

F64 = torch.float64
INT_MAX = 2 ** 31 - 1
NINF = float("-inf")
TOL = 1e-5

VOCABS = (1, 3, 4, 255, 256, 257, 1023, 1024, 1028, 1030, 2052)
B, T = 3, 4
LENGTHS = (T, 1, 0)
LONG_LENGTHS = (T + 3, T, 2)          # once a length greater than T: it decodes T rows


# ---- the restatement ----------------------------------------------------------------------------------------------------
def row_ref(x, tg):
    """(lse, loss, rank, pred) of one row of fp32 logits; the arithmetic in fp64, the comparisons on the values as given"""
    V = x.numel()
    xd = x.to(F64)
    m = float(xd.max())
    lse = m + float(torch.log(torch.exp(xd - m).sum()))
    pred = int((xd == m).nonzero()[0])
    if tg < 0 or tg >= V:
        return lse, float("nan"), INT_MAX, pred
    xt = xd[tg]
    rank = int((xd > xt).sum()) + int((xd[:tg] == xt).sum())
    return lse, lse - float(xt), rank, pred


def metrics_ref(scores, targets, lengths, k):
    """scores (B, T, V) fp32, targets (B, T) int64, lengths: B decode lengths -> dict of lse / loss [B*T] (fp64), rank [B*T],
    preds [B, T], hits [2] (int32 values), total (fp64: the cross-entropy part of the loss), n_tokens"""
    Bn, Tn, _ = scores.shape
    lse, loss = torch.zeros(Bn * Tn, dtype=F64), torch.zeros(Bn * Tn, dtype=F64)
    rank = torch.full((Bn * Tn,), -1, dtype=torch.int64)
    preds = torch.zeros(Bn, Tn, dtype=torch.int64)
    n = 0
    for b in range(Bn):
        for t in range(min(int(lengths[b]), Tn)):
            r = b * Tn + t
            lse[r], loss[r], rank[r], preds[b, t] = row_ref(scores[b, t], int(targets[b, t]))
            n += 1
    hits = torch.tensor([int(((rank >= 0) & (rank < k)).sum()), int((rank == 0).sum())])
    return dict(lse=lse, loss=loss, rank=rank, preds=preds, hits=hits, total=loss.sum() / max(n, 1), n_tokens=n)


# ---- tie-free rows (the restatement and topk agree on every one) ----------------------------------------------------------
def gen_tie_free(Bn, Tn, V, seed):
    """every row a permutation of V distinct values; targets anywhere in [0, V)"""
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(-3.0, 3.0, V) if V > 1 else torch.zeros(1)
    assert base.unique().numel() == V
    scores = torch.stack([base[torch.randperm(V, generator=g)] for _ in range(Bn * Tn)]).view(Bn, Tn, V)
    targets = torch.randint(0, V, (Bn, Tn), generator=g)
    return scores, targets


# ---- adversarial rows -----------------------------------------------------------------------------------------------------
# Where the planted elements go.  The vector form gives thread i the elements 4i..4i+3 (+1024 per sweep), the scalar form
# gives it i (+256 per sweep); a wave is 64 threads.  The list walks through vector lanes (0..3, 6), the four waves of
# either form (65, 130, 195 scalar; 257, 515, 777 vector), the last elements of the first sweep and the first of the next
# (1022..1030), a second vector sweep (1500, 2049) and the ends of the row.  The first five already differ in lane, wave
# and sweep of both forms: k = 5 plants no more than that.
_SPOTS = (1, 322, 1027, 707, 2049, 0, 2, 3, 6, 65, 130, 195, 257, 300, 515, 777, 1022, 1023, 1024, 1025, 1029, 1500)


def _spots(V, avoid, n, g):
    """n distinct indices != avoid, the planted spots first (and V-1, V/2), then random ones; fewer when the row is short"""
    out = []
    for v in _SPOTS + (V - 1, V // 2):
        if 0 <= v < V and v != avoid and v not in out:
            out.append(v)
    rest = [v for v in torch.randperm(V, generator=g).tolist() if v != avoid and v not in out]
    return (out + rest)[:max(n, 0)]


def _plain(V, g):
    """distinct values in (-1, 1): a shuffled grid"""
    base = torch.linspace(-0.9, 0.9, V) if V > 1 else torch.zeros(1)
    return base[torch.randperm(V, generator=g)].clone()


def row_above(V, k, g, n):
    """exactly min(n, V-1) logits above the target, the rest below it"""
    x = _plain(V, g)
    tg = (V // 3) if V > 2 else V - 1
    x[tg] = 2.0
    for i, v in enumerate(_spots(V, tg, n, g)):
        x[v] = 3.0 + 0.01 * i
    return x, tg


def row_tied_target(V, k, g):
    """the target's value also at lower and at higher indices, in other lanes, waves and sweeps; two logits above it"""
    x = _plain(V, g)
    tg = V // 2
    x[tg] = 1.5
    sp = _spots(V, tg, V, g)
    ties = [v for v in sp if v < tg][:5] + [v for v in sp if v > tg][:5]
    for v in ties:
        x[v] = 1.5
    for v in [v for v in sp if v not in ties][:2]:
        x[v] = 2.5
    return x, tg


def row_tied_max(V, k, g):
    """the maximum at several indices across waves and sweeps; the lowest of them is the arg-max; the target is one of the
    others when there is one"""
    x = _plain(V, g)
    at = sorted({v for v in (1, 3, 130, 515, 777, 1025, 2049, V - 1) if 0 <= v < V})
    for v in at:
        x[v] = 4.0
    return x, max(at)


def row_all_equal(V, k, g):
    return torch.full((V,), 0.25), V // 2


def row_neg_inf(V, k, g):
    """-inf entries, a whole vector of them and the first element among them; the target is finite"""
    x = _plain(V, g)
    tg = V - 1
    for v in list(range(0, min(8, V - 1))) + _spots(V, tg, 15, g)[5:]:
        x[v] = NINF
    return x, tg


def row_target_first(V, k, g):
    return _plain(V, g), 0


def row_target_last(V, k, g):
    return _plain(V, g), V - 1


def row_target_argmax(V, k, g):
    x = _plain(V, g)
    return x, int(x.argmax())


def row_label_below(V, k, g):
    return _plain(V, g), -1


def row_label_above(V, k, g):
    return _plain(V, g), V


KINDS = dict(
    hit=lambda V, k, g: row_above(V, k, g, k - 1), miss=lambda V, k, g: row_above(V, k, g, k), tied_target=row_tied_target,
    tied_max=row_tied_max, all_equal=row_all_equal, neg_inf=row_neg_inf, first=row_target_first, last=row_target_last,
    argmax=row_target_argmax, below=row_label_below, above=row_label_above)

# what fills the decoded rows of a case, in the order (b, t) of the decoded rows; "labels" is the one with bad labels (its
# loss is NaN), "long" runs LONG_LENGTHS
VARIANTS = dict(
    ranks=(LENGTHS, ("hit", "miss", "tied_target", "tied_max", "all_equal")),
    ends=(LENGTHS, ("neg_inf", "first", "last", "argmax", "miss")),
    labels=(LENGTHS, ("below", "above", "hit", "tied_target", "neg_inf")),
    long=(LONG_LENGTHS, ("miss", "hit", "all_equal", "tied_max", "tied_target", "argmax", "last", "first", "neg_inf", "hit")))


def gen_case(V, k, variant, seed=0):
    """scores (B, T, V), targets (B, T) (bad labels included), lengths, the kind of every decoded row.  Rows that are not
    decoded hold plain values and a valid target."""
    lengths, kinds = VARIANTS[variant]
    g = torch.Generator().manual_seed(7919 * seed + 31 * V + k + 1000003 * sorted(VARIANTS).index(variant))
    scores = torch.stack([_plain(V, g) for _ in range(B * T)]).view(B, T, V)
    targets = torch.randint(0, V, (B, T), generator=g)
    names, i = [], 0
    for b in range(B):
        for t in range(min(lengths[b], T)):
            x, tg = KINDS[kinds[i]](V, k, g)
            scores[b, t], targets[b, t] = x, tg
            names.append(kinds[i])
            i += 1
    assert i == len(kinds)
    return scores, targets, list(lengths), names


def ks_of(V):
    return (1, 5, V + 1)
