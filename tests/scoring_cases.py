"""The cases of the scoring kernel (scnattn_rollout_score), shared by the CPU restatement in tests/test_scoring_refs.py and the
GPU module tests/test_gpu_scoring_kernels.py.  A case walks STEPS steps on one state; its rows take a FLAVOUR per (row, step,
run), so every flavour meets every V, every load path and both temperatures somewhere in the table:
    plain   uniform in +-3; the target at index 0, at V - 1, at the maximum, at the minimum in turn
    ties    integers in -2 .. 2, so the target sits among equals (words equal to it with a lower index count); every third such
            row is ALL-EQUAL, where rank must be the target's index
    zeros   -0.0, +0.0 and -1.0 mixed; the target on a zero: -0 == +0 in the ORDER
    inf     most logits -inf; the target finite, or -inf (logp = -inf), or the row's ONE finite logit (logp = +0.0)
    wide    uniform in +-80
ntok per row cycles through 0 .. 4: a row that is closed from the start (zero records), rows that close at steps 0, 1 and 2
(the counters go down once each), and a row still open after the last step.  The configuration with three images closes
image 1 (nsrc = 0: nothing of it is read or written, whatever its ntok says)."""
import torch

import scoring_refs as SR
from kernel_harness import SENT, SENTI, _bound_ok

STEPS = 3
RECORDS = ("token", "logp", "rank", "best")
VS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 10000)
# (N, K, closed image or None)
CONFIGS = {"N1K1": (1, 1, None), "N1K3": (1, 3, None), "N3K8": (3, 8, 1)}
INV_TEMPS = (1.0, float(torch.tensor(1.0 / 0.7, dtype=torch.float32)))
# the load paths: (name, ld as a function of V, base misaligned by one float)
FORMS = (("ld=V", lambda V: V, 0), ("ld>V vector", lambda V: (V + 3) // 4 * 4 + 4, 0), ("ld>V scalar", lambda V: (V + 3) // 4 * 4 + 5, 0),
         ("base+4B scalar", lambda V: (V + 3) // 4 * 4 + 4, 1))
RUNS = tuple((f, it) for f in range(len(FORMS)) for it in range(len(INV_TEMPS)))
FLAVOURS = ("plain", "ties", "zeros", "inf", "wide")
NINF = float("-inf")


def row_of(g, V, flavour, turn):
    """-> (logits fp32 [V], target)"""
    def rnd(n=V):
        return torch.rand(n, generator=g)

    def pick(n):
        return int(torch.randint(0, n, (1,), generator=g))

    if flavour == "plain":
        x = (rnd() * 6 - 3).float()
        tgt = (0, V - 1, int(x.argmax()), int(x.argmin()))[turn % 4]
    elif flavour == "ties":
        x = torch.full((V,), 1.25) if turn % 3 == 2 else torch.floor(rnd() * 5 - 2).float()
        tgt = pick(V)
    elif flavour == "zeros":
        x = torch.tensor([-0.0, 0.0, -1.0])[torch.randint(0, 3, (V,), generator=g)].clone()
        zeros = (x == 0).nonzero().reshape(-1)
        tgt = int(zeros[pick(zeros.numel())]) if zeros.numel() else 0
    elif flavour == "inf":
        x = (rnd() * 6 - 3).float()
        keep = pick(V)
        if turn % 3 == 2 or V == 1:         # one finite logit, and it is the target
            x[:] = NINF
            x[keep] = 0.75
            tgt = keep
        else:
            x[rnd() < 0.7] = NINF
            x[keep] = 1.5                   # at least one finite logit
            gone = (x == NINF).nonzero().reshape(-1)
            tgt = int(gone[pick(gone.numel())]) if turn % 3 == 1 and gone.numel() else keep
    else:
        x = (rnd() * 160 - 80).float()
        tgt = pick(V)
    return x, tgt


def gen_case(V, cfg, run):
    """-> dict: N, K, closed, form, inv_temp, ld, mis, logits [STEPS] of fp32 [R, V], target int32 [STEPS, R], ntok int32 [R],
    nsrc int32 [N], flavour [STEPS][R]"""
    N, K, closed = CONFIGS[cfg]
    f, it = RUNS[run]
    R = N * K
    g = torch.Generator().manual_seed(424200 + 97 * V + 1009 * N + 31 * K + run)
    logits, target, flav = [], torch.zeros(STEPS, R, dtype=torch.int32), []
    for t in range(STEPS):
        x = torch.zeros(R, V)
        names = []
        for r in range(R):
            names.append(FLAVOURS[(r + t + run) % len(FLAVOURS)])
            x[r], tgt = row_of(g, V, names[-1], r + 2 * t + run)
            target[t, r] = tgt
        logits.append(x)
        flav.append(names)
    ntok = torch.tensor([(r + run) % 5 for r in range(R)], dtype=torch.int32)
    nsrc = torch.full((N,), K, dtype=torch.int32)
    if closed is not None:
        nsrc[closed] = 0
    name, ld_of, mis = FORMS[f]
    return dict(N=N, K=K, closed=closed, form=name, inv_temp=INV_TEMPS[it], ld=ld_of(V), mis=mis, logits=logits, target=target,
                ntok=ntok, nsrc=nsrc, flavour=flav)


def y32(x, inv_temp):
    """fl(logits * inv_temp): the fp32 number the kernel forms"""
    return x.float() * torch.tensor(inv_temp, dtype=torch.float32)


def bits(x):
    return x.view(torch.int32)


def judge(V, case, got, form):
    """every record of every row; -> counts for the case's own coverage assertions"""
    N, K = case["N"], case["K"]
    R = N * K
    ntok, nsrc = case["ntok"], case["nsrc"]
    nopen, open_rows = got["nopen0"].clone(), int(got["nopen0"].sum())
    sum_logp = torch.zeros(R)
    seen = dict(open=0, zero=0, closed_image=0, closing=0, inf=0, pzero=0, ties=0, allequal=0)
    want_lp, bound_lp, got_lp = [], [], []
    for t in range(STEPS):
        y = y32(case["logits"][t], case["inv_temp"])
        tgt = case["target"][t].long()
        ref = SR.of_y(y.double(), tgt)
        bound = SR.logp_bound(ref)
        lo, hi = SR.rank_interval(y, tgt)
        for r in range(R):
            n = r // K
            rec = {k: got[k][t, r] for k in RECORDS}
            if nsrc[n] == 0:                    # a closed image: neither read nor written
                assert all(int(rec[k]) == SENTI for k in ("token", "rank", "best")) and int(bits(rec["logp"])) == SENT, (t, r)
                seen["closed_image"] += 1
                continue
            if t >= ntok[r]:                    # a closed row of an open image: zero records
                assert all(int(bits(rec[k])) == 0 for k in RECORDS), (t, r, rec)
                seen["zero"] += 1
                continue
            seen["open"] += 1
            where = "%s V=%d t=%d row %d (%s)" % (form, V, t, r, case["flavour"][t][r])
            assert int(rec["token"]) == int(tgt[r]), where
            assert int(rec["best"]) == int(ref["best"][r]), "%s: best %d, reference %d" % (where, rec["best"], ref["best"][r])
            assert int(lo[r]) <= int(rec["rank"]) <= int(hi[r]), where
            assert int(rec["rank"]) == int(ref["rank"][r]), "%s: rank %d, reference %d" % (where, rec["rank"], ref["rank"][r])
            assert (int(rec["rank"]) == 0) == (int(rec["best"]) == int(tgt[r])), where
            w = float(ref["logp"][r])
            if w == float("-inf"):
                assert float(rec["logp"]) == w, "%s: logp %r for a -inf target" % (where, float(rec["logp"]))
                seen["inf"] += 1
            else:
                want_lp.append(w), bound_lp.append(float(bound[r])), got_lp.append(float(rec["logp"]))
            if int(torch.isfinite(y[r]).sum()) == 1 and int(rec["rank"]) == 0:
                assert int(bits(rec["logp"])) == 0, "%s: one finite logit must give +0.0, got %r" % (where, float(rec["logp"]))
                seen["pzero"] += 1
            same = int((y[r] == y[r, tgt[r]]).sum())
            seen["ties"] += int(same > 1)
            if same == V and V > 1:
                assert int(rec["rank"]) == int(tgt[r]), where
                seen["allequal"] += 1
            sum_logp[r] = sum_logp[r] + rec["logp"]                 # fp32, as the kernel adds
            if t + 1 == ntok[r]:                # the closing step: the counters go down by one, once
                nopen[n] -= 1
                open_rows -= 1
                seen["closing"] += 1
    if got_lp:
        _bound_ok("rollout_score " + form, "logp", torch.tensor(got_lp), torch.tensor(want_lp, dtype=torch.float64),
                  torch.tensor(bound_lp, dtype=torch.float64), "=2 u (dmax + 3 + |logp|)")
    open_img = (nsrc > 0).repeat_interleave(K)
    assert torch.equal(bits(got["sum_logp"])[open_img], bits(sum_logp)[open_img]), (got["sum_logp"], sum_logp)
    assert bool((bits(got["sum_logp"])[~open_img] == 0).all())      # the closed image's accumulators keep what they held
    assert torch.equal(got["nopen"], nopen) and int(got["open_rows"]) == open_rows, (got["nopen"], nopen, got["open_rows"])
    assert torch.equal(got["nsrc"], nsrc) and torch.equal(got["ntok"], ntok) and torch.equal(got["target"], case["target"])
    return seen


# ---- the captions of the driver tests (tests/test_gpu_scoring.py), chosen on the CPU reference alone ------------------------
# Three captions per image: slot 0 random words (rank far from 0: what a foreign caption looks like), slot 1 the caption the
# fp64 rollout reference SAMPLES for that image at temperature 0.7 with (ROLL_SEED, draw 0) (the model's own kind of
# caption: low ranks), slot 2 by image: ONE token; 51 tokens and no <end>; <end> in the middle with words behind it; a short
# caption without <end>.  CAPTION_SEED was not searched: with continuous logits over 23 .. 1003 words a near-tie between the
# target and a neighbour is rare, and tests/test_scoring_refs.py asserts the share of judged positions on the CPU (at least
# 3/4; it is above 0.99 for every case).
CAPTION_SEED, ROLL_SEED = 20, 5
DRIVER_K = 3
DRIVER_INV_TEMP = INV_TEMPS[1]
_DRIVER = {}


def captions_for(kind, P64, wm, enc, tags, salt):
    """-> (targets [R][...], ntok [R]) for R = N * DRIVER_K rows: the tokens that follow <start>"""
    import rollout_refs as RR
    V, N = len(wm), enc.shape[0]
    start, end = wm["<start>"], wm["<end>"]
    g = torch.Generator().manual_seed(CAPTION_SEED + salt)
    roll = RR.rollout(kind, P64, 1, wm, enc.double(), None if tags is None else tags.double(), ROLL_SEED, 0, DRIVER_INV_TEMP)

    def words(n):
        return torch.randint(1, V - 3, (n,), generator=g).tolist()

    targets = []
    for n in range(N):
        targets.append(words(int(torch.randint(1, 12, (1,), generator=g))) + [end])
        targets.append(RR.caption_of(roll, n, start)[1:])
        targets.append(([end], words(51), words(4) + [end] + words(4), words(5))[n % 4])
    return targets, [len(x) for x in targets]


def driver_case(name, kind):
    """One of beam_refs.FIXTURES -> dict(d, wm, enc, tags, targets, ntok, ref (scoring_refs.score in fp64)); once per process"""
    import beam_refs as BR
    from helpers import params_from, t
    if name not in _DRIVER:
        d, V = BR.sharpened(name)
        wm = BR.word_map(V)
        enc = t(d["enc"])
        tags = t(d["tags"]) if kind != "pure_attention" else None
        P64 = params_from(d, dtype=torch.float64)
        targets, ntok = captions_for(kind, P64, wm, enc, tags, [n for n, _ in BR.FIXTURES].index(name))
        ref = SR.score(kind, P64, DRIVER_K, wm, enc.double(), None if tags is None else tags.double(), targets, ntok,
                       DRIVER_INV_TEMP)
        _DRIVER[name] = dict(d=d, wm=wm, enc=enc, tags=tags, targets=targets, ntok=ntok, ref=ref)
    return _DRIVER[name]


# the vector-width shapes of tests/test_gpu_rollout.py: (parameter seed) per kind
VECTOR_SEEDS = {"attention_scn": 6, "pure_scn": 78}


def vector_case(kind):
    """E=256, A=128, D=F=128, M=64, S=40, 7x7, V=1003, N=3 (test_gpu_beam_search._uniform_params)"""
    import beam_refs as BR
    from helpers import params_from
    from test_gpu_beam_search import _uniform_params
    key = "vector_" + kind
    if key not in _DRIVER:
        g = torch.Generator().manual_seed(VECTOR_SEEDS[kind])
        d, V, E, S = _uniform_params(kind, g)
        enc, tags = torch.rand(3, 7, 7, E, generator=g), torch.rand(3, S, generator=g)
        wm = BR.word_map(V)
        P64 = params_from(d, dtype=torch.float64)
        targets, ntok = captions_for(kind, P64, wm, enc, tags, 10 + len(kind))
        ref = SR.score(kind, P64, DRIVER_K, wm, enc.double(), tags.double(), targets, ntok, 1.0)
        _DRIVER[key] = dict(d=d, wm=wm, enc=enc, tags=tags, targets=targets, ntok=ntok, ref=ref)
    return _DRIVER[key]


def rank_checked(ref):
    """[R][ntok] bool: the reference's gap between the target and its nearest neighbour exceeds the band"""
    return [[g > b for g, b in zip(gs, bs)] for gs, bs in zip(ref["tgap"], ref["band"])]
