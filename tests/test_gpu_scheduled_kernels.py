"""GPU tests (``-m gpu``) of the scheduled-sampling kernel of csrc/rollout.hip through the C ABI, alone:
scnattn_rollout_pick_mixed per row against the fp64 reference of tests/scheduled_refs.py and tests/rollout_refs.py.  The coin
(`replaced`) and every record of a row that keeps its gold word are EXACT; a replaced row's token passes rollout_refs.token_ok
(the band) and its logp lies within rollout_refs.logp_at's bound at the device's token; the book-keeping (sum_logp as the fp32
sum of the device's own records, nopen, open_rows) is derived from nmix and must be met exactly.

Buffers are guarded windows (tests/kernel_harness.py): NaN around the logits and in the gap ld - V of every row, the sentinel
around and inside every record.  A case walks three steps on one state with nmix in {0, 1, 2, 3, 7}, so rows are empty from
the start, close on the way or stay open; with more than one image, image 1 is closed (nsrc = 0: its rows and records keep the
sentinel).  Shapes: V = 1 (one word), 3, 4 (exactly one group of four), 5, 257, 1027 (more than one sweep of the workgroup's
256 x 4 words, odd), 10 000; R = 1 x 1, 3 x 2, 2 x 8; ld = V and ld = V + 1 (a multiple of 4 at V = 3, 4, 1027 and
10 000: the 16-byte loads, the bases being aligned; every other one is the scalar path); prob 0, 0.25, 1; greedy on and
off; inv_temp 1 and fl32(1/0.7).
The 1 % cap on ambiguous rows is judged by the reference alone (rollout_refs.ambiguous on the replaced rows); the seeds of
gen_case were fixed on the CPU, where no case has an ambiguous row."""
import ctypes as C

import pytest
import torch

import rollout_refs as RR
import scheduled_refs as SS
from kernel_harness import GBuf, GBufI, SENT, SENTI, _bound_ok, _call, _write_report      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "scheduled-sampling kernel vs fp64: worst |got - ref| / bound over all cases (tests/rollout_refs.py: the bound)"

SEED = 0x5eed0123456789ab
STEPS = 3
SEED_BASE = 4001     # of the generated logits; fixed on the CPU reference so that no case holds an ambiguous row
VS = (1, 3, 4, 5, 257, 1027, 10000)
CONFIGS = {"N1K1": (1, 1), "N3K2": (3, 2), "N2K8": (2, 8)}
PROBS = (0.0, 0.25, 1.0)
INV_TEMPS = (1.0, SS.INV_TEMP)
NMIX = (3, 0, 1, 7, 2, 3, 1, 7, 0, 2, 3, 3, 1, 7, 2, 0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def gen_case(V, cfg, ld_extra, prob_i, greedy, it_idx):
    """logits STEPS x [R, V] uniform in +-3, gold words in [0, V), nmix, nsrc; image 1 closed when there is one"""
    N, K = CONFIGS[cfg]
    R = N * K
    g = torch.Generator().manual_seed(SEED_BASE + 7 * V + 131 * N + 17 * K + 3 * ld_extra + 5 * prob_i + 11 * int(greedy) + it_idx)
    logits = [(torch.rand(R, V, generator=g) * 6 - 3).float() for _ in range(STEPS)]
    gold = torch.randint(0, V, (STEPS, R), generator=g).to(torch.int32)
    nmix = torch.tensor([NMIX[(r + V) % len(NMIX)] for r in range(R)], dtype=torch.int32)
    nmix[0] = 3 if R == 1 else nmix[0]
    nsrc = torch.full((N,), K, dtype=torch.int32)
    if N > 1:
        nsrc[1] = 0
    draw = 1 + 4 * prob_i + 2 * ld_extra + it_idx
    return dict(N=N, K=K, V=V, ld=V + ld_extra, logits=logits, gold=gold, nmix=nmix, nsrc=nsrc, prob=PROBS[prob_i],
                greedy=greedy, inv_temp=INV_TEMPS[it_idx], draw=draw)


def run_case(dev, case, entry="mixed"):
    """-> host copies of every buffer after STEPS steps (guards checked); the records as [STEPS, R]"""
    N, K, V, R = case["N"], case["K"], case["V"], case["N"] * case["K"]
    nmix, nsrc = case["nmix"], case["nsrc"]
    nopen = torch.where(nsrc > 0, (nmix.view(N, K) > 0).sum(dim=1).to(torch.int32), torch.zeros_like(nsrc))
    length = nmix if entry == "mixed" else torch.zeros_like(nmix)       # the plain pick: every row open, nothing closes
    bufs = dict(open_rows=GBufI(dev, 1, vals=nopen.sum()), nsrc=GBufI(dev, N, vals=nsrc), nopen=GBufI(dev, N, vals=nopen),
                nmix=GBufI(dev, R, vals=length), sum_logp=GBuf(dev, (R,), vals=torch.zeros(R), out=True),
                token=GBufI(dev, STEPS * R), logp=GBuf(dev, (STEPS, R), out=True), sample=GBufI(dev, STEPS * R),
                replaced=GBufI(dev, STEPS * R), gold=GBufI(dev, STEPS * R, vals=case["gold"]))
    arr = (C.c_void_p * 7)(*[bufs[k].ptr for k in ("open_rows", "nsrc", "nopen", "nmix", "sum_logp", "token", "logp")])
    at = lambda name, t: C.c_void_p(bufs[name].ptr.value + 4 * t * R)      # noqa: E731
    for t in range(STEPS):
        lb = GBuf(dev, (R, V), (case["ld"], 1), vals=case["logits"][t])
        if entry == "mixed":
            _call("scnattn_rollout_pick_mixed", dev, N, K, V, lb.ptr, case["ld"], case["inv_temp"], case["prob"], SEED,
                  case["draw"], t, int(case["greedy"]), STEPS, arr, at("gold", t), at("sample", t), at("replaced", t))
        else:           # an <end> no row can pick: V
            _call("scnattn_rollout_pick", dev, N, K, V, lb.ptr, case["ld"], case["inv_temp"], SEED, case["draw"], t, 0, V,
                  STEPS, arr)
    got = {k: b.read(k) for k, b in bufs.items()}
    for k in ("token", "logp", "sample", "replaced", "gold"):
        got[k] = got[k].view(STEPS, R)
    got["nopen0"] = nopen
    return got


def bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def judge(case, got, seen):
    N, K, V, R = case["N"], case["K"], case["V"], case["N"] * case["K"]
    nmix, nsrc = case["nmix"], case["nsrc"]
    sum_logp = torch.zeros(R)
    nopen, open_rows = got["nopen0"].clone(), int(got["nopen0"].sum())
    want_lp, bound_lp, got_lp = [], [], []
    for t in range(STEPS):
        ref = SS.mixed_step(case["logits"][t].double(), K, case["inv_temp"], case["prob"], SEED, case["draw"], t,
                            case["greedy"], case["gold"][t], nmix)
        p = ref["p"]
        amb = RR.ambiguous(p)
        for r in range(R):
            n = r // K
            rec = tuple(int(bits(got[k])[t, r]) for k in ("token", "sample", "logp", "replaced"))
            if nsrc[n] == 0:                    # a closed image: neither read nor written
                assert rec == (SENTI, SENTI, SENT, SENTI), (t, r, rec)
                seen["closed_image"] += 1
                continue
            if not ref["open"][r]:              # a closed row of an open image: 0 / -1 / +0.0 / 0
                assert rec == (0, -1, 0, 0), (t, r, rec)
                seen["closed"] += 1
                continue
            assert rec[3] == int(ref["replaced"][r]), "the coin of row %d step %d: %d" % (r, t, rec[3])
            if not ref["replaced"][r]:          # gold / -1 / +0.0 / 0, exactly
                assert rec == (int(case["gold"][t, r]), -1, 0, 0), (t, r, rec)
                seen["kept"] += 1
            else:
                tok = rec[0]
                assert rec[1] == tok and rec[3] == 1, (t, r, rec)
                seen["replaced"] += 1
                seen["ambiguous"] += int(amb[r])
                assert RR.token_ok(p, r, tok), "V=%d t=%d row %d: token %d (reference %d, fp64 gap %.3e, band %.3e)" % (
                    V, t, r, tok, int(p["token"][r]), float(p["key"][r].double().max() - p["key"][r, tok]),
                    float(RR.band(p)[r]))
                w, b = RR.logp_at(p, r, tok)
                want_lp.append(w), bound_lp.append(b), got_lp.append(float(got["logp"][t, r]))
                sum_logp[r] = sum_logp[r] + got["logp"][t, r]                  # fp32, as the kernel adds
            if ref["closing"][r]:
                nopen[n] -= 1
                open_rows -= 1
                seen["closing"] += 1
    if got_lp:
        _bound_ok("rollout_pick_mixed", "logp", torch.tensor(got_lp), torch.tensor(want_lp, dtype=torch.float64),
                  torch.tensor(bound_lp, dtype=torch.float64),
                  "=u (|y_tok| + |lse| + 2 |log s| + |logp| + 4 (V + 8) + 2 dmax + 2)")
    open_image = (nsrc > 0).repeat_interleave(K)
    assert torch.equal(bits(got["sum_logp"])[open_image], bits(sum_logp)[open_image]), (got["sum_logp"], sum_logp)
    assert bool((bits(got["sum_logp"])[~open_image] == 0).all())              # as the test initialised it: never touched
    assert torch.equal(got["nopen"], nopen) and torch.equal(got["nsrc"], nsrc) and int(got["open_rows"]) == open_rows
    assert torch.equal(got["nmix"], nmix) and torch.equal(got["gold"], case["gold"])       # read-only


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("V", VS)
def test_rollout_pick_mixed(dev, V, cfg):
    seen = dict(closed_image=0, closed=0, kept=0, replaced=0, ambiguous=0, closing=0)
    for ld_extra in (0, 1):
        for prob_i in range(len(PROBS)):
            for greedy in (False, True):
                it_idx = (ld_extra + prob_i + int(greedy)) % 2
                case = gen_case(V, cfg, ld_extra, prob_i, greedy, it_idx)
                got = run_case(dev, case)
                before = dict(seen)
                judge(case, got, seen)
                if PROBS[prob_i] == 0.0:
                    assert seen["replaced"] == before["replaced"]
                if PROBS[prob_i] == 1.0:
                    assert seen["kept"] == before["kept"]
    N, K = CONFIGS[cfg]
    print("%s V=%d: %s" % (cfg, V, seen))
    assert 100 * seen["ambiguous"] <= seen["replaced"]
    assert seen["kept"] > 0 and seen["replaced"] > 0 and seen["closing"] > 0
    assert (seen["closed_image"] > 0) == (N > 1) and (seen["closed"] > 0 or N * K == 1)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("V", VS)
def test_prob_one_is_the_plain_pick_bit_for_bit(dev, V, cfg):
    """non-greedy, every row open for all three steps: the tokens and logp of scnattn_rollout_pick on the same logits,
    (seed, draw, t) and K (no greedy_first)"""
    N, K = CONFIGS[cfg]
    for ld_extra in (0, 1):
        case = gen_case(V, cfg, ld_extra, 2, False, ld_extra)
        case["nmix"] = torch.full((N * K,), STEPS, dtype=torch.int32)
        mixed, plain = run_case(dev, case), run_case(dev, case, entry="plain")
        rows = (case["nsrc"] > 0).repeat_interleave(K)
        assert bool(rows.any())
        for k in ("token", "logp"):
            assert torch.equal(bits(mixed[k])[:, rows], bits(plain[k])[:, rows]), (ld_extra, k)
        assert torch.equal(bits(mixed["sum_logp"])[rows], bits(plain["sum_logp"])[rows])
        assert torch.equal(mixed["sample"][:, rows], mixed["token"][:, rows]) and bool((mixed["replaced"][:, rows] == 1).all())
        assert int(mixed["open_rows"]) == 0 and int(plain["open_rows"]) == int(rows.sum())


def test_same_seed_and_draw_same_bits_another_draw_another_coin(dev):
    case = gen_case(1027, "N2K8", 0, 1, False, 1)
    case["nmix"] = torch.full((16,), STEPS, dtype=torch.int32)
    a, b = run_case(dev, case), run_case(dev, case)
    c = run_case(dev, dict(case, draw=case["draw"] + 1))
    for k in ("token", "logp", "sample", "replaced", "sum_logp"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert not torch.equal(a["replaced"], c["replaced"])
    d = run_case(dev, dict(case, ld=case["ld"] + 1))                    # nor on the path that loads the row
    for k in ("token", "sample", "replaced"):
        assert torch.equal(a[k], d[k]), k


def test_gold_outside_the_vocabulary_is_recorded_as_given(dev):
    case = gen_case(257, "N1K1", 0, 0, False, 0)
    case["gold"] = torch.tensor([[-7], [257], [SENTI - 1]], dtype=torch.int32)
    got = run_case(dev, case)
    assert got["token"].reshape(-1).tolist() == case["gold"].reshape(-1).tolist()
    assert got["sample"].reshape(-1).tolist() == [-1] * 3 and not bool(got["replaced"].any()) and int(got["open_rows"]) == 0


def test_refusals(dev):
    V, R = 5, 3
    lb = GBuf(dev, (R, V), (V, 1), vals=torch.zeros(R, V))
    ib = GBufI(dev, R * STEPS, vals=torch.zeros(R * STEPS))
    fb = GBuf(dev, (R * STEPS,), vals=torch.zeros(R * STEPS), out=True)
    arr = (C.c_void_p * 7)(ib.ptr, ib.ptr, ib.ptr, ib.ptr, fb.ptr, ib.ptr, fb.ptr)
    tail = (STEPS, arr, ib.ptr, ib.ptr, ib.ptr)
    for args in ((1, 9, V, lb.ptr, V, 1.0, 0.5, SEED, 0, 0, 0) + tail,                 # K > 8
                 (1, 0, V, lb.ptr, V, 1.0, 0.5, SEED, 0, 0, 0) + tail,                 # K < 1
                 (1, 3, V, lb.ptr, V, 0.0, 0.5, SEED, 0, 0, 0) + tail,                 # inv_temp
                 (1, 3, V, lb.ptr, V, float("inf"), 0.5, SEED, 0, 0, 0) + tail,
                 (1, 3, V, lb.ptr, V, float("nan"), 0.5, SEED, 0, 0, 0) + tail,
                 (1, 3, V, lb.ptr, V, 1.0, -0.01, SEED, 0, 0, 0) + tail,               # prob
                 (1, 3, V, lb.ptr, V, 1.0, 1.01, SEED, 0, 0, 0) + tail,
                 (1, 3, V, lb.ptr, V, 1.0, float("nan"), SEED, 0, 0, 0) + tail,
                 (1, 3, V, lb.ptr, V - 1, 1.0, 0.5, SEED, 0, 0, 0) + tail,             # ld < V
                 (1, 3, V, lb.ptr, V, 1.0, 0.5, SEED, 0, STEPS, 0) + tail,             # step beyond the records
                 (1, 3, V, lb.ptr, V, 1.0, 0.5, SEED, 0, 0, 0, STEPS, arr, None, ib.ptr, ib.ptr),      # a null record
                 (1, 3, V, lb.ptr, V, 1.0, 0.5, SEED, 0, 0, 0, STEPS, arr, ib.ptr, ib.ptr, None)):
        with pytest.raises(RuntimeError):
            _call("scnattn_rollout_pick_mixed", dev, *args)
    assert bool((ib.read("untouched") == 0).all()) and bool((fb.read("untouched") == 0).all())
