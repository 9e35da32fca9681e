"""GPU tests (``-m gpu``) of the two kernels of csrc/rollout.hip through the C ABI, each alone: scnattn_rollout_pick per row
against the fp64 reference of tests/rollout_refs.py (the band of the token, the bound of logp: its docstring), its
book-keeping exactly, and scnattn_rollout_advance bit for bit.

Buffers are guarded windows (tests/kernel_harness.py): NaN around the logits and in the gap ld - V of every row, the sentinel
around and inside every record.  A case walks three steps t = 0, 1, 2 on one state, so rows close on the way: a row closes when
it picks <end>, which the logits make likely on chosen rows of step 1 (and, at V = 5, anywhere).  What a step must leave is
derived from the DEVICE's own tokens once they have passed the band: length, sum_logp (the fp32 sum of the device's logp
records, bit for bit), the per-image and global open counters.

Shapes: V = 5 (below one sweep of the workgroup's 256 x 4 words), 1003 (odd), 1024 (exactly one sweep), 2051 (more than one);
R = 1, 7 and 3 images x 3 slots with greedy_first, image 1 of which is closed (nsrc = 0: its rows and records keep the
sentinel); the base 16-byte aligned with ld % 4 == 0 (the 16-byte loads, the last partial group scalar) and offset by one float
(the scalar path); inv_temp 1 and 1 / 0.7; another draw per combination."""
import ctypes as C

import pytest
import torch

import rollout_refs as RR
from kernel_harness import GBuf, GBufI, SENT, SENTI, _bound_ok, _call, _write_report      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "rollout kernels vs fp64: worst |got - ref| / bound over all cases (tests/rollout_refs.py: the band, the bound)"

SEED = 0x5eed0123456789ab
STEPS = 3
VS = (5, 1003, 1024, 2051)
# (N, K, greedy_first, closed image or None)
CONFIGS = {"R1": (1, 1, False, None), "R7": (7, 1, False, None), "K3greedy": (3, 3, True, 1), "K7greedy": (1, 7, True, None)}
INV_TEMPS = (1.0, float(torch.tensor(1.0 / 0.7, dtype=torch.float32)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def gen_logits(V, N, K, greedy_first, mis, it_idx):
    """STEPS x [R, V] logits uniform in +-3; exact ties at the top of every arg-max row at step 0 (two or three equal maxima);
    <end> = V - 1 raised on rows r % 3 == 1 at step 1"""
    g = torch.Generator().manual_seed(9000 + 7 * V + 131 * N + 17 * K + 3 * mis + it_idx)
    R = N * K
    out = []
    for t in range(STEPS):
        x = (torch.rand(R, V, generator=g) * 6 - 3).float()
        if t == 0 and greedy_first and V >= 5:
            for r in range(0, R, K):
                a = int(torch.randint(0, V - 3, (1,), generator=g))
                x[r, a + 1] = x[r, a + 3] = 3.5
                if r == 0:
                    x[r, V - 2] = 3.5
        if t == 1 and V > 5:
            x[1::3, V - 1] += 20.0
        out.append(x)
    return out


def _state(dev, N, K, closed):
    R = N * K
    nsrc = torch.full((N,), K, dtype=torch.int32)
    length = torch.zeros(R, dtype=torch.int32)
    if closed is not None:
        nsrc[closed] = 0
        length[closed * K:(closed + 1) * K] = 2
    nopen = nsrc.clone()
    bufs = dict(open_rows=GBufI(dev, 1, vals=torch.tensor([int(nopen.sum())])), nsrc=GBufI(dev, N, vals=nsrc),
                nopen=GBufI(dev, N, vals=nopen), length=GBufI(dev, R, vals=length),
                sum_logp=GBuf(dev, (R,), vals=torch.zeros(R), out=True), token=GBufI(dev, STEPS * R),
                logp=GBuf(dev, (STEPS, R), out=True))
    arr = (C.c_void_p * 7)(*[bufs[k].ptr for k in ("open_rows", "nsrc", "nopen", "length", "sum_logp", "token", "logp")])
    return bufs, arr, nsrc, length


def _run(dev, V, cfg, mis, it_idx, draw, logits=None, rows_N=None):
    """-> host copies of every state buffer after STEPS steps (guards checked)"""
    N, K, greedy, closed = cfg
    N = rows_N or N
    logits = logits or gen_logits(V, N, K, greedy, mis, it_idx)
    ld = ((V + 3) // 4) * 4 + 4
    bufs, arr, nsrc0, len0 = _state(dev, N, K, closed)
    for t in range(STEPS):
        lb = GBuf(dev, (N * K, V), (ld, 1), vals=logits[t], mis=mis)
        _call("scnattn_rollout_pick", dev, N, K, V, lb.ptr, ld, INV_TEMPS[it_idx], SEED, draw, t, int(greedy), V - 1, STEPS, arr)
    got = {k: b.read(k) for k, b in bufs.items()}
    got["token"] = got["token"].view(STEPS, N * K)
    got["logp"] = got["logp"].view(STEPS, N * K)
    return got, logits, nsrc0, len0


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("V", VS)
def test_rollout_pick(dev, V, cfg):
    N, K, greedy, closed = CONFIGS[cfg]
    R = N * K
    rows, n_amb, n_closed_records, n_ties = 0, 0, 0, 0
    for mis in (0, 1):
        for it_idx in (0, 1):
            draw = 1 + 2 * mis + it_idx
            got, logits, nsrc0, len0 = _run(dev, V, CONFIGS[cfg], mis, it_idx, draw)
            form = "rollout_pick %s" % ("vector" if mis == 0 else "scalar")
            length, sum_logp = len0.clone(), torch.zeros(R)
            nopen, open_rows = nsrc0.clone(), int(nsrc0.sum())
            want_lp, bound_lp, got_lp = [], [], []
            for t in range(STEPS):
                p = RR.pick(logits[t].double(), K, INV_TEMPS[it_idx], SEED, draw, t, greedy)
                amb = RR.ambiguous(p)
                for r in range(R):
                    n = r // K
                    tok, lp = int(got["token"][t, r]), got["logp"][t, r]
                    if nsrc0[n] == 0:           # a closed image: neither read nor written
                        assert tok == SENTI and int(lp.view(torch.int32)) == SENT, (t, r)
                        continue
                    if length[r]:               # a closed row of an open image: <pad> / +0.0
                        assert tok == 0 and int(lp.view(torch.int32)) == 0, (t, r, tok, float(lp))
                        n_closed_records += 1
                        continue
                    rows += 1
                    n_amb += int(amb[r])
                    assert RR.token_ok(p, r, tok), "%s V=%d t=%d row %d: token %d (reference %d, fp64 gap %.3e, band %.3e)" % (
                        form, V, t, r, tok, int(p["token"][r]), float(p["key"][r].double().max() - p["key"][r, tok]),
                        float(RR.band(p)[r]))
                    n_ties += int((p["key"][r] == p["key"][r, tok]).sum() > 1)
                    w, b = RR.logp_at(p, r, tok)
                    want_lp.append(w), bound_lp.append(b), got_lp.append(float(lp))
                    sum_logp[r] = sum_logp[r] + lp                                  # fp32, as the kernel adds
                    if tok == V - 1:
                        length[r] = t + 1
                        nopen[n] -= 1
                        open_rows -= 1
            _bound_ok(form, "logp", torch.tensor(got_lp), torch.tensor(want_lp, dtype=torch.float64),
                      torch.tensor(bound_lp, dtype=torch.float64),
                      "=u (|y_tok| + |lse| + 2 |log s| + |logp| + 4 (V + 8) + 2 dmax + 2)")
            assert torch.equal(got["length"], length), (got["length"], length)
            assert torch.equal(got["sum_logp"].view(torch.int32), sum_logp.view(torch.int32)), (got["sum_logp"], sum_logp)
            assert torch.equal(got["nopen"], nopen) and torch.equal(got["nsrc"], nsrc0) and int(got["open_rows"]) == open_rows
    print("%s V=%d: %d rows judged, %d ambiguous, %d rows with exactly equal keys at the pick, %d records of closed rows"
          % (cfg, V, rows, n_amb, n_ties, n_closed_records))
    assert 100 * n_amb <= rows
    assert n_closed_records > 0 or R == 1 and V > 5
    assert n_ties > 0 or not greedy or V < 5


def test_same_seed_and_draw_same_tokens_another_draw_other_tokens(dev):
    V, cfg = 1003, (7, 1, False, None)
    a, logits, _, _ = _run(dev, V, cfg, 0, 0, 5)
    b, _, _, _ = _run(dev, V, cfg, 0, 0, 5, logits=logits)
    c, _, _, _ = _run(dev, V, cfg, 0, 0, 6, logits=logits)
    assert torch.equal(a["token"], b["token"]) and torch.equal(a["logp"].view(torch.int32), b["logp"].view(torch.int32))
    assert not torch.equal(a["token"], c["token"])
    # row r does not depend on the number of rows: the first three alone
    d, _, _, _ = _run(dev, V, cfg, 0, 0, 5, logits=[x[:3].clone() for x in logits], rows_N=3)
    assert torch.equal(d["token"], a["token"][:, :3]) and torch.equal(d["logp"].view(torch.int32), a["logp"][:, :3].view(torch.int32))
    # nor on the path that loads it
    e, _, _, _ = _run(dev, V, cfg, 1, 0, 5, logits=logits)
    assert torch.equal(e["token"], a["token"])


@pytest.mark.parametrize("M", (5, 300))
def test_rollout_advance(dev, M):
    N, K, V = 3, 3, 11
    g = torch.Generator().manual_seed(70 + M)
    table = torch.randn(V, M, generator=g)
    tok = torch.tensor([0, 10, 3, SENTI, -4, 11, 7, 7, 1], dtype=torch.int32)      # a record never written, below, above the table
    nopen = torch.tensor([2, 0, 1], dtype=torch.int32)
    tb, eb = GBuf(dev, (V, M), vals=table, mis=1), GBuf(dev, (N * K, M), out=True, mis=1)
    kb, ob, sb = GBufI(dev, N * K, vals=tok), GBufI(dev, N, vals=nopen), GBufI(dev, N)
    _call("scnattn_rollout_advance", dev, N, K, M, V, kb.ptr, tb.ptr, eb.ptr, ob.ptr, sb.ptr)
    want = table[tok.long().clamp(0, V - 1)]
    assert torch.equal(eb.read("emb").view(torch.int32), want.view(torch.int32))
    assert sb.read("nsrc").tolist() == [K, 0, K] and ob.read("nopen").tolist() == nopen.tolist()
    assert kb.read("token").tolist() == tok.tolist()
