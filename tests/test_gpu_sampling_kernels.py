"""GPU tests (``-m gpu``) of the filtered pick of csrc/rollout.hip through the C ABI, alone: scnattn_rollout_pick_f per row
against the references of tests/sampling_refs.py (its docstring: the exact ORDER, the mass band and the accepted range of nkeep,
the key band of the token and the bound of logp GIVEN the device's nkeep), its book-keeping exactly.

Buffers are the guarded windows of tests/kernel_harness.py, as in tests/test_gpu_rollout_kernels.py: NaN around the logits and
in the gap ld - V of every row, the sentinel around and inside every record, nkeep included.  A run walks three steps on one
state, so rows close on the way; what a step must leave is derived from the DEVICE's own tokens once they have passed.  The
cases and their logits are stated in tests/sampling_cases.py, which the CPU module checks for the cap asserted here: in every
case at least 80 % of the judged rows are SHARP (one accepted nkeep); the rest are still judged, by range.

Shapes: V = 5 and 257 (fewer words than threads / just above), 1003 (odd), 1024 (exactly one group of four per thread), 2051
(the next register size), 10000 once (the largest); V = 2051 with force_passes and V = 20011 once for the global-memory path.  Rows, bases and temperatures: those of the plain pick's
module."""
import ctypes as C

import pytest
import torch

import sampling_cases as SC
import sampling_refs as SR
from kernel_harness import GBuf, GBufI, SENT, SENTI, _bound_ok, _call, _write_report      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = ("filtered rollout pick vs fp64: worst |got - ref| / bound over all cases (tests/sampling_refs.py: the mass "
                "band, the key band, the bound)")
STEPS = SC.STEPS


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


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
                logp=GBuf(dev, (STEPS, R), out=True), nkeep=GBufI(dev, STEPS * R))
    arr = (C.c_void_p * 7)(*[bufs[k].ptr for k in ("open_rows", "nsrc", "nopen", "length", "sum_logp", "token", "logp")])
    return bufs, arr, nsrc, length


def _run(dev, V, cfg, logits, mis, inv_temp, draw, top_k, top_p, force_passes=0, plain=False):
    """-> host copies of every state buffer after STEPS steps (guards checked); plain: scnattn_rollout_pick instead"""
    from scnattn import _lib
    N, K, greedy, closed = SC.CONFIGS[cfg]
    R = N * K
    ld = ((V + 3) // 4) * 4 + 4
    bufs, arr, nsrc0, len0 = _state(dev, N, K, closed)
    filt = _lib.SampleFilter(top_k=top_k, top_p=top_p)
    for t in range(STEPS):
        lb = GBuf(dev, (R, V), (ld, 1), vals=logits[t], mis=mis)
        if plain:
            _call("scnattn_rollout_pick", dev, N, K, V, lb.ptr, ld, inv_temp, SC.SEED, draw, t, int(greedy), V - 1, STEPS, arr)
        else:
            _call("scnattn_rollout_pick_f", dev, N, K, V, lb.ptr, ld, inv_temp, SC.SEED, draw, t, int(greedy), V - 1, STEPS, arr,
                  C.byref(filt), C.c_void_p(bufs["nkeep"].ptr.value + 4 * t * R), force_passes)
    got = {k: b.read(k) for k, b in bufs.items()}
    for k in ("token", "logp", "nkeep"):
        got[k] = got[k].view(STEPS, R)
    return got, nsrc0, len0


def _same_bits(a, b, keys=None):
    for k in keys or a:
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), k


def _judge_case(dev, name, V, cfg, runs, force_passes=0, twice=0):
    N, K, greedy, closed = SC.CONFIGS[cfg]
    R = N * K
    rows = n_sharp = n_closed_records = n_cut_ties = 0
    for ri, run in enumerate(runs):
        logits = SC.run_logits(V, cfg, run)
        inv_temp = SC.INV_TEMPS[run["it_idx"]]
        form = "rollout_pick_f %s%s" % ("vector" if run["mis"] == 0 else "scalar", " passes" if force_passes or V > 10240 else "")
        got, nsrc0, len0 = _run(dev, V, cfg, logits, run["mis"], inv_temp, run["draw"], run["top_k"], run["top_p"], force_passes)
        if ri == twice:                     # the same inputs, the same bits
            again, _, _ = _run(dev, V, cfg, logits, run["mis"], inv_temp, run["draw"], run["top_k"], run["top_p"], force_passes)
            _same_bits(got, again)
        ps = SC.reference_steps(V, cfg, run, logits)
        off = not 1 <= run["top_k"] < V and SR.f32(run["top_p"]) == 1.0      # e.g. top_k = 50 at V = 5: the plain kernel runs
        if off:
            assert bool((got["nkeep"] == SENTI).all()), "a filter that is off wrote nkeep"
        length, sum_logp = len0.clone(), torch.zeros(R)
        nopen, open_rows = nsrc0.clone(), int(nsrc0.sum())
        want_lp, bound_lp, got_lp = [], [], []
        for t in range(STEPS):
            p = ps[t]
            for r in range(R):
                n = r // K
                tok, lp, nk = int(got["token"][t, r]), got["logp"][t, r], int(got["nkeep"][t, r])
                where = "%s %s V=%d %r t=%d row %d" % (form, name, V, run, t, r)
                if nsrc0[n] == 0:           # a closed image: neither read nor written
                    assert tok == SENTI and int(lp.view(torch.int32)) == SENT and nk == SENTI, where
                    continue
                if length[r]:               # a closed row of an open image: <pad> / +0.0 / 0
                    assert tok == 0 and int(lp.view(torch.int32)) == 0 and nk == (SENTI if off else 0), (where, tok, float(lp), nk)
                    n_closed_records += 1
                    continue
                if off:
                    nk = V                  # the whole row: judged as a kept set of V words
                rows += 1
                k = p["kept"][r]
                n_sharp += int(k["sharp"])
                assert SR.nkeep_ok(p, r, nk), "%s: nkeep %d outside [%d, %d] (reference %d)" % (where, nk, k["lo"], k["hi"],
                                                                                                 k["nkeep"])
                y = p["y"][r]
                if nk < V and float(y[k["order"][nk - 1]]) == float(y[k["order"][nk]]):
                    n_cut_ties += 1         # equal values on both sides of the cut: the index decided
                assert SR.token_ok(p, r, tok, nk), "%s: token %d with nkeep %d (reference %d, band %.3e)" % (
                    where, tok, nk, int(p["token"][r]), SR.key_band(p, r))
                w, b = SR.logp_at_plain(p, r, tok) if off else SR.logp_at(p, r, tok, nk)
                want_lp.append(w), bound_lp.append(b), got_lp.append(float(lp))
                if nk == 1 and not off:
                    assert int(lp.view(torch.int32)) == 0, "%s: logp of a kept set of one is not +0.0" % where
                sum_logp[r] = sum_logp[r] + lp                                  # fp32, as the kernel adds
                if tok == V - 1:
                    length[r] = t + 1
                    nopen[n] -= 1
                    open_rows -= 1
        _bound_ok(form, "logp", torch.tensor(got_lp), torch.tensor(want_lp, dtype=torch.float64),
                  torch.tensor(bound_lp, dtype=torch.float64), "=u (|logp| + 2 dk + 8), dk = max |y - m| over the kept words")
        assert torch.equal(got["length"], length), (got["length"], length)
        assert torch.equal(got["sum_logp"].view(torch.int32), sum_logp.view(torch.int32)), (got["sum_logp"], sum_logp)
        assert torch.equal(got["nopen"], nopen) and torch.equal(got["nsrc"], nsrc0) and int(got["open_rows"]) == open_rows
    print("%s V=%d: %d rows judged, %d SHARP, %d with equal values across the cut, %d records of closed rows"
          % (name, V, rows, n_sharp, n_cut_ties, n_closed_records))
    assert n_sharp >= SC.SHARP_SHARE * rows, (n_sharp, rows)
    return rows, n_cut_ties, n_closed_records


@pytest.mark.parametrize("cfg", sorted(SC.CONFIGS))
@pytest.mark.parametrize("V", SC.VS)
def test_filtered_pick(dev, V, cfg):
    rows, ties, closed_records = _judge_case(dev, cfg, V, cfg, SC.runs_of(V, cfg))
    N, K, _, _ = SC.CONFIGS[cfg]
    assert closed_records > 0 or N * K == 1
    assert ties > 0 or V == 5, "no run of the case had equal values on both sides of a cut"


@pytest.mark.parametrize("name,V,cfg,which,force_passes,salt", SC.EXTRA, ids=[e[0] for e in SC.EXTRA])
def test_filtered_pick_large_and_passes(dev, name, V, cfg, which, force_passes, salt):
    _judge_case(dev, name, V, cfg, SC.runs_of(V, cfg, which, salt), force_passes)


@pytest.mark.parametrize("V", (1003, 2051))
def test_passes_and_register_paths_agree(dev, V):
    """the two ways to hold a row (registers, global-memory passes) add the same numbers in the same order: the same bits"""
    cfg = "R7"
    for run in SC.runs_of(V, cfg, (5, 7, 9), salt=7):
        logits = SC.run_logits(V, cfg, run)
        a, _, _ = _run(dev, V, cfg, logits, run["mis"], SC.INV_TEMPS[run["it_idx"]], run["draw"], run["top_k"], run["top_p"], 0)
        b, _, _ = _run(dev, V, cfg, logits, run["mis"], SC.INV_TEMPS[run["it_idx"]], run["draw"], run["top_k"], run["top_p"], 1)
        _same_bits(a, b)


@pytest.mark.parametrize("cfg", ("R7", "K3greedy"))
@pytest.mark.parametrize("V", (5, 1003, 2051))
def test_filter_off_leaves_the_bits_of_the_plain_pick(dev, V, cfg):
    """top_k 0 and >= V with top_p 1: every buffer holds what scnattn_rollout_pick leaves, and nkeep is not written"""
    N, K, greedy, _ = SC.CONFIGS[cfg]
    for mis in (0, 1):
        logits = SC.gen_logits(V, N, K, greedy, "u3", 40 + mis)
        want, _, _ = _run(dev, V, cfg, logits, mis, SC.INV_TEMPS[1], 3, 0, 1.0, plain=True)
        assert bool((want["nkeep"] == SENTI).all())
        for top_k in (0, V, V + 7):
            got, _, _ = _run(dev, V, cfg, logits, mis, SC.INV_TEMPS[1], 3, top_k, 1.0)
            _same_bits(got, want)


@pytest.mark.parametrize("V", (257, 2051))
def test_top_k_of_one_is_the_arg_max_with_logp_zero(dev, V):
    """noisy rows (no greedy slot): token = the first word of the ORDER, logp = +0.0 to the bit, nkeep = 1"""
    cfg = "R7"
    N, K, greedy, _ = SC.CONFIGS[cfg]
    for kind in ("u3", "quant"):
        logits = SC.gen_logits(V, N, K, greedy, kind, 50)
        got, _, len0 = _run(dev, V, cfg, logits, 0, SC.INV_TEMPS[1], 9, 1, 1.0)
        open_ = [True] * (N * K)
        for t in range(STEPS):
            y = SR.y32(logits[t], SC.INV_TEMPS[1])
            for r in range(N * K):
                if not open_[r]:
                    assert int(got["nkeep"][t, r]) == 0 and int(got["token"][t, r]) == 0
                    continue
                first = int(SR.order(y[r])[0])
                assert int(got["token"][t, r]) == first and int(got["nkeep"][t, r]) == 1, (kind, t, r)
                assert int(got["logp"][t, r].view(torch.int32)) == 0
                open_[r] = first != V - 1
        assert bool((got["sum_logp"].view(torch.int32) == 0).all())


def test_refusals_reach_no_kernel(dev):
    """a filter out of range and a null nkeep record are refused with every record left in the sentinel"""
    from scnattn import _lib
    V, cfg = 257, "R7"
    N, K, greedy, closed = SC.CONFIGS[cfg]
    bufs, arr, _, _ = _state(dev, N, K, closed)
    lb = GBuf(dev, (N * K, V), (V + 3, 1), vals=SC.gen_logits(V, N, K, greedy, "u3", 60)[0])
    for top_k, top_p, nk in ((-1, 1.0, True), (3, 0.0, True), (3, 1.5, True), (3, float("nan"), True), (3, -0.5, True),
                             (3, 0.9, False)):
        filt = _lib.SampleFilter(top_k=top_k, top_p=top_p)
        with pytest.raises(RuntimeError):
            _call("scnattn_rollout_pick_f", dev, N, K, V, lb.ptr, V + 3, 1.0, SC.SEED, 0, 0, 0, V - 1, STEPS, arr, C.byref(filt),
                  bufs["nkeep"].ptr if nk else None, 0)
    assert bool((bufs["token"].read("token") == SENTI).all()) and bool((bufs["nkeep"].read("nkeep") == SENTI).all())
