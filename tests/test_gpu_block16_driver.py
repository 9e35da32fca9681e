"""GPU tests (``-m gpu``) of the drivers of the mixed-precision training Bottleneck: csrc/block16.cpp through the C ABI
(scnattn_block16_fwd, then scnattn_block16_bwd) and the two autograd nodes of scnattn/conv16.py, judged stage by stage
against fp64 with the chain-of-custody bounds of tests/block16_refs.py.

C ABI, direct.  Every buffer is a guarded window (tests/kernel_harness.py): inputs sit in NaN, the scratch is exactly as
large as the header says (part, bnpart: block16_refs.part_floats), and save, stats, tmp, dgb, each dw[i], part and bnpart sit
in the sentinel, inside and around.  Words the geometry does not use must keep it: stats / dgb rows past p for bn1 and bn2
and the downsample's row of an identity block, dx / dxd with need_dx == 0, the dw[i] of a NULL gradient.  Each case runs two
consecutive steps (the second step's shift is the first step's stored mean), each step twice (same bits), with need_dx = 0
(dres stays visible and is judged alone), with every dw NULL, and with a side stream; what the runs share is bit-equal.

Through autograd, in both BLOCK16 modes: y, dx (with the dxd scatter-add; per element one more bf16 rounding of the sum of
two judged maps), every gradient, the running statistics and num_batches_tracked are bit-equal to the judged C-ABI run of
the same inputs; so are the runs under four need patterns, with SIDE_WGRAD off, with flat-buffer gradients, with an fp32
NCHW dout, and a second backward(retain_graph=True) doubles every gradient exactly.

The worst err / bound per stage and geometry goes to the run's parity report;
profiles/parity_report_block16_driver.txt keeps a copy."""
import ctypes as C

import pytest
import torch
from torch import nn

import block16_refs as R
import conv_refs as CR
from kernel_harness import GBuf, GBuf16, SENT, SENT16

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT_TITLE = ("bf16 Bottleneck drivers (scnattn_block16_fwd / _bwd) vs fp64, stage by stage on the driver's own stored inputs: "
                "worst |got - ref| / bound per result and geometry, two steps; bounds: tests/block16_refs.py; a bit-for-bit "
                "check (dres, unused words, slot padding, mask mix, conditioning) prints 0.000 when it holds")
_WORST = {}             # (stage result, geometry) -> worst err / bound
_ABI = {}               # geometry -> [(state, S)] of the judged full C-ABI run, per step
GIDS = [g.id for g in R.GEOMS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    """two fp32 split workspaces (main, side) of WS_FLOATS with a marked tail that must survive the module"""
    t = torch.full((2, R.WS_FLOATS + 64), float("nan"), device=dev)
    t[:, R.WS_FLOATS:] = 12345.0
    yield t
    assert bool((t[:, R.WS_FLOATS:] == 12345.0).all()), "a split product wrote past the workspace it was given"


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    _WORST.clear()
    yield
    if not _WORST:
        return
    from test_gpu_parity import _report
    names = sorted({k[0] for k in _WORST})
    lines = ["%-34s " % "result" + " ".join("%-8s" % i for i in GIDS)]
    for n in names:
        lines.append("%-34s " % n + " ".join("%-8s" % ("%.3f" % _WORST[(n, i)] if (n, i) in _WORST else "-") for i in GIDS))
    _report(lines, REPORT_TITLE)


def _note(T):
    for k, v in T.ratios.items():
        _WORST[(k, T.gid)] = max(_WORST.get((k, T.gid), 0.0), v)


# ==== the C-ABI call on guarded windows ==================================================================================
def _sent32(buf):
    return bool((buf.flat.view(torch.int32) == SENT).all())


class _Windows:
    """every buffer of one step of a geometry and the scnattn_block16 that points at them"""

    def __init__(self, g, I, t, state, dev, ws, variant="full", side=None):
        from scnattn.conv16 import _Block16
        self.g, self.variant, self.side = g, variant, side
        need_dx, dws = R.VARIANTS[variant]
        d, cv = R.dims(g), R.carve(g)
        self.cv = cv
        b = self.b = _Block16(g.N, g.Cin, g.Hi, g.Wi, g.p, g.s, g.down)
        vec = lambda v: GBuf(dev, v.shape, vals=v)
        self.inp = []
        self.run_mean, self.run_var = [], []
        for i in range(d["nbn"]):
            vs = [vec(I["gamma"][i]), vec(I["beta"][i]), vec(state["shift"][i])]
            w = I["w"][i]
            ww = [GBuf16(dev, w.shape[0], w.shape[1] * w.shape[2], vals=w), GBuf16(dev, w.shape[2], w.shape[1] * w.shape[0], vals=I["wt"][i])]
            self.inp += vs + ww
            b.gamma[i], b.beta[i], b.shift[i] = (v.ptr.value for v in vs)
            b.w[i], b.wt[i] = ww[0].ptr, ww[1].ptr
            b.eps[i], b.momentum[i] = R.EPS[i], R.MOM[i]
            self.run_mean.append(GBuf(dev, (d["Cn"][i],), vals=state["run_mean"][i], out=True))
            self.run_var.append(GBuf(dev, (d["Cn"][i],), vals=state["run_var"][i], out=True))
            b.run_mean[i], b.run_var[i] = self.run_mean[i].ptr.value, self.run_var[i].ptr.value
        self.x = GBuf16(dev, d["Rin"], g.Cin, vals=I["x"][t])
        self.dout = GBuf16(dev, d["Rout"], d["C4"], vals=I["dout"][t])
        self.save, self.tmp = GBuf16(dev, 1, cv["save_elems"]), GBuf16(dev, 1, cv["tmp_elems"])
        self.stats, self.dgb = GBuf(dev, (cv["stats_floats"],), out=True), GBuf(dev, (cv["dgb_floats"],), out=True)
        self.part, self.bnpart = GBuf(dev, (R.part_floats(g),), out=True), GBuf(dev, (R.part_floats(g),), out=True)
        self.dw = [GBuf(dev, (I["w"][i].numel(),), out=True) for i in range(d["nbn"])]
        b.ws, b.ws_floats = ws[0].data_ptr(), R.WS_FLOATS
        b.part, b.bnpart, b.bnpart_floats = self.part.ptr.value, self.bnpart.ptr.value, R.part_floats(g)
        b.x, b.save, b.stats = self.x.ptr, self.save.ptr, self.stats.ptr.value
        b.dout, b.tmp, b.dgb = self.dout.ptr, self.tmp.ptr, self.dgb.ptr.value
        for i in range(d["nbn"]):
            b.dw[i] = self.dw[i].ptr.value if dws[i] else None
        b.need_dx = need_dx
        if side is not None:
            b.side_stream, b.side_ws, b.side_ws_floats = side.cuda_stream, ws[1].data_ptr(), R.WS_FLOATS

    def outputs(self):
        return [self.save, self.tmp] + [self.stats, self.dgb, self.part, self.bnpart] + self.dw

    def untouched(self):
        return self.save.untouched() and self.tmp.untouched() and all(_sent32(w) for w in self.outputs()[2:])


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _pieces(flat, table):
    return {name: flat[off:off + r * c].view(r, c) for name, (off, r, c) in table.items()}


def _run(g, I, t, state, dev, ws, variant="full", side=None):
    """forward, then backward -> S as block16_refs' judges take it, every window read back through its guard check"""
    from scnattn import _lib
    h = _lib.lib()
    W = _Windows(g, I, t, state, dev, ws, variant, side)
    need_dx, dws = R.VARIANTS[variant]
    d, cv = R.dims(g), W.cv
    assert h.scnattn_block16_fwd(_stream(dev), C.byref(W.b)) == 0, h.scnattn_last_error()
    torch.cuda.synchronize()
    S = _pieces(W.save.read("save")[0], cv["save"])
    S["stats"], S["part"], S["bnpart_fwd"] = W.stats.read("stats"), W.part.read("part"), W.bnpart.read("bnpart")
    S["run_mean"] = [v.read("run_mean") for v in W.run_mean]
    S["run_var"] = [v.read("run_var") for v in W.run_var]
    assert W.tmp.untouched() and _sent32(W.dgb) and all(_sent32(w) for w in W.dw), "the forward call wrote to a backward buffer"
    dxp, dxdp = C.c_void_p(1), C.c_void_p(1)
    assert h.scnattn_block16_bwd(_stream(dev), C.byref(W.b), C.byref(dxp), C.byref(dxdp)) == 0, h.scnattn_last_error()
    torch.cuda.synchronize()
    again = _pieces(W.save.read("save after the backward call")[0], cv["save"])
    assert all(torch.equal(S[k].view(torch.int16), again[k].view(torch.int16)) for k in again), "the backward call changed save"
    assert torch.equal(S["stats"].view(torch.int32), W.stats.read("stats").view(torch.int32)), "the backward call changed stats"
    tmp = _pieces(W.tmp.read("tmp")[0], cv["tmp"])
    at = lambda name: W.tmp.ptr + 2 * cv["tmp"][name][0]
    if not need_dx:
        assert dxp.value is None and dxdp.value is None, "need_dx == 0: dx_out / dxd_out must be NULL"
        for name in ("dx", "dxd"):
            if name in tmp:
                assert bool((tmp[name].view(torch.int16) == SENT16).all()), "need_dx == 0: %s was written" % name
                tmp[name] = None
    elif g.down:
        assert dxp.value == at("dx") and dxdp.value == at("dxd")
    else:
        assert dxp.value == at("dres") and dxdp.value is None, "an identity block: dx_out is dres, dxd_out NULL"
        tmp["dx"], tmp["dres"] = tmp["dres"], None
    S.update(tmp)
    S["dgb"], S["bnpart"] = W.dgb.read("dgb"), W.bnpart.read("bnpart")
    S["dw"] = [None] * 4
    for i, w in enumerate(W.dw):
        if dws[i]:
            S["dw"][i] = w.read("dw[%d]" % i).view(I["w"][i].shape[0], -1)
        else:
            assert _sent32(w), "dw[%d] is NULL for the call, its window was written" % i
    assert bool((W.part.read("part").view(torch.int32) == S["part"].view(torch.int32)).all()), "the backward call wrote to part"
    return S


def _bits(v):
    return v.contiguous().view(torch.int16 if v.dtype == BF else torch.int32)


def _same(a, b, what, skip=()):
    """every result both runs hold is bit-equal"""
    for k in a:
        if k in skip:
            continue
        va, vb = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for i, (p, q) in enumerate(zip(va, vb)):
            if p is None or q is None:
                continue
            assert torch.equal(_bits(p), _bits(q)), "%s: %s[%d] differs" % (what, k, i)


def _abi(g, dev, ws):
    """the judged full run of a geometry over the consecutive steps, once per module"""
    if g.id not in _ABI:
        I = R.inputs(g)
        state, out = R.first_state(I), []
        for t in range(R.STEPS):
            S = _run(g, I, t, state, dev, ws)
            T = R.judge_step(g, I, t, state, S)
            _note(T)
            for k, v in sorted(T.ratios.items()):
                print("%s step %d %s: worst err/bound %.3f" % (g.id, t, k, v))
            assert not T.fails, "%s step %d: %s" % (g.id, t, "; ".join(T.fails))
            out.append((state, S))
            state = R.next_state(g, S)
        _ABI[g.id] = out
    return _ABI[g.id]


@pytest.mark.parametrize("gid", GIDS)
def test_block16_c_abi_stage_by_stage_vs_fp64(dev, ws, gid):
    g = R.by_id(gid)
    I = R.inputs(g)
    side = torch.cuda.Stream(device=dev)
    for t, (state, S) in enumerate(_abi(g, dev, ws)):
        _same(S, _run(g, I, t, state, dev, ws), "%s step %d, two runs" % (gid, t))
        # need_dx = 0: dres stays visible and is judged on its own; dx_out / dxd_out NULL (checked in _run)
        Sn = _run(g, I, t, state, dev, ws, "no_dx")
        T = R.judge_bwd(g, I, t, Sn, "no_dx", R.Tally(gid))
        _note(T)
        assert not T.fails, "%s step %d need_dx = 0: %s" % (gid, t, "; ".join(T.fails))
        assert Sn["dres"] is not None
        _same(S, Sn, "%s step %d need_dx = 0" % (gid, t), skip=("dx", "dxd", "dres"))
        # every dw NULL: the windows keep the sentinel (checked in _run), the rest is the same
        _same(S, _run(g, I, t, state, dev, ws, "no_dw"), "%s step %d all dw NULL" % (gid, t), skip=("dw",))
        # weight gradients on a side stream
        _same(S, _run(g, I, t, state, dev, ws, "full", side), "%s step %d side stream" % (gid, t))


# ==== through autograd ===================================================================================================
PATTERNS = {"all": (True, (1, 1, 1, 1)), "x_no_grad": (False, (1, 1, 1, 1)), "convs_frozen": (True, (0, 0, 0, 0)),
            "conv2_frozen": (True, (1, 0, 1, 1))}


def _module(g, I, state, dev):
    """the Bottleneck of a geometry holding the case's operands: bf16-representable fp32 master weights, the BatchNorm vectors,
    eps, momenta, running statistics and conditioning shifts of the first step"""
    from scnattn import block as B, conv as SC
    from scnattn.resnet import Bottleneck, FusedBatchNorm2d
    d = R.dims(g)
    down = None
    if g.down:
        down = nn.Sequential(nn.Conv2d(g.Cin, d["C4"], kernel_size=1, stride=g.s, bias=False), FusedBatchNorm2d(d["C4"]))
    m = Bottleneck(g.Cin, g.p, g.s, down)
    with torch.no_grad():
        for i, (cv, bn) in enumerate(zip(B.convs(m), B.bns(m))):
            w = I["w"][i].float()
            k = 3 if w.shape[1] == 9 else 1
            cv.weight.copy_(w.view(w.shape[0], k, k, w.shape[2]).permute(0, 3, 1, 2))
            bn.weight.copy_(I["gamma"][i]); bn.bias.copy_(I["beta"][i])
            bn.running_mean.copy_(state["run_mean"][i]); bn.running_var.copy_(state["run_var"][i])
            bn.eps, bn.momentum = R.EPS[i], R.MOM[i]
    m = m.to(dev).to(memory_format=torch.channels_last).train()
    for i, bn in enumerate(B.bns(m)):
        SC._set_shift(bn, state["shift"][i].to(dev))
    return m


def _map4(t, N, H, W, dev):
    """[N*H*W][C] rows -> the (N, C, H, W) channels-last map on the GPU"""
    return t.to(dev).view(N, H, W, t.shape[1]).permute(0, 3, 1, 2)


def _rows(t4):
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1]).cpu()


def _autograd(g, dev, mode, pattern="all", side=True, flat=False, dout_fp32_nchw=False, sweeps=1):
    """the consecutive steps of a geometry through Bottleneck.forward / backward -> per step dict(out, dx, dw, dgb pairs,
    run_mean, run_var, nbt)"""
    from scnattn import block as B, conv as SC, conv16 as C16
    I = R.inputs(g)
    d = R.dims(g)
    x_grad, dws = PATTERNS[pattern]
    old = (C16.BLOCK16, SC.SIDE_WGRAD)
    res = []
    try:
        C16.BLOCK16, SC.SIDE_WGRAD = mode, side
        m = _module(g, I, R.first_state(I), dev)
        for cv, on in zip(B.convs(m), dws):
            cv.weight.requires_grad_(bool(on))
        opt = None
        if flat:
            from utils.optimizer import FusedClampAdam
            opt = FusedClampAdam([p for p in m.parameters() if p.requires_grad], lr=0.0, grad_clip=5.0)
        for t in range(R.STEPS):
            C16.refresh_weights(m)
            x4 = _map4(I["x"][t], g.N, g.Hi, g.Wi, dev).requires_grad_(x_grad)
            assert C16.bf16_reason(m, x4) is None, C16.bf16_reason(m, x4)
            for p in m.parameters():
                p.grad = None
            y = m(x4)
            assert y.dtype == BF
            dout = _map4(I["dout"][t], g.N, d["Ho"], d["Wo"], dev)
            if dout_fp32_nchw:
                dout = dout.float().contiguous()
            for k in range(sweeps):
                y.backward(dout, retain_graph=k + 1 < sweeps)
            if opt is not None:
                opt.flat.gather()
            torch.cuda.synchronize()
            out = {"out": _rows(y.detach()), "dx": _rows(x4.grad) if x_grad else None, "dw": [None] * 4, "dgb": [None] * 4}
            for i, (cv, bn) in enumerate(zip(B.convs(m), B.bns(m))):
                if dws[i]:
                    assert cv.weight.grad.dtype == torch.float32
                    out["dw"][i] = cv.weight.grad.permute(0, 2, 3, 1).reshape(cv.weight.shape[0], -1).cpu()
                out["dgb"][i] = torch.stack([bn.bias.grad, bn.weight.grad]).cpu()
            out["run_mean"] = [bn.running_mean.cpu() for bn in B.bns(m)]
            out["run_var"] = [bn.running_var.cpu() for bn in B.bns(m)]
            out["nbt"] = [int(bn.num_batches_tracked) for bn in B.bns(m)]
            res.append(out)
    finally:
        C16.BLOCK16, SC.SIDE_WGRAD = old
        SC.join_side_streams()
    return res


def _of_abi(g, S):
    """the C-ABI run's results in _autograd's form (dx with the caller's dxd add)"""
    d = R.dims(g)
    dgb = S["dgb"].view(4, 2, d["C4"])
    return {"out": S["out"], "dx": R.dx_sum(g, S["dx"], S["dxd"]) if g.down else S["dx"], "dw": S["dw"],
            "dgb": [dgb[i, :, :d["Cn"][i]] for i in range(d["nbn"])], "run_mean": S["run_mean"], "run_var": S["run_var"]}


def _equal(a, b, what, scale=1.0):
    """bit-equal results; scale: every gradient of b is that multiple of a's (exact for a power of two)"""
    for k in ("out", "run_mean", "run_var"):
        _same({k: a[k]}, {k: b[k]}, what)
    for k in ("dx", "dw", "dgb"):
        va, vb = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for i, (p, q) in enumerate(zip(va, vb)):
            if p is None or q is None:
                continue
            assert torch.equal(_bits(p * scale), _bits(q)), "%s: %s[%d] differs" % (what, k, i)


@pytest.mark.parametrize("mode", ["c", "py"])
@pytest.mark.parametrize("gid", GIDS)
def test_autograd_is_bit_equal_to_the_judged_c_abi_run(dev, ws, gid, mode):
    g = R.by_id(gid)
    abi = _abi(g, dev, ws)
    for t, got in enumerate(_autograd(g, dev, mode)):
        S = abi[t][1]
        _equal(_of_abi(g, S), got, "%s step %d BLOCK16=%s" % (gid, t, mode))
        assert got["nbt"] == [t + 1] * R.dims(g)["nbn"]
        if g.down:                                   # the final dx per element: one more rounding of the sum of two judged maps
            T = R.Tally(gid)
            want = R.dx_sum(g, S["dx"].double(), S["dxd"].double())
            T.ok("dx + dxd", "dx", got["dx"], want, (R.U8 + 2 * R.U) * want.abs())
            _note(T)
            assert not T.fails, T.fails


@pytest.mark.parametrize("pattern", ["x_no_grad", "convs_frozen", "conv2_frozen"])
@pytest.mark.parametrize("gid", GIDS)
def test_need_patterns_c_and_py_are_bit_identical(dev, ws, gid, pattern):
    """and what a pattern still computes is what the full run computed"""
    g = R.by_id(gid)
    abi = _abi(g, dev, ws)
    c, py = _autograd(g, dev, "c", pattern), _autograd(g, dev, "py", pattern)
    x_grad, dws = PATTERNS[pattern]
    for t in range(R.STEPS):
        _equal(c[t], py[t], "%s step %d %s c / py" % (gid, t, pattern))
        _equal(_of_abi(g, abi[t][1]), c[t], "%s step %d %s" % (gid, t, pattern))
        for r in (c[t], py[t]):
            assert (r["dx"] is not None) == x_grad
            assert [w is not None for w in r["dw"][:R.dims(g)["nbn"]]] == [bool(v) for v in dws[:R.dims(g)["nbn"]]]


@pytest.mark.parametrize("mode", ["c", "py"])
@pytest.mark.parametrize("gid", GIDS)
def test_side_stream_flat_gradients_fp32_dout_and_a_second_sweep(dev, ws, gid, mode):
    """SIDE_WGRAD off, flat-buffer gradients (FusedClampAdam), an fp32 NCHW dout of bf16-representable values: the bits of the
    judged run.  One forward and two backward(retain_graph=True) without zero_grad: exactly twice every gradient (doubling
    is exact; the second sweep takes _grad_out's fresh-tensor path and side_ok's join)."""
    g = R.by_id(gid)
    abi = _abi(g, dev, ws)
    for what, kw, scale in (("SIDE_WGRAD off", dict(side=False), 1.0), ("flat gradients", dict(flat=True), 1.0),
                            ("fp32 NCHW dout", dict(dout_fp32_nchw=True), 1.0), ("two sweeps", dict(sweeps=2), 2.0)):
        for t, got in enumerate(_autograd(g, dev, mode, **kw)):
            _equal(_of_abi(g, abi[t][1]), got, "%s step %d BLOCK16=%s %s" % (gid, t, mode, what), scale)


# ==== refusals ===========================================================================================================
def test_refusals_name_the_error_and_write_nothing(dev, ws):
    from scnattn import _lib
    h = _lib.lib()
    g = R.by_id("d1")
    I = R.inputs(g)
    d = R.dims(g)
    W = _Windows(g, I, 0, R.first_state(I), dev, ws)
    need_bnd = 2 * d["C4"] * CR.stat_ld(d["Rout"])
    assert g.id == R.REFUSAL_GEOM

    def mutated(**kw):
        from scnattn.conv16 import _Block16
        b = _Block16.from_buffer_copy(W.b)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(b, k)[v[0]] = v[1]
            else:
                setattr(b, k, v)
        return b

    for kw, calls, text in R.refusals(g):
        b = mutated(**kw)
        for which in calls:
            dxp, dxdp = C.c_void_p(1), C.c_void_p(1)
            rc = h.scnattn_block16_fwd(_stream(dev), C.byref(b)) if which == "fwd" else \
                h.scnattn_block16_bwd(_stream(dev), C.byref(b), C.byref(dxp), C.byref(dxdp))
            assert rc == -1, (kw, which)
            msg = h.scnattn_last_error()
            assert text in msg and b"block16" in msg, (kw, which, msg)
    torch.cuda.synchronize()
    assert W.untouched(), "a refused call wrote to an output window"
    for v in W.run_mean + W.run_var:
        v.read("running statistics")
    # the forward call needs no more of bnpart than the downsample's partials: that much is accepted
    b = mutated(bnpart_floats=need_bnd)
    assert h.scnattn_block16_fwd(_stream(dev), C.byref(b)) == 0, h.scnattn_last_error()
    torch.cuda.synchronize()
    W.bnpart.read("bnpart")
