"""The BatchNorm kernels of csrc/batchnorm.hip -- the chunk-major family (scnattn_bn_stats / _stats_fold / _apply / _bwd,
scnattn_bn_workspace_floats) and the finalize-on-load family (scnattn_bn_finalize / _apply_fin / _bwd_reduce / _bwd_dx_fin)
-- per element against the fp64 references of tests/bn_refs.py, on fp32 and bf16 maps, one entry point per call.

How a case is judged (the judges and their bounds are bn_refs.judge_*, the harness tests/kernel_harness.py):
  * every map, vector and partial is a guarded window: inputs in NaN -- the padding [nchunk, ldp) of an input partial too --
    outputs in the sentinel, inside too until written.  The maps are dense [R][C] (the ABI has no leading dimension), so their
    guards are the margins (Win); a partial's are also the slots [nchunk, ldp) and [ldp, ldp_cap); the workspace of bn_stats /
    bn_bwd is a window of exactly scnattn_bn_workspace_floats(C) floats whose words past nchunk * 2 * C keep the sentinel;
  * partial slots, finalize outputs, element-wise maps and the masked gradient: the tiers of bn_refs' docstring;
  * every case runs twice and gives the same bits (all sums are in fixed order); scnattn_bn_finalize gives the bits of
    scnattn_bn_apply_fin's statistics on the same partials; gout == dy (bn_bwd_reduce) and dz == g (bn_bwd_dx_fin) give the
    bits of the call without the alias;
  * refusals return an error and leave every output window as the sentinel.
The worst err / bound per (kernel, result) goes to the run's parity report; profiles/parity_report_bn_stem_kernels.txt keeps
a copy.  The dispatch the tables mirror is bn_refs.row_chunks / pick_chunks / ew_chunks / bwd_variant / reduce_variant;
tests/test_bn_stem_refs.py asserts without a GPU that every instance of bn_refs.REQUIRED is reached.
"""
import ctypes as ct

import pytest
import torch

import bn_refs as B
from kernel_harness import BF, GBuf, NAN, SENT, SENT16, _bound_ok, _call, _note, _write_report  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "BatchNorm kernels vs fp64: worst |got - ref| / bound over all cases"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


class Win:
    """A dense map (fp32 or bf16) with margins of 64 elements, without a per-element index: inputs in NaN, outputs
    (out=True; `vals`: the old contents of a window written in place) in the sentinel.  mis: elements the base is moved by."""

    def __init__(self, dev, shape, vals=None, bf16=0, out=False, mis=0):
        self.shape, self.n, self.bf16 = tuple(shape), int(torch.Size(shape).numel()), bf16
        dt, it, self.sent = (BF, torch.int16, SENT16) if bf16 else (torch.float32, torch.int32, SENT)
        self.it, self.lo = it, 64 + mis
        total = self.lo + self.n + 64
        host = torch.full((total,), self.sent, dtype=it).view(dt).clone() if out else torch.full((total,), NAN, dtype=dt)
        if vals is not None:
            host[self.lo:self.lo + self.n] = vals.reshape(-1).to(dt)
        self.flat = host.to(dev)
        assert self.flat.data_ptr() % 64 == 0
        self.ptr = ct.c_void_p(self.flat.data_ptr() + (2 if bf16 else 4) * self.lo)

    def read(self, what):
        host = self.flat.cpu()
        bits = host.view(self.it)
        guard = torch.cat([bits[:self.lo], bits[self.lo + self.n:]])
        assert bool((guard == self.sent).all()), "%s: %d guard elements overwritten" % (what, int((guard != self.sent).sum()))
        return host[self.lo:self.lo + self.n].view(self.shape).float()


def _untouched(b):
    it, sent = (torch.int16, SENT16) if b.flat.dtype == BF else (torch.int32, SENT)
    return bool((b.flat.cpu().view(it) == sent).all())


def _vec(dev, v):
    return GBuf(dev, v.shape, None, v)


def _vout(dev, shape, vals=None):
    return GBuf(dev, shape, None, vals, out=True)


def _p(b):
    return None if b is None else b.ptr


def _rd(b, what):
    return None if b is None else b.read(what)


def _ws(dev, C, nchunk):
    """the chunk-major workspace: a window [nchunk][2][C] at the front of exactly scnattn_bn_workspace_floats(C) floats"""
    from scnattn._lib import lib
    need = lib().scnattn_bn_workspace_floats(C)
    assert need == B.workspace_floats(C) and nchunk <= B.MAX_CHUNKS
    return GBuf(dev, (nchunk, 2, C), None, out=True, tail=need - nchunk * 2 * C)


def _bits(t):
    return t.float().contiguous().view(torch.int32)


def _same(a, b):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(_bits(a[k]), _bits(b[k])), "%s differs between two runs" % k
        else:
            assert a[k] == b[k], k


# ==== one call of each entry point =======================================================================================
def run_stats(dev, c):
    I = B.inputs(c)
    nchunk, _ = B.pick_chunks(c.R, c.C)
    x = Win(dev, (c.R, c.C), I["x"], c.bf16)
    ws, mean, invstd = _ws(dev, c.C, nchunk), _vout(dev, (c.C,)), _vout(dev, (c.C,))
    rm = _vout(dev, (c.C,), I["run_mean"]) if c.rm else None
    rv = _vout(dev, (c.C,), I["run_var"]) if c.rv else None
    ss = _vout(dev, (c.C, 2)) if c.fold else None
    if c.fold:
        ga, be = _vec(dev, I["gamma"]), _vec(dev, I["beta"])
        _call("scnattn_bn_stats_fold", dev, c.R, c.C, x.ptr, B.EPS, B.MOM, ws.ptr, mean.ptr, invstd.ptr, _p(rm), _p(rv), ga.ptr,
              be.ptr, ss.ptr)
    else:
        _call("scnattn_bn_stats", dev, c.R, c.C, x.ptr, c.bf16, B.EPS, B.MOM, ws.ptr, mean.ptr, invstd.ptr, _p(rm), _p(rv))
    return {"partial": ws.read("workspace"), "mean": mean.read("mean"), "invstd": invstd.read("invstd"),
            "run_mean": _rd(rm, "run_mean"), "run_var": _rd(rv, "run_var"), "ss": _rd(ss, "ss_out")}


def run_apply(dev, c):
    I = B.inputs(c)
    z, res = Win(dev, (c.R, c.C), I["z"], c.bf16), (Win(dev, (c.R, c.C), I["res"], c.bf16) if c.res else None)
    v = [_vec(dev, I[k]) for k in ("mean", "invstd", "gamma", "beta")]
    y = Win(dev, (c.R, c.C), None, c.bf16, out=True)
    _call("scnattn_bn_apply", dev, c.R, c.C, z.ptr, _p(res), c.bf16, v[0].ptr, v[1].ptr, v[2].ptr, v[3].ptr, c.relu, y.ptr)
    return {"y": y.read("y")}


def run_bwd(dev, c):
    I = B.inputs(c)
    nchunk, _ = B.pick_chunks(c.R, c.C)
    dy, z = Win(dev, (c.R, c.C), I["dy"], c.bf16), Win(dev, (c.R, c.C), I["z"], c.bf16)
    y = Win(dev, (c.R, c.C), I["y"], c.bf16) if c.y else None
    v = [_vec(dev, I[k]) for k in ("mean", "invstd", "gamma", "beta")]
    beta = v[3] if (c.relu and not c.y) else None            # needed for the mask from z only
    ws, dbeta, dgamma = _ws(dev, c.C, nchunk), _vout(dev, (c.C,)), _vout(dev, (c.C,))
    dz = Win(dev, (c.R, c.C), None, c.bf16, out=True) if c.dz else None
    dres = Win(dev, (c.R, c.C), None, c.bf16, out=True) if c.dres else None
    _call("scnattn_bn_bwd", dev, c.R, c.C, dy.ptr, _p(y), z.ptr, c.bf16, v[0].ptr, v[1].ptr, v[2].ptr, _p(beta), c.relu, c.train,
          ws.ptr, dbeta.ptr, dgamma.ptr, _p(dz), _p(dres))
    return {"partial": ws.read("workspace"), "dbeta": dbeta.read("dbeta"), "dgamma": dgamma.read("dgamma"),
            "dz": _rd(dz, "dz"), "dres": _rd(dres, "dres")}


def run_fin(dev, c, entry="scnattn_bn_apply_fin"):
    I = B.inputs(c)
    part = GBuf(dev, (2, c.C, c.ldp), None, I["partial"])          # NaN in [nchunk, ldp) and around
    shift = _vec(dev, I["shift"]) if c.shift else None
    ga, be = _vec(dev, I["gamma"]), _vec(dev, I["beta"])
    mean, invstd = _vout(dev, (c.C,)), _vout(dev, (c.C,))
    rm = _vout(dev, (c.C,), I["run_mean"]) if c.rm else None
    rv = _vout(dev, (c.C,), I["run_var"]) if c.rv else None
    ss = _vout(dev, (c.C, 2)) if c.ss else None
    y = None
    if entry == "scnattn_bn_finalize":
        _call(entry, dev, c.R, c.C, part.ptr, c.ldp, c.nchunk, _p(shift), B.EPS, B.MOM, mean.ptr, invstd.ptr, _p(rm), _p(rv),
              ga.ptr if c.ss else None, be.ptr if c.ss else None, _p(ss))
    else:
        z, res = Win(dev, (c.R, c.C), I["z"], c.bf16), (Win(dev, (c.R, c.C), I["res"], c.bf16) if c.res else None)
        y = Win(dev, (c.R, c.C), None, c.bf16, out=True)
        _call(entry, dev, c.R, c.C, z.ptr, _p(res), c.bf16, part.ptr, c.ldp, c.nchunk, _p(shift), B.EPS, B.MOM, ga.ptr, be.ptr,
              c.relu, y.ptr, mean.ptr, invstd.ptr, _p(rm), _p(rv), _p(ss))
    return {"y": _rd(y, "y"), "mean": mean.read("mean"), "invstd": invstd.read("invstd"), "run_mean": _rd(rm, "run_mean"),
            "run_var": _rd(rv, "run_var"), "ss": _rd(ss, "ss_out")}


def run_reduce(dev, c, alias=None):
    I = B.inputs(c)
    alias = c.alias if alias is None else alias
    nchunk, _ = B.pick_chunks(c.R, c.C)
    ldp = B.ldp_of(nchunk)
    cap = ldp + c.cap
    z = Win(dev, (c.R, c.C), I["z"], c.bf16)
    y = Win(dev, (c.R, c.C), I["y"], c.bf16) if c.relu else None
    gout = None
    if alias:
        dy = gout = Win(dev, (c.R, c.C), I["dy"], c.bf16, out=True)      # in place: margins in the sentinel
    else:
        dy = Win(dev, (c.R, c.C), I["dy"], c.bf16)
        if c.gout:
            gout = Win(dev, (c.R, c.C), None, c.bf16, out=True)
    mean, invstd = _vec(dev, I["mean"]), _vec(dev, I["invstd"])
    part = GBuf(dev, (2, c.C, nchunk), (c.C * ldp, ldp, 1), out=True, tail=2 * c.C * cap + 64)   # [ldp, ldp_cap) lies in the tail
    nch = ct.c_int(-1)
    _call("scnattn_bn_bwd_reduce", dev, c.R, c.C, dy.ptr, _p(y), z.ptr, c.bf16, mean.ptr, invstd.ptr, c.relu, part.ptr, cap,
          _p(gout), ct.byref(nch))
    return {"partial": part.read("partial"), "gout": _rd(gout, "gout"), "nchunk": nch.value}


def run_dxfin(dev, c, alias=None):
    I = B.inputs(c)
    alias = c.alias if alias is None else alias
    part = GBuf(dev, (2, c.C, c.ldp), None, I["partial"])
    z = Win(dev, (c.R, c.C), I["z"], c.bf16)
    if alias:
        g = dz = Win(dev, (c.R, c.C), I["g"], c.bf16, out=True)
    else:
        g, dz = Win(dev, (c.R, c.C), I["g"], c.bf16), Win(dev, (c.R, c.C), None, c.bf16, out=True)
    v = [_vec(dev, I[k]) for k in ("mean", "invstd", "gamma")]
    dbeta, dgamma = _vout(dev, (c.C,)), _vout(dev, (c.C,))
    _call("scnattn_bn_bwd_dx_fin", dev, c.R, c.C, g.ptr, z.ptr, c.bf16, v[0].ptr, v[1].ptr, v[2].ptr, part.ptr, c.ldp, c.nchunk,
          dbeta.ptr, dgamma.ptr, dz.ptr)
    return {"dbeta": dbeta.read("dbeta"), "dgamma": dgamma.read("dgamma"), "dz": dz.read("dz")}


def _twice(run, dev, c):
    a, b = run(dev, c), run(dev, c)
    _same(a, b)
    return a


# ==== per element ========================================================================================================
@pytest.mark.parametrize("c", B.STATS_CASES, ids=B.case_id)
def test_bn_stats(dev, c):
    B.judge_stats(c, B.inputs(c), _twice(run_stats, dev, c), B.kernel_of(c), _bound_ok, note=_note)


@pytest.mark.parametrize("c", B.APPLY_CASES, ids=B.case_id)
def test_bn_apply(dev, c):
    B.judge_apply(c, B.inputs(c), _twice(run_apply, dev, c), B.kernel_of(c), _bound_ok)


@pytest.mark.parametrize("c", B.BWD_CASES, ids=B.case_id)
def test_bn_bwd(dev, c):
    B.judge_bwd(c, B.inputs(c), _twice(run_bwd, dev, c), B.kernel_of(c), _bound_ok)


@pytest.mark.parametrize("c", B.FIN_CASES, ids=B.case_id)
def test_bn_apply_fin(dev, c):
    out = _twice(run_fin, dev, c)
    B.judge_fin(c, B.inputs(c), out, B.kernel_of(c), _bound_ok)
    fin = run_fin(dev, c, "scnattn_bn_finalize")               # statistics only: the same bits, judged under its own name
    for k in ("mean", "invstd", "run_mean", "run_var", "ss"):
        assert (out[k] is None and fin[k] is None) or torch.equal(_bits(out[k]), _bits(fin[k])), k
    B.judge_fin(c, B.inputs(c), fin, "bn_finalize", _bound_ok)


@pytest.mark.parametrize("c", B.REDUCE_CASES, ids=B.case_id)
def test_bn_bwd_reduce(dev, c):
    out = _twice(run_reduce, dev, c)
    B.judge_reduce(c, B.inputs(c), out, B.kernel_of(c), _bound_ok)
    if c.alias:
        _same(out, run_reduce(dev, c, alias=0))


@pytest.mark.parametrize("c", B.DXFIN_CASES, ids=B.case_id)
def test_bn_bwd_dx_fin(dev, c):
    out = _twice(run_dxfin, dev, c)
    B.judge_dxfin(c, B.inputs(c), out, B.kernel_of(c), _bound_ok)
    if c.alias:
        _same(out, run_dxfin(dev, c, alias=0))


def test_workspace_floats(dev):
    from scnattn._lib import lib
    for C in (4, 8, 64, 72, 2048):
        assert lib().scnattn_bn_workspace_floats(C) == B.workspace_floats(C)


# ==== refusals: host-side argument checks, nothing is launched ===========================================================
class _Kit:
    """operands of a small call (R = 32, one chunk): every output window starts as the sentinel"""
    R, C = 32, 8

    def __init__(self, dev, bf16=0, mis=0, pmis=0):
        g = torch.Generator().manual_seed(7)
        R, C = self.R, self.C
        self.bf16 = bf16
        for k in ("z", "res", "dy", "y"):
            setattr(self, k, Win(dev, (R, C), torch.randn(R, C, generator=g), bf16, mis=mis if k == "z" else 0))
        for k in ("mean", "invstd", "gamma", "beta", "shift"):
            setattr(self, k, _vec(dev, 0.5 + torch.rand(C, generator=g)))
        self.pin = GBuf(dev, (2, C, 8), None, torch.rand(2, C, 8, generator=g), mis=pmis)
        self.o1, self.o2 = Win(dev, (R, C), None, bf16, out=True), Win(dev, (R, C), None, bf16, out=True)
        self.omis = Win(dev, (R, C), None, bf16, out=True, mis=1)
        self.v = [_vout(dev, (C,)) for _ in range(4)]
        self.ss, self.pout = _vout(dev, (C, 2)), _vout(dev, (2, C, 8))
        self.ws = _vout(dev, (B.workspace_floats(C),))
        self.outs = [self.o1, self.o2, self.omis, self.ss, self.pout, self.ws] + self.v


def _stats(k, C=None, x=None):
    return ("scnattn_bn_stats", k.R, C or k.C, (x or k.z).ptr, k.bf16, B.EPS, B.MOM, k.ws.ptr, k.v[0].ptr, k.v[1].ptr, None, None)


def _fin(k, C=None, ldp=8, nchunk=5, z=None, y=None, shift=None, rm=None):
    return ("scnattn_bn_apply_fin", k.R, C or k.C, (z or k.z).ptr, None, k.bf16, k.pin.ptr, ldp, nchunk, _p(shift), B.EPS, B.MOM,
            k.gamma.ptr, k.beta.ptr, 1, (y or k.o1).ptr, k.v[0].ptr, k.v[1].ptr, _p(rm), None, None)


def _finalize(k, ldp=8, nchunk=5, gamma=True, ss=False):
    return ("scnattn_bn_finalize", k.R, k.C, k.pin.ptr, ldp, nchunk, None, B.EPS, B.MOM, k.v[0].ptr, k.v[1].ptr, None, None,
            k.gamma.ptr if gamma else None, k.beta.ptr if gamma else None, k.ss.ptr if ss else None)


def _dxfin(k, C=None, ldp=8, nchunk=5, g=None, dz=None):
    return ("scnattn_bn_bwd_dx_fin", k.R, C or k.C, (g or k.dy).ptr, k.z.ptr if g is None else k.res.ptr, k.bf16, k.mean.ptr,
            k.invstd.ptr, k.gamma.ptr, k.pin.ptr, ldp, nchunk, k.v[0].ptr, k.v[1].ptr, (dz or k.o1).ptr)


def _reduce(k, C=None, relu=1, y=True, gout=True, cap=8):
    return ("scnattn_bn_bwd_reduce", k.R, C or k.C, k.dy.ptr, k.y.ptr if y else None, k.res.ptr, k.bf16, k.mean.ptr, k.invstd.ptr,
            relu, k.pout.ptr, cap, k.o1.ptr if gout else None, None)


def _bwd(k, C=None, y=True, beta=True):
    return ("scnattn_bn_bwd", k.R, C or k.C, k.dy.ptr, k.y.ptr if y else None, k.res.ptr, k.bf16, k.mean.ptr, k.invstd.ptr,
            k.gamma.ptr, k.beta.ptr if beta else None, 1, 1, k.ws.ptr, k.v[0].ptr, k.v[1].ptr, k.o1.ptr, k.o2.ptr)


# (what, kit arguments, the call)
REFUSALS = [
    ("C % 4 != 0 in bn_stats", {}, lambda k: _stats(k, C=6)),
    ("C % 4 != 0 in bn_apply", {}, lambda k: ("scnattn_bn_apply", k.R, 6, k.res.ptr, None, 0, k.mean.ptr, k.invstd.ptr, k.gamma.ptr,
                                              k.beta.ptr, 1, k.o1.ptr)),
    ("C % 4 != 0 in bn_bwd", {}, lambda k: _bwd(k, C=6)),
    ("C % 4 != 0 in bn_apply_fin", {}, lambda k: _fin(k, C=6)),
    ("C % 4 != 0 in bn_bwd_reduce", {}, lambda k: _reduce(k, C=6)),
    ("C % 4 != 0 in bn_bwd_dx_fin", {}, lambda k: _dxfin(k, C=6)),
    ("x 4 bytes off in bn_stats", {"mis": 1}, _stats),
    ("x 2 bytes off in bn_stats", {"mis": 1, "bf16": 1}, _stats),
    ("z 4 bytes off in bn_apply_fin", {"mis": 1}, _fin),
    ("z 2 bytes off in bn_apply_fin", {"mis": 1, "bf16": 1}, _fin),
    ("y 4 bytes off in bn_apply_fin", {}, lambda k: _fin(k, z=k.res, y=k.omis)),
    ("g 4 bytes off in bn_bwd_dx_fin", {"mis": 1}, lambda k: _dxfin(k, g=k.z)),
    ("g 2 bytes off in bn_bwd_dx_fin", {"mis": 1, "bf16": 1}, lambda k: _dxfin(k, g=k.z)),
    ("dz 2 bytes off in bn_bwd_dx_fin", {"bf16": 1}, lambda k: _dxfin(k, dz=k.omis)),
    ("ldp < nchunk in bn_apply_fin", {}, lambda k: _fin(k, z=k.res, ldp=4, nchunk=5)),
    ("ldp < nchunk in bn_finalize", {}, lambda k: _finalize(k, ldp=4, nchunk=5)),
    ("ldp < nchunk in bn_bwd_dx_fin", {}, lambda k: _dxfin(k, ldp=4, nchunk=5)),
    ("ldp % 4 != 0 in bn_apply_fin", {}, lambda k: _fin(k, z=k.res, ldp=6)),
    ("ldp % 4 != 0 in bn_finalize", {}, lambda k: _finalize(k, ldp=6)),
    ("ldp % 4 != 0 in bn_bwd_dx_fin", {}, lambda k: _dxfin(k, ldp=6)),
    ("partial not 16-byte aligned in bn_apply_fin", {"pmis": 1}, lambda k: _fin(k, z=k.res)),
    ("partial not 16-byte aligned in bn_finalize", {"pmis": 1}, _finalize),
    ("partial not 16-byte aligned in bn_bwd_dx_fin", {"pmis": 1}, _dxfin),
    ("shift == run_mean", {}, lambda k: _fin(k, z=k.res, shift=k.shift, rm=k.shift)),
    ("ss_out without gamma / beta in bn_finalize", {}, lambda k: _finalize(k, gamma=False, ss=True)),
    ("ss_out without gamma / beta in bn_stats_fold", {}, lambda k: ("scnattn_bn_stats_fold", k.R, k.C, k.res.ptr, B.EPS, B.MOM, k.ws.ptr,
                                                                    k.v[0].ptr, k.v[1].ptr, None, None, None, None, k.ss.ptr)),
    ("relu without y and beta in bn_bwd", {}, lambda k: _bwd(k, y=False, beta=False)),
    ("relu without y in bn_bwd_reduce", {}, lambda k: _reduce(k, y=False)),
    ("ldp_cap too small", {}, lambda k: _reduce(k, cap=0)),
    ("gout without relu in bn_bwd_reduce", {}, lambda k: _reduce(k, relu=0, y=False, gout=True)),
]


@pytest.mark.parametrize("what,kit,args", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_refusals(dev, what, kit, args):
    k = _Kit(dev, **kit)
    before = k.shift.flat.clone()
    name, *rest = args(k)
    with pytest.raises(RuntimeError):
        _call(name, dev, *rest)
    torch.cuda.synchronize()
    for b in k.outs:
        assert _untouched(b), what
    assert torch.equal(k.shift.flat.view(torch.int32), before.view(torch.int32)), what
