"""What the per-kernel GPU test modules share (tests/test_gpu_decoder_kernels.py, tests/test_gpu_attn_variant_kernels.py,
tests/test_gpu_gemm_kernels.py,
tests/test_gpu_bn_kernels.py, tests/test_gpu_stem_kernels.py, tests/test_gpu_seq_driver.py, and for the bf16 windows tests/test_gpu_eval16_kernels.py,
tests/test_gpu_conv16_kernels.py): guarded buffers, the C-ABI call, the
per-element sum judge and the parity-report fixture.  How a case is judged: DESIGN.md 3.
A plain module (tests/ is on sys.path, like decoder_kernel_refs); a test module imports `_write_report` by name to get
its own table in the run's parity report."""
import ctypes as C

import pytest
import torch

U = 2.0 ** -24
SENT = 0x7FC5A5A5          # a quiet-NaN bit pattern: a kernel that reads its own output margin poisons its result too
NAN = float("nan")
SENT16 = 0x7FC5            # the same for bf16 windows (GBuf16)
BF = torch.bfloat16


# ---- report -------------------------------------------------------------------------------------------------------------
_STATS = {}     # (kernel, result) -> [worst ratio, kind, worst yardstick, cases]


def _note(kernel, name, ratio, kind, yard=0.0):
    s = _STATS.setdefault((kernel, name), [0.0, kind, 0.0, 0])
    s[0], s[2], s[3] = max(s[0], ratio), max(s[2], yard), s[3] + 1


@pytest.fixture(scope="module", autouse=True)
def _write_report(request):
    """Module-scoped: a test module imports it by name; its REPORT_TITLE heads the table (the decode-step title otherwise).
    A `kind` that starts with "=" is the bound's own description and is printed as it stands."""
    _STATS.clear()
    yield
    if not _STATS:
        return
    from test_gpu_parity import _report
    w = max([18] + [len(k[0]) for k in _STATS])
    fmt = "%%-%ds %%-10s %%-9s %%-6s %%s" % w
    lines = [fmt % ("kernel", "result", "err/bound", "cases", "bound")]
    for (kern, name), (ratio, kind, yard, n) in sorted(_STATS.items()):
        how = kind[1:] if kind.startswith("=") else "(n+8)*2^-24*sum|terms|" if kind == "sum" else \
            "(n+16)*2^-24*(sum|terms|*|scale|+|mean*scale|+|beta|+|res|)" \
            if kind == "eval" else \
            "4 x rho x row max, rho = CPU-fp32 worst row-relative error [%.3e]; rows below 1e-6 x tensor max: 4 x CPU-fp32 " \
            "worst element error" % yard if kind == "row" else \
            "min(4 x CPU-fp32 worst element error [worst seen %.3e], %s x row max)" % (yard, kind)
        lines.append(fmt.replace("%-9s %-6s", "%-9.3f %-6d") % (kern, name, ratio, n, how))
    _report(lines, getattr(request.module, "REPORT_TITLE",
                           "decode-step primitives vs fp64: worst |got - ref| / bound over all cases"))
    _STATS.clear()


# ---- guarded buffers ----------------------------------------------------------------------------------------------------
class GBuf:
    """A strided window `shape` / `strides` (elements) inside a flat allocation: 16 floats (+ `mis`) in front, `tail` behind.
    Inputs: NaN everywhere outside the window.  Outputs (out=True): the sentinel everywhere (window included unless `vals`
    is given: accumulators), checked by read().  mis = 1 offsets the base by one float (not 16-byte aligned)."""

    def __init__(self, dev, shape, strides=None, vals=None, out=False, mis=0, tail=64):
        shape = tuple(int(n) for n in shape)
        if strides is None:                                   # dense
            strides, acc = [], 1
            for n in reversed(shape):
                strides.insert(0, acc)
                acc *= n
        self.base = 16 + mis
        span = 1 + sum((n - 1) * int(s) for n, s in zip(shape, strides))
        total = self.base + span + int(tail)
        if out:
            host = torch.full((total,), SENT, dtype=torch.int32).view(torch.float32).clone()
        else:
            host = torch.full((total,), NAN, dtype=torch.float32)
        pos = torch.zeros((), dtype=torch.long) + self.base
        for n, s in zip(shape, strides):
            pos = pos.unsqueeze(-1) + torch.arange(n) * int(s)
        assert pos.numel() == pos.unique().numel(), "overlapping window"
        self.pos, self.out = pos, out
        if vals is not None:
            host[pos] = vals.to(torch.float32).expand(shape)
        self.flat = host.to(dev)
        assert self.flat.data_ptr() % 64 == 0
        self.ptr = C.c_void_p(self.flat.data_ptr() + 4 * self.base)

    def read(self, what):
        host = self.flat.cpu()
        guard = torch.ones(host.numel(), dtype=torch.bool)
        guard[self.pos.reshape(-1)] = False
        bad = (host.view(torch.int32)[guard] != SENT).nonzero().reshape(-1)
        assert bad.numel() == 0, "%s: %d guard words overwritten (first at window offset %d)" % (
            what, bad.numel(), int(guard.nonzero().reshape(-1)[bad[0]]) - self.base)
        return host[self.pos]


class GBig:
    """GBuf for a dense window of `n` floats that is too large to build and compare on the host (a workspace with its GEMM
    partials): filled and checked on the device.  16 sentinel floats in front, `tail` behind, the window filled with `fill`
    (a float, NaN included) or left in the sentinel; read() proves the margins intact and returns the window (host)."""

    def __init__(self, dev, n, fill=None, tail=64):
        self.base, self.n = 16, int(n)
        self.flat = torch.empty(self.base + self.n + int(tail), dtype=torch.float32, device=dev)
        self.flat.view(torch.int32).fill_(SENT)
        assert self.flat.data_ptr() % 64 == 0
        self.ptr = C.c_void_p(self.flat.data_ptr() + 4 * self.base)
        self.window = self.flat[self.base:self.base + self.n]
        if fill is not None:
            self.window.fill_(fill)

    def check(self, what):
        words = self.flat.view(torch.int32)
        bad = int((words[:self.base] != SENT).sum()) + int((words[self.base + self.n:] != SENT).sum())
        assert bad == 0, "%s: %d guard words overwritten" % (what, bad)

    def read(self, what):
        self.check(what)
        return self.window.cpu()


class GBuf16:
    """A [rows][cols] bf16 window with leading dimension `ld` inside a flat allocation, 64 elements in front and behind.
    Inputs: NaN everywhere outside the window (and in [cols, ld)).  Outputs (vals None, or out=True with the old values of
    an accumulated-into window): the sentinel everywhere else.  mis offsets the base by that many elements (1: not 4-byte
    aligned, 2: 4-byte but not 8-byte aligned)."""

    def __init__(self, dev, rows, cols, ld=None, vals=None, out=False, mis=0):
        ld = ld or cols
        self.base, self.rows, self.cols, self.ld = 64 + mis, rows, cols, ld
        total = self.base + (rows - 1) * ld + cols + 64
        if vals is None or out:
            host = torch.full((total,), SENT16, dtype=torch.int16).view(BF).clone()
        else:
            host = torch.full((total,), float("nan"), dtype=BF)
        self.pos = (self.base + torch.arange(rows).unsqueeze(1) * ld + torch.arange(cols)).reshape(-1)
        if vals is not None:
            host[self.pos] = vals.reshape(-1)
        self.flat = host.to(dev)
        assert self.flat.data_ptr() % 64 == 0
        self.ptr = self.flat.data_ptr() + 2 * self.base

    def read(self, what):
        host = self.flat.cpu()
        guard = torch.ones(host.numel(), dtype=torch.bool)
        guard[self.pos] = False
        bad = (host.view(torch.int16)[guard] != SENT16).nonzero().reshape(-1)
        assert bad.numel() == 0, "%s: %d guard elements overwritten" % (what, bad.numel())
        return host[self.pos].view(self.rows, self.cols)

    def untouched(self):
        return bool((self.flat.view(torch.int16) == SENT16).all())


SENTI = 0x5A5AA5A5         # the sentinel of integer windows (GBufI): no token, length or flag a test uses


class GBufI:
    """A dense window of `n` int32 (or int64: wide=True) elements, 16 in front and behind, the sentinel everywhere (an
    integer has no NaN) except where `vals` are given; read() proves the margins intact."""

    def __init__(self, dev, n, vals=None, wide=False):
        self.n, self.dtype = int(n), torch.int64 if wide else torch.int32
        host = torch.full((self.n + 32,), SENTI, dtype=self.dtype)
        if vals is not None:
            host[16:16 + self.n] = vals.reshape(-1).to(self.dtype)
        self.flat = host.to(dev)
        self.ptr = C.c_void_p(self.flat.data_ptr() + (8 if wide else 4) * 16)

    def read(self, what):
        host = self.flat.cpu()
        assert bool((host[:16] == SENTI).all()) and bool((host[16 + self.n:] == SENTI).all()), \
            "%s: guard words overwritten" % what
        return host[16:16 + self.n]


CPU = torch.device("cpu")


def _call(name, dev, *args, arm=False):
    """The C-ABI call on the GPU `dev`, synchronised.  With dev = CPU nothing runs: the same arguments (host windows of the
    same alignment and leading dimensions) go through scnattn_plan_next and the launch plan of the call is returned -- what
    the library would launch, from the library; a refusal raises the same RuntimeError either way.  arm: the same query with
    the GPU's own windows and stream."""
    from scnattn._lib import call, plan
    if dev.type == "cpu":
        return plan(name, None, *args)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    got = plan(name, st, *args) if arm else call(name, st, *args)
    torch.cuda.synchronize()
    return got


# ---- judging ------------------------------------------------------------------------------------------------------------
def _sum_ok(kernel, name, got, ref):
    """|got - ref| <= (n + 8) * 2^-24 * S per element"""
    want, bound = ref[name].double(), (ref[name + "_n"] + 8) * U * ref[name + "_abs"].double()
    got = got.double().reshape(want.shape)
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s %s: worst err/bound %.3f (n = %d)" % (kernel, name, worst, ref[name + "_n"]))
    assert bool((err <= bound).all()), "%s %s: worst err/bound %.3f at %d, %d NaN" % (
        kernel, name, worst, int(ratio.reshape(-1).nan_to_num(1e30).argmax()), int(got.isnan().sum()))
    _note(kernel, name, worst, "sum")


def _bound_ok(kernel, name, got, want, bound, kind="sum"):
    """|got - want| <= bound per element, for a bound the caller derived (per-slot partials, per-tap n, the eval epilogue);
    an element whose bound is 0 must be equal, a NaN (an output word never written) fails"""
    want, bound = want.double(), bound.double().expand(want.shape)
    got = got.double().reshape(want.shape)
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30)
    worst = float(ratio.nan_to_num(1e30).max()) if ratio.numel() else 0.0
    print("%s %s: worst err/bound %.3f" % (kernel, name, worst))
    assert bool((err <= bound).all()), "%s %s: worst err/bound %.3f at %d, %d NaN" % (
        kernel, name, worst, int(ratio.reshape(-1).nan_to_num(1e30).argmax()), int(got.isnan().sum()))
    _note(kernel, name, worst, kind)


def _slab_buf(dev, vals, extra_ld=3, extra_stride=5):
    """vals [n, rows, W] -> window with ld = W + extra_ld, slab stride = rows * ld + extra_stride, one NaN slab behind"""
    n, rows, W = vals.shape
    ld = W + extra_ld
    stride = rows * ld + extra_stride
    return GBuf(dev, vals.shape, (stride, ld, 1), vals, tail=stride + 64), stride, ld
