"""The stem kernels of csrc/stem.hip -- scnattn_stem_tiles, scnattn_stem_conv7 (the persistent 7x7 / stride 2 implicit GEMM with
its statistics epilogue) and scnattn_stem_bn_relu_maxpool -- per element against the fp64 references of tests/stem_refs.py, one
entry point per call.

How a case is judged (the judges are stem_refs.judge_conv / judge_pool, the harness tests/kernel_harness.py):
  * x is a GBuf window in NaN with the strides of its memory format: NCHW, channels-last, or an NCHW view cropped out of a larger
    image (sh > W, NaN in the gaps); w likewise (NCHW, channels-last); z, the partials and the pooled map are windows in the
    sentinel.  The partial window is [2][64][workgroups] with row stride ldp = (workgroups + 3) & ~3: the slots [workgroups, ldp)
    must keep the sentinel;
  * z against fp64 conv2d with (147 + 8) u conv2d(|x|, |w|); slot b of the partials against the fp64 sums of the kernel's own
    stored z over the valid pixels of the tiles workgroup b walked (stem_refs.tile_walk); the pooled map within
    u max_window(|z scale| + |shift|) (bf16: the project's bf16 form), all-negative windows +0.0 bit for bit;
  * every case runs twice and gives the same bits; refusals return an error and leave the output as the sentinel.
The worst err / bound per (kernel, result) goes to the run's parity report; profiles/parity_report_bn_stem_kernels.txt keeps
a copy.
"""
import pytest
import torch

import stem_refs as S
from kernel_harness import GBuf, GBuf16, SENT, _bound_ok, _call, _write_report  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

REPORT_TITLE = "stem kernels vs fp64: worst |got - ref| / bound over all cases"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


def _bits(t):
    return t.float().contiguous().view(torch.int32)


def run_conv(dev, c, xs=None, bufs=None):
    from scnattn._lib import lib
    I = S.conv_inputs(c.N, c.H, c.W)
    Ho, Wo = S.out_hw(c.H, c.W)
    xs, wsd = xs or S.x_layout(c), S.w_layout(c)
    x = GBuf(dev, (c.N, 3, c.H, c.W), tuple(abs(s) for s in xs), I["x"])
    w = GBuf(dev, (64, 3, 7, 7), wsd, I["w"])
    z = GBuf(dev, (c.N * Ho * Wo, 64), None, out=True)
    nt = lib().scnattn_stem_tiles(c.N, c.H, c.W)
    assert nt == S.stem_tiles(c.N, c.H, c.W)
    ld = S.ldp(c.N, c.H, c.W)
    part = GBuf(dev, (2, 64, nt), (64 * ld, ld, 1), out=True) if c.stat else None
    shift = GBuf(dev, (64,), None, I["shift"]) if c.stat == 2 else None
    if bufs is not None:
        bufs += [z] + ([part] if part else [])
    _call("scnattn_stem_conv7", dev, c.N, c.H, c.W, x.ptr, *xs, w.ptr, *wsd, z.ptr, part.ptr if part else None,
          shift.ptr if shift else None)
    return {"z": z.read("z"), "partial": part.read("partial") if part else None}


def run_pool(dev, c, mis=0, bufs=None):
    I = S.pool_inputs(c)
    Ho, Wo = S.out_hw(c.Hz, c.Wz)
    z, ss = GBuf(dev, I["z"].shape, None, I["z"]), GBuf(dev, (c.C, 2), None, I["ss"])
    rows = c.N * Ho * Wo
    out = GBuf16(dev, rows, c.C) if c.obf else GBuf(dev, (rows, c.C), None, out=True, mis=mis)
    if bufs is not None:
        bufs.append(out)
    _call("scnattn_stem_bn_relu_maxpool", dev, c.N, c.Hz, c.Wz, c.C, z.ptr, ss.ptr, out.ptr, c.obf)
    return out.read("out").float()


@pytest.mark.parametrize("c", S.CONV_CASES, ids=S.case_id)
def test_stem_conv7(dev, c):
    a, b = run_conv(dev, c), run_conv(dev, c)
    assert torch.equal(_bits(a["z"]), _bits(b["z"])) and (a["partial"] is None or torch.equal(_bits(a["partial"]), _bits(b["partial"])))
    S.judge_conv(c, S.conv_inputs(c.N, c.H, c.W), a, "stem_conv7", _bound_ok)


@pytest.mark.parametrize("c", S.POOL_CASES, ids=S.case_id)
def test_stem_bn_relu_maxpool(dev, c):
    a, b = run_pool(dev, c), run_pool(dev, c)
    assert torch.equal(_bits(a), _bits(b))
    S.judge_pool(c, S.pool_inputs(c), a, "stem_bn_relu_maxpool<%s>" % ("bf16" if c.obf else "f32"), _bound_ok)


def test_stem_tiles(dev):
    from scnattn._lib import lib
    for (N, H, W) in [(1, 1, 1), (1, 33, 17), (3, 50, 70), (2, 17, 33), (767, 5, 5), (768, 5, 5), (770, 5, 5), (32, 256, 256)]:
        assert lib().scnattn_stem_tiles(N, H, W) == S.stem_tiles(N, H, W)


def _untouched(bufs):
    return all(bool((b.flat.cpu().view(torch.int32) == SENT).all()) for b in bufs)


def test_refuses_negative_strides(dev):
    c = S.CONV_CASES[3]
    sn, sc, sh, sw = S.x_layout(c)
    for xs in [(sn, sc, sh, -sw), (sn, sc, -sh, sw), (-sn, sc, sh, sw)]:
        bufs = []
        with pytest.raises(RuntimeError):
            run_conv(dev, c, xs=xs, bufs=bufs)
        assert bufs and _untouched(bufs)


def test_refuses_an_output_off_16_bytes(dev):
    bufs = []
    with pytest.raises(RuntimeError):
        run_pool(dev, S.POOL_CASES[0], mis=1, bufs=bufs)
    assert bufs and _untouched(bufs)
    bufs = []
    with pytest.raises(RuntimeError):
        run_pool(dev, S.POOL_CASES[0]._replace(C=6), bufs=bufs)       # C % 4 != 0: refused before any input is looked at
    assert bufs and _untouched(bufs)
