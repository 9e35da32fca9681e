"""The two forms of one BatchNorm expression must give the same bits (``-m gpu``, fp32, through the C ABI).

csrc/batchnorm.hip evaluates the forward expression bn_norm(z) = fma((z - mean) * invstd, gamma, beta) in the apply kernels
of both generations and recomputes it for the ReLU mask of the backward pass; all of them call the one definition in
csrc/tile.h.  Nothing else states the contract that follows from it:
  (a) a backward pass that recomputes the mask from z gives the bits of one that reads the mask from the forward output y;
  (b) scnattn_bn_apply_fin (statistics finalized inside) gives the bits of scnattn_bn_apply on the statistics it returned.
Shapes: (300, 72) ragged last row chunk, partial 64-column block, the min(c, C - 4) clamp; (70, 2048) many column blocks,
one chunk; (4200, 8) more than 64 channel-major and more than 16 chunk-major partials per channel."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(300, 72), (70, 2048), (4200, 8)]
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


def _inputs(R, Cc, dev):
    g = torch.Generator().manual_seed(100 + R + Cc)
    z = (torch.randn(R, Cc, generator=g) * 1.5 + 0.3).to(dev)
    res = torch.randn(R, Cc, generator=g).to(dev)
    dy = torch.randn(R, Cc, generator=g).to(dev)
    gamma = (1 + 0.3 * torch.randn(Cc, generator=g)).to(dev)      # both signs of gamma occur at C = 72 and 2048
    beta = (0.2 * torch.randn(Cc, generator=g)).to(dev)
    return z, res, dy, gamma, beta


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_mask_recomputed_from_z_gives_the_bits_of_the_mask_read_from_y(dev, R, Cc):
    from scnattn._lib import lib, check
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    z, _, dy, gamma, beta = _inputs(R, Cc, dev)
    ws = torch.empty(L.scnattn_bn_workspace_floats(Cc), device=dev)
    mean, invstd = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
    check(L.scnattn_bn_stats(st, R, Cc, z.data_ptr(), 0, EPS, 0.1, ws.data_ptr(), mean.data_ptr(), invstd.data_ptr(), None, None),
          "scnattn_bn_stats")
    y = torch.empty_like(z)
    check(L.scnattn_bn_apply(st, R, Cc, z.data_ptr(), None, 0, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                             beta.data_ptr(), 1, y.data_ptr()), "scnattn_bn_apply")
    assert 0.2 < (y > 0).float().mean().item() < 0.8, "the mask must cut something and keep something"
    for train in (1, 0):
        got = {}
        for form, yp in (("y", y.data_ptr()), ("z", None)):
            dz = torch.empty_like(z)
            dbeta, dgamma = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
            check(L.scnattn_bn_bwd(st, R, Cc, dy.data_ptr(), yp, z.data_ptr(), 0, mean.data_ptr(), invstd.data_ptr(),
                                   gamma.data_ptr(), beta.data_ptr(), 1, train, ws.data_ptr(), dbeta.data_ptr(),
                                   dgamma.data_ptr(), dz.data_ptr(), None), "scnattn_bn_bwd")
            got[form] = (dz, dbeta, dgamma)
        for name, a, b in zip(("dz", "dbeta", "dgamma"), got["y"], got["z"]):
            assert _same_bits(a, b), "%s differs between the two mask forms (train=%d)" % (name, train)


@pytest.mark.parametrize("R,Cc", SHAPES)
def test_apply_fin_gives_the_bits_of_apply_on_the_statistics_it_returned(dev, R, Cc):
    from scnattn._lib import lib, check
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    z, res, _, gamma, beta = _inputs(R, Cc, dev)
    # channel-major partials [2][C][ldp] of sum(z - s), sum((z - s)^2) per 64-row block, as a producer's epilogue leaves them
    shift = z[:64].mean(0).contiguous()
    n = (R + 63) // 64
    ldp = (n + 3) & ~3
    d = torch.cat([z - shift, torch.zeros(n * 64 - R, Cc, device=dev)]).view(n, 64, Cc)
    part = torch.full((2, Cc, ldp), float("nan"), device=dev)       # the padding past n must never be read into a sum
    part[0, :, :n] = d.sum(1).t()
    part[1, :, :n] = (d * d).sum(1).t()
    for relu in (0, 1):
        for r in (None, res):
            y1, y2 = torch.empty_like(z), torch.empty_like(z)
            mean, invstd = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
            check(L.scnattn_bn_apply_fin(st, R, Cc, z.data_ptr(), None if r is None else r.data_ptr(), 0, part.data_ptr(), ldp, n,
                                         shift.data_ptr(), EPS, 0.1, gamma.data_ptr(), beta.data_ptr(), relu, y1.data_ptr(),
                                         mean.data_ptr(), invstd.data_ptr(), None, None, None), "scnattn_bn_apply_fin")
            check(L.scnattn_bn_apply(st, R, Cc, z.data_ptr(), None if r is None else r.data_ptr(), 0, mean.data_ptr(),
                                     invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), relu, y2.data_ptr()), "scnattn_bn_apply")
            assert torch.isfinite(y1).all()
            assert (mean - z.mean(0)).abs().max().item() <= 1e-4, "apply_fin's statistics are not those of z"
            assert _same_bits(y1, y2), "apply_fin and apply differ (relu=%d, residual=%s)" % (relu, r is not None)
