"""beam_row_topk_ens (csrc/beam.hip) through the C ABI, one launch per call, against the fp64 reference of
tests/ensemble_refs.py; buffers are guarded windows (tests/kernel_harness.py: sentinel around outputs, NaN around inputs
and in the rows of dead slots).

How a case is judged:
  * parity: M logits rows per live row, drawn from a fixed seed list until the fp64 top K+1 of every live row AND the top
    kk+1 of the merged candidates of the image are separated by at least 64 x the derived bound of score + c_v
    (ensemble_refs.value_bounds, derivation there) -- asserted on the CPU before the kernel is called; then the selected
    words must be EQUAL and the values within the bound.  Three images per case: all K sources live, nsrc < K, a finished
    image; rows of dead slots hold NaN and must be neither read into a result nor written.
  * bit-identity: mode 0 with one member and w = 1, and with the same row twice and w = (0.5, 0.5), writes the bits of
    scnattn_beam_row_topk on the same buffers, staged and unstaged.
  * ties: equal combined values leave in index order.  Every refusal of the entry point is exercised."""
import ctypes as C

import pytest
import torch

import beam_refs as BR
import ensemble_refs as ER
from kernel_harness import GBuf, NAN, SENT, _bound_ok, _call, _write_report  # noqa: F401  (the fixture)
from test_gpu_decoder_kernels import _gen

pytestmark = pytest.mark.gpu
REPORT_TITLE = "ensemble row selection vs fp64: worst |got - ref| / bound over all cases (tests/ensemble_refs.py: the bound)"
WEIGHTS = {1: None, 2: (0.625, 0.375), 4: (0.4, 0.3, 0.2, 0.1)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ints(dev, vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _live(nsrc, K):
    return torch.tensor([j < n for n in nsrc for j in range(K)])


def _untouched(buf, live, what):
    got = buf.read(what)
    dead = got[~live].view(torch.int32)
    assert bool((dead == SENT).all()), "%s: %d words of dead slots were written" % (what, int((dead != SENT).sum()))
    return got[live]


def _ld(V, kind):
    return V + 3 if kind == "scalar" else ((V + 3) & ~3) + 4


def _ens(dev, M, rows, lds, w, mode, K, V, N, b_s, nsrc_d, b_v, b_i, passes):
    """the call; rows: M GBuf windows"""
    pl = (C.c_void_p * M)(*[r.ptr.value if r is not None else None for r in rows])
    ll = (C.c_long * M)(*lds)
    wl = (C.c_float * M)(*w)
    _call("scnattn_beam_row_topk_ens", dev, N, K, V, M, pl, ll, wl, mode, b_s.ptr, C.c_void_p(nsrc_d.data_ptr()), b_v.ptr, b_i.ptr,
          passes)


def _draw(V, K, M, w, mode, nsrc, kk, seed0):
    """M logits [K,V] and scores [K] of ONE image, in the way test_gpu_beam_kernels._draw draws them: a head of min(2K, V)
    words above the bulk in every row -- the same words for every member, each member with its own step (0.5 + 0.1 m), jitter
    and bulk -- until the fp64 top K+1 of every live row and the merged top kk+1 are separated by >= 64 x the bound"""
    for seed in range(seed0, seed0 + 50):
        g = _gen(seed)
        logits = [(torch.randn(K, V, generator=g) * 3).float() for _ in range(M)]
        for j in range(K):
            head = torch.randperm(V, generator=g)[:2 * K]
            for m in range(M):
                logits[m][j, head] = 12.0 + (0.5 + 0.1 * m) * torch.arange(head.numel()) + 0.2 * torch.rand(head.numel(), generator=g)
        scores = (torch.randn(K, generator=g) * 2).float()
        l64, s64 = [x.double()[:nsrc] for x in logits], scores.double()[:nsrc]
        K1 = min(K + 1, V)
        cv, ci, _ = ER.row_topk_ens(l64, w, mode, s64, K1)
        _, bv = ER.value_bounds(l64, w, mode, s64)
        bound = float(bv.gather(1, ci).max())
        picks = BR.merge(cv[:, :K], ci[:, :K], V, min(kk + 1, nsrc * K))
        gaps = [picks[i][0] - picks[i + 1][0] for i in range(len(picks) - 1)]
        rowgaps = float((cv[:, :-1] - cv[:, 1:]).min()) if K1 > 1 else 1.0
        if all(gp >= 64 * bound for gp in gaps) and rowgaps >= 64 * bound:
            return logits, scores
    raise AssertionError("no seed separates the candidates")


CASES = [(V, K, M, mode, 0, ld) for V in (37, 1003, 1004, 10000) for K in (1, 3, 5, 8) for M in (1, 2, 4) for mode in (0, 1)
         for ld in ("scalar", "vector")] + \
        [(1003, K, M, mode, 1, ld) for K in (1, 3, 5, 8) for M in (1, 2, 4) for mode in (0, 1) for ld in ("scalar", "vector")]


@pytest.mark.parametrize("V,K,M,mode,passes,ldkind", CASES)
def test_row_topk_ens_vs_fp64(dev, V, K, M, mode, passes, ldkind):
    """words equal, values within the derived bound; passes = 1: every round recomputes c_v from the M global rows"""
    nsrc = [K, max(K - 2, 1), 0]
    kk = [K, max(K - 2, 1), 0]
    N, R = 3, 3 * K
    w = ER.member_weights(WEIGHTS[M], M)
    logits = [torch.zeros(N, K, V) for _ in range(M)]
    scores = torch.zeros(N, K)
    for n in range(2):
        lg, scores[n] = _draw(V, K, M, w, mode, nsrc[n], kk[n], 100 * V + 10 * K + n)
        for m in range(M):
            logits[m][n] = lg[m]
    live = _live(nsrc, K)
    ld = _ld(V, ldkind)
    rows = []
    for m in range(M):
        x = logits[m].reshape(R, V).clone()
        x[~live] = NAN
        rows.append(GBuf(dev, (R, V), (ld, 1), x))
    b_s = GBuf(dev, (R,), None, scores.reshape(R))
    b_v, b_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
    _ens(dev, M, rows, [ld] * M, w, mode, K, V, N, b_s, _ints(dev, nsrc), b_v, b_i, passes)
    gv = _untouched(b_v, live, "row values")
    gi = _untouched(b_i, live, "row words").view(torch.int32)
    l64 = [x.reshape(R, V).double()[live] for x in logits]
    s64 = scores.reshape(R).double()[live]
    cv, ci, _ = ER.row_topk_ens(l64, w, mode, s64, K)
    assert torch.equal(gi.long(), ci), "row top-K words differ"
    _, bv = ER.value_bounds(l64, w, mode, s64)
    _bound_ok("beam_row_topk_ens %s" % ("logprob", "prob")[mode], "value", gv, cv, bv.gather(1, ci),
              kind=("=sum_m w_m b_m + M u sum_m w_m |l_m|", "=max_m (b_m + u |d_m|) + (2M + 3) u + 2 u |log s| + u |c|")[mode] +
              " + 2 u (|score| + |c|), b_m = u ((V + 8) + 2 (|x_m| + |lse_m|))")


@pytest.mark.parametrize("V", [1003, 10000])
@pytest.mark.parametrize("passes", [0, 1])
@pytest.mark.parametrize("ldkind", ["scalar", "vector"])
def test_mode0_bits_of_beam_row_topk(dev, V, passes, ldkind):
    """one member with w = 1, and the same row twice with w = (0.5, 0.5): outv / outi bit for bit those of
    scnattn_beam_row_topk on the same buffers"""
    K, N = 5, 3
    nsrc = [K, 2, 0]
    R = N * K
    g = _gen(V + passes)
    x = (torch.randn(R, V, generator=g) * 4).float()
    x[:, 7] = x[:, 11]                  # ties inside a row do not disturb the identity
    sc = (torch.randn(R, generator=g) * 2).float()
    live = _live(nsrc, K)
    x[~live] = NAN
    ld = _ld(V, ldkind)
    b_l, b_s = GBuf(dev, (R, V), (ld, 1), x), GBuf(dev, (R,), None, sc)
    nsrc_d = _ints(dev, nsrc)
    r_v, r_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
    _call("scnattn_beam_row_topk", dev, N, K, V, b_l.ptr, ld, b_s.ptr, C.c_void_p(nsrc_d.data_ptr()), r_v.ptr, r_i.ptr, passes)
    want_v, want_i = r_v.read("values").view(torch.int32), r_i.read("words").view(torch.int32)
    assert bool((want_i[live] >= 0).all()) and bool((want_i[live] < V).all())
    for M, w in ((1, [1.0]), (2, [0.5, 0.5])):
        b_v, b_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
        _ens(dev, M, [b_l] * M, [ld] * M, w, 0, K, V, N, b_s, nsrc_d, b_v, b_i, passes)
        assert torch.equal(b_v.read("values").view(torch.int32), want_v), "M = %d: values differ in bits" % M
        assert torch.equal(b_i.read("words").view(torch.int32), want_i), "M = %d: words differ" % M


@pytest.mark.parametrize("mode", [0, 1])
def test_exact_ties_leave_in_index_order(dev, mode):
    """two members; duplicated logits inside both members' rows give equal combined values: lower word first, in the
    staged and in the unstaged path, and two identical live rows give identical candidates"""
    V, K, N = 37, 4, 1
    a = torch.linspace(-2, 1, V)
    b = torch.linspace(1, -1, V)
    for row in (a, b):
        row[[3, 9, 20]] = 2.5
        row[[5, 6]] = 2.0
    la = torch.stack([a, a, torch.full((V,), NAN), torch.full((V,), NAN)])
    lb = torch.stack([b, b, torch.full((V,), NAN), torch.full((V,), NAN)])
    scores = torch.tensor([-1.25, -1.25, 0.0, 0.0])
    nsrc = _ints(dev, [2])
    b_a, b_b, b_s = GBuf(dev, (K, V), None, la), GBuf(dev, (K, V), None, lb), GBuf(dev, (K,), None, scores)
    w = ER.member_weights((0.625, 0.375), 2)
    for passes in (0, 1):
        b_v, b_i = GBuf(dev, (K, K), None, out=True), GBuf(dev, (K, K), None, out=True)
        _ens(dev, 2, [b_a, b_b], [V, V], w, mode, K, V, N, b_s, nsrc, b_v, b_i, passes)
        gi, gv = b_i.read("words").view(torch.int32), b_v.read("values")
        assert gi[:2].tolist() == [[3, 9, 20, 5]] * 2
        assert torch.equal(gv[0], gv[1]) and float(gv[0, 0]) == float(gv[0, 2]) and float(gv[0, 2]) > float(gv[0, 3])
        assert bool((gi[2:] == SENT).all())


def test_refusals(dev):
    V, K, N = 16, 2, 1
    x = GBuf(dev, (N * K, V), None, torch.zeros(N * K, V))
    b_s = GBuf(dev, (N * K,), None, torch.zeros(N * K))
    nsrc = _ints(dev, [1])
    b_v, b_i = GBuf(dev, (N * K, K), None, out=True), GBuf(dev, (N * K, K), None, out=True)

    def go(M=2, K=K, V=V, rows=None, lds=None, w=None, mode=0):
        rows = [x] * max(M, 1) if rows is None else rows
        n = len(rows)
        pl = (C.c_void_p * n)(*[r.ptr.value if r is not None else None for r in rows])
        ll = (C.c_long * n)(*(lds or [16] * n))
        wl = (C.c_float * n)(*(w or [1.0 / n] * n))
        _call("scnattn_beam_row_topk_ens", dev, N, K, V, M, pl, ll, wl, mode, b_s.ptr, C.c_void_p(nsrc.data_ptr()), b_v.ptr,
              b_i.ptr, 0)

    go()                                                    # the arguments the refusals below vary are fine
    bad = [dict(M=0), dict(M=5, rows=[x] * 5), dict(K=0), dict(K=9), dict(V=1), dict(rows=[x, None]), dict(lds=[16, 15]),
           dict(w=[1.0, 0.0]), dict(w=[1.5, -0.5]), dict(w=[0.5, float("inf")]), dict(w=[0.5, NAN]), dict(mode=2),
           dict(mode=-1)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid argument|members"):
            go(**kw)
    b_v.read("values"), b_i.read("words")                  # ... and a refusal launches nothing: the one good call wrote
    assert int(b_i.read("words").view(torch.int32)[0, 0]) == 0
