"""The fp64 GEMM references (tests/gemm_refs.py), the judge and the case tables of tests/test_gpu_gemm_kernels.py, without a GPU:
  * the references equal torch.einsum in fp64;
  * the bound is attainable: the same product evaluated in fp32 on the CPU (torch.matmul; slice by slice for the skinny
    slabs) passes the judge at every table row -- the bound excludes nothing a correct fp32 evaluation produces;
  * the judge is sensitive: an fp32 result with one planted defect fails;
  * the library itself says which instance every row reaches: the row's own call goes through scnattn_plan_next on host
    windows (test_gpu_gemm_kernels.skinny_plan / dense_plan), gemm_refs.skinny_name / dense_name render the plan; every
    row reaches the instance its `inst` names and every instance the GPU module lists is reached by a row."""
import pytest
import torch

import gemm_refs as R
import test_gpu_gemm_kernels as T
from kernel_harness import U, _sum_ok

SKINNY_IDS = ["%d-%s-%dx%dx%d-ks%d" % (i, r.form, r.rows, r.N, r.K, r.ks) for i, r in enumerate(T.SKINNY)]
DENSE_IDS = ["%d-%s" % (i, T._dense_id(r)) for i, r in enumerate(T.DENSE)]
cdiv = R.cdiv


def _fails(kernel, name, got, ref):
    with pytest.raises(AssertionError, match="worst err/bound"):
        _sum_ok(kernel, name, got, ref)


# ==== the dispatch, asked of the library ===============================================================================
_PLANS = {}


def skinny_dispatch(r):
    """-> (inst, ksplit the call runs with, XVEC) from the launch plan of the row's own call"""
    if r not in _PLANS:
        p, ks = T.skinny_plan(r)
        _PLANS[r] = (R.skinny_name(p), ks, bool(p.vec))
    return _PLANS[r]


def dense_dispatch(r):
    """-> (inst, dict(S, kper, K)) from the launch plan of the row's own call"""
    key = T._dense_id(r) + repr((r.lay, r.ws, sorted(r.opts.items())))
    if key not in _PLANS:
        p = T.dense_plan(r)
        _PLANS[key] = (R.dense_name(p), dict(S=p.S, kper=p.kper, K=r.K))
    return _PLANS[key]


# ==== tables =============================================================================================================
@pytest.mark.parametrize("r", T.SKINNY, ids=SKINNY_IDS)
def test_skinny_rows_reach_the_instance_they_name(r):
    inst, ks, xvec = skinny_dispatch(r)
    assert inst == r.inst
    assert inst.startswith("nb%d c%d " % R.skinny_blocking(r.K, ks, r.form)[1:3])      # the slices the references are cut by
    # XVEC is false for exactly the cause the row names: with that one cause taken away the same call loads 16 bytes
    assert xvec == (not r.x), "XVEC is %s, the row says %r" % (xvec, r.x)
    L = T.sk_layout(r)
    if r.x == "K":
        assert (r.K % 4 or r.K < 4) and not L["mis"] and L["ldx"] % 4 == 0 and L["xg"] % 4 == 0
    elif r.x:
        assert r.K % 4 == 0 and r.K >= 4 and skinny_dispatch(r._replace(x=""))[2], "%r is not the only cause" % r.x
    assert L["xg"] > r.K and L["ldx"] > (r.groups - 1) * L["xg"] + r.K and L["ldw"] > r.N and L["wg"] > r.K * L["ldw"]
    assert L["ldy"] > r.N and L["yg"] > r.rows * L["ldy"] and L["yslab"] > r.groups * L["yg"]


def test_skinny_table_covers_every_instance():
    seen = {}
    for r in T.SKINNY:
        inst, ks, xvec = skinny_dispatch(r)
        nb, chunks, v, e, z = (int(t[1 if t[0] in "cvez" else 2:]) for t in inst.split())
        causes = {r.x} if r.x else set()            # test_skinny_rows_reach_the_instance_they_name holds the row to it
        seen.setdefault(r.form, []).append((nb, chunks, v, e, z, frozenset(causes), r))
    for form, nbs in (("f32", range(1, 9)), ("bf16w", range(1, 9)), ("bf16", (2, 4, 6, 8))):
        rows = seen[form]
        assert {t[0] for t in rows} == set(nbs), form                       # every NB
        assert {t[2] for t in rows} == {0, 1}, form                         # XVEC true and false
        assert {t[1] for t in rows} >= {1, 2}, form                         # the several-chunk loop
        assert {t[4] for t in rows} >= {1, 2}, form                         # grid.z > 1
        assert any(t[3] > 0 for t in rows), form                            # empty K-slices
    allrows = [t for rows in seen.values() for t in rows]
    for cause in ("mis", "ldx", "xg", "K"):
        assert any(t[5] == {cause} for t in allrows), cause                 # each cause of XVEC = false on its own
    assert any(t[6].K < 4 for t in allrows)
    assert {t[1] for t in allrows} >= {1, 2, 4}
    assert {t[6].rows for t in allrows} >= {1, 31, 32, 33, 40}
    assert {t[6].N for t in allrows} >= {1, 31, 32, 33, 45, 4608}
    assert {t[6].groups for t in allrows} == {1, 4}
    assert {t[6].ks for t in allrows} >= {0, 1, 2, 3, 16}
    assert any(t[6].K == 33 and t[6].ks == 16 and t[3] == 14 for t in allrows)
    assert any(t[6].K == 40 and t[6].ks == 2 for t in allrows)
    for K in (9, 33, 77, 128, 132, 192, 200, 256):
        assert {r.form for r in T.SKINNY if r.K == K and r.ks == 1} >= {"f32", "bf16w"}, K
    old = {(32, 128, 512, 1, 0), (32, 2048, 2048, 1, 0), (7, 45, 77, 1, 3), (32, 512, 1024, 4, 0), (5, 36, 40, 4, 2),
           (1, 33, 9, 1, 1), (40, 64, 128, 1, 2), (32, 4608, 512, 1, 4), (32, 512, 4608, 1, 16)}     # the shapes of test_gpu_parity.py
    assert old <= {(r.rows, r.N, r.K, r.groups, r.ks) for r in T.SKINNY}


@pytest.mark.parametrize("r", T.DENSE, ids=DENSE_IDS)
def test_dense_rows_reach_the_instance_they_name(r):
    inst, _ = dense_dispatch(r)
    assert inst == r.inst
    L = T.dg_layout(r)
    if "tn" not in r.lay:
        assert L["lda"] > L["wA"] and L["ldb"] > L["wB"] and L["sA"] > L["hA"] * L["lda"] and L["sB"] > L["hB"] * L["ldb"]
    assert L["ldc"] > r.N and L["sC"] > r.M * L["ldc"]


def test_dense_table_covers_every_instance():
    rows = [(r, dense_dispatch(r)) for r in T.DENSE]
    inst = {r.inst for r in T.DENSE}
    lay = lambda r: (r.ta, r.tb)
    every = {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {lay(r) for r in T.DENSE if r.inst.startswith("sgemm v0")} == every
    assert {lay(r) for r in T.DENSE if r.inst.startswith("sgemm v1")} == every
    for mi in (1, 2, 4):
        assert {lay(r) for r in T.DENSE if r.inst.startswith("cgemm mi%d" % mi)} == every, mi
        assert any(r.inst.startswith("cgemm mi%d" % mi) and r.inst.endswith("sst") for r in T.DENSE) or mi == 2
        assert any(r.inst.startswith("cgemm mi%d" % mi) and (r.opts.get("force_mi") == mi or r.opts.get("cgemm_mi") == mi)
                   for r in T.DENSE), mi
    assert any(r.inst.endswith("sst") for r in T.DENSE) and any(r.inst.endswith("vst") for r in T.DENSE)
    for cause in ("ldc1", "C1"):
        assert any(cause in r.lay and r.inst.endswith("sst") for r in T.DENSE), cause
    assert any(r.tb and r.N % 4 and r.inst.startswith("cgemm") and r.inst.endswith("sst") for r in T.DENSE)
    for cause in ("A1", "lda1"):
        assert any(cause in r.lay and r.inst.startswith("sgemm v0") for r in T.DENSE), cause
    # split-K: un-split, in-launch combine, the reduce launch entered three ways, short last slice, the --S loop, ws = NULL
    assert any(" S1 " in r.inst for r in T.DENSE) and any(" comb " in r.inst for r in T.DENSE)
    assert "cgemm mi1 S16 red vst" in inst                                                     # S = 16
    assert any(r.opts.get("cgemm_combine") == 0 and " red " in r.inst and "S16" not in r.inst for r in T.DENSE)
    assert any(r.inst.endswith("red sst") for r in T.DENSE)                                    # creduce_kernel<false>
    assert any(r.inst.startswith("cgemm mi4") and " comb " in r.inst and "B" in r.epi and "m" in r.epi for r in T.DENSE)
    assert any(" comb " in r.inst and r.epi == "abBm" for r in T.DENSE)
    assert any(r.batch > 1 and d["S"] > 1 for r, (i, d) in rows if i.startswith("cgemm"))
    assert any(r.batch > 1 and d["S"] > 1 for r, (i, d) in rows if i.startswith("sgemm"))
    for fam in ("sgemm", "cgemm"):
        assert any(i.startswith(fam) and d["S"] > 1 and d["K"] % d["kper"] for r, (i, d) in rows), fam     # short last slice
        assert any(i.startswith(fam) and isinstance(r.ws, int) and d["S"] == r.ws for r, (i, d) in rows), fam   # --S loop
        assert any(i.startswith(fam) and r.ws == "null" and r.K >= 2048 for r, (i, d) in rows), fam
    assert any(i == "sgemm v0 S2" and r.K == 256 for r, (i, d) in rows)                        # tiles <= 16, kmin 128
    assert any(i.startswith("sgemm") and d["S"] > 1 and r.K == 512 and
               cdiv(r.M, 128) * cdiv(r.N, 128) * r.batch > 16 for r, (i, d) in rows)           # tiles > 16, kmin 256
    assert "sgemm v1 S16" in inst                                                              # splitk_reduce_kernel
    # epilogue terms alone and together, batches, the drivers' forms, the edges
    assert {"", "a", "b", "B", "m", "abBm"} <= {r.epi for r in T.DENSE}
    assert {r.batch for r in T.DENSE} == {1, 5}
    for fam in ("sgemm v0", "sgemm v1", "cgemm"):
        assert any(r.lay == "tn" and r.epi == "1" and r.inst.startswith(fam) for r in T.DENSE), fam
    assert any(r.lay == "colblk" for r in T.DENSE)
    assert {r.M for r in T.DENSE} >= {1, 63, 64, 65, 127, 128, 129, 196}
    assert {r.N for r in T.DENSE} >= {1, 4, 60, 64, 68, 128, 132, 700}
    assert {r.K for r in T.DENSE} >= {1, 4, 15, 16, 20, 252, 257, 2048}
    assert len(T._COMBINE_ROWS) >= 2 and any(r.batch > 1 for r in T._COMBINE_ROWS) and \
        any(r.epi == "abBm" for r in T._COMBINE_ROWS)
    m = T.dg_mask(196)
    assert m[0] == 0 and m[195] == 0 and m[64] == 0 and m[128] == 0 and m.sum() == 190


# ==== the references =====================================================================================================
def test_gemm_reference_equals_einsum():
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Z, M, N, K = 3, 7, 5, 11
    bias, c0 = rnd(N), rnd(Z, M, N)
    mask = torch.tensor([0.0, 1, 1, 0, 1, 1, 0])
    for ta in (False, True):
        for tb in (False, True):
            a, b = rnd(Z, K, M) if ta else rnd(Z, M, K), rnd(Z, N, K) if tb else rnd(Z, K, N)
            ea, eb = ("zkm" if ta else "zmk"), ("znk" if tb else "zkn")
            prod = torch.einsum("%s,%s->zmn" % (ea, eb), a, b)
            prod_abs = torch.einsum("%s,%s->zmn" % (ea, eb), a.abs(), b.abs())
            r = R.gemm(a, b, ta, tb)
            assert r["c_n"] == K and torch.allclose(r["c"], prod, rtol=0, atol=1e-13)
            assert torch.allclose(r["c_abs"], prod_abs, rtol=0, atol=1e-13)
            c0n = c0.clone()
            c0n[:, mask == 0] = float("nan")
            r = R.gemm(a, b, ta, tb, 2.0, 0.5, c0n, bias, mask)
            want = (2.0 * prod + 0.5 * c0 + bias) * mask.double().view(1, M, 1)
            want_abs = (2.0 * prod_abs + 0.5 * c0.abs() + bias.abs()) * mask.double().view(1, M, 1)
            assert r["c_n"] == K + 2 and torch.allclose(r["c"], want, rtol=0, atol=1e-13)
            assert torch.allclose(r["c_abs"], want_abs, rtol=0, atol=1e-13)
            assert bool((r["c"][:, mask == 0] == 0).all()) and bool((r["c_abs"][:, mask == 0] == 0).all())
            r2 = R.gemm(a[0], b[0], ta, tb, bias=bias)              # 2-d operands: one batch
            assert r2["c_n"] == K + 1 and torch.allclose(r2["c"], prod[0] + bias, rtol=0, atol=1e-13)


def test_skinny_reference_equals_einsum_and_slices_follow_the_host():
    g = torch.Generator().manual_seed(2)
    X, W = torch.randn(3, 2, 77, generator=g, dtype=torch.float64), torch.randn(2, 77, 5, generator=g, dtype=torch.float64)
    full = torch.einsum("rgk,gkn->grn", X, W)
    for form, ks, want in (("f32", 3, [(0, 32), (32, 64), (64, 77)]), ("bf16", 3, [(0, 64), (64, 77), (77, 77)]),
                           ("f32", 1, [(0, 77)]), ("bf16w", 16, [(0, 32), (32, 64), (64, 77)] + [(77, 77)] * 13)):
        sl = R.skinny_slices(77, ks, form)
        assert sl == want
        r = R.skinny(X, W, sl)
        assert r["y"].shape == (ks, 2, 3, 5) and r["y_n"] == [ke - kb for kb, ke in sl] and r["sum_n"] == 77
        assert torch.allclose(r["sum"], full, rtol=0, atol=1e-12)
        assert torch.allclose(r["sum_abs"], torch.einsum("rgk,gkn->grn", X.abs(), W.abs()), rtol=0, atol=1e-12)
        for s, (kb, ke) in enumerate(sl):
            assert torch.allclose(r["y"][s], torch.einsum("rgk,gkn->grn", X[:, :, kb:ke], W[:, kb:ke]), rtol=0, atol=1e-12)
    # skinny_plan (csrc/skinny.hip) at the sizes the comments of the GPU table quote
    assert R.skinny_blocking(33, 16, "f32") == (8, 1, 1, 32) and R.skinny_blocking(40, 2, "f32") == (8, 1, 1, 32)
    assert R.skinny_blocking(260, 1, "f32") == (128, 8, 2, 512) and R.skinny_blocking(1024, 1, "bf16") == (256, 8, 4, 1024)
    assert R.skinny_blocking(132, 1, "f32")[1] == 5 and R.skinny_blocking(132, 1, "bf16")[1] == 6
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.1415926])       # ties to even: down, up
    assert R.bf16_round(x).tolist()[:2] == [1.0, 1.0 + 2.0 ** -6] and R.bf16_round(x.double()).dtype == torch.float64
    assert torch.equal(R.bf16_bits(x).view(torch.bfloat16).float(), R.bf16_round(x))


# ==== the bound is attainable ============================================================================================
_WORST = {}


def _skinny_fp32(r, ks=None):
    """-> (slabs [ks, g, rows, N] evaluated slice by slice in fp32 on the CPU, the fp64 reference, the slices)"""
    X, W = T._skinny_inputs(r)
    Xo, Wo = R.skinny_operands(X, W, r.form)
    ks = ks or skinny_dispatch(r)[1]
    slices = R.skinny_slices(r.K, ks, r.form)
    return R.skinny(Xo, Wo, slices)["y"], R.skinny(Xo.double(), Wo.double(), slices), slices


def _ratio(got, ref, name):
    bound = (ref[name + "_n"] + 8) * U * ref[name + "_abs"].double()
    err = (got.double() - ref[name].double()).abs()
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30).max())


@pytest.mark.parametrize("r", T.SKINNY, ids=SKINNY_IDS)
def test_fp32_cpu_skinny_product_is_inside_the_bound(r):
    Y, ref, slices = _skinny_fp32(r)
    for s, (kb, ke) in enumerate(slices):
        if ke == kb:
            assert bool((Y[s] == 0).all())
        else:
            _sum_ok("cpu fp32 skinny", "y", Y[s], R.slab(ref, s))
            _WORST["skinny slab"] = max(_WORST.get("skinny slab", 0.0), _ratio(Y[s], R.slab(ref, s), "y"))
    total = R.slab_sum_f32(Y)
    _sum_ok("cpu fp32 skinny", "sum", total, ref)
    _WORST["skinny sum"] = max(_WORST.get("skinny sum", 0.0), _ratio(total, ref, "sum"))
    print("worst err/bound of the fp32 CPU evaluation so far: %s" % _WORST)


def _dense_fp32(r):
    a, b, alpha, beta, c0, bias, mask = T.dg_inputs(r)
    got = R.gemm(a, b, bool(r.ta), bool(r.tb), alpha, beta, c0, bias, mask)["c"]
    ref = R.gemm(a.double(), b.double(), bool(r.ta), bool(r.tb), alpha, beta, None if c0 is None else c0.double(),
                 None if bias is None else bias.double(), mask)
    return got, ref, (a, b, alpha, beta, c0, bias, mask)


@pytest.mark.parametrize("r", T.DENSE, ids=DENSE_IDS)
def test_fp32_cpu_dense_product_is_inside_the_bound(r):
    got, ref, _ = _dense_fp32(r)
    assert got.dtype == torch.float32
    _sum_ok("cpu fp32 gemm", "c", got, ref)
    _WORST["dense"] = max(_WORST.get("dense", 0.0), _ratio(got, ref, "c"))
    print("worst err/bound of the fp32 CPU evaluation so far: %s" % _WORST)


# ==== the judge is sensitive =============================================================================================
_FULL = next(r for r in T.DENSE if r.inst == "cgemm mi1 S4 comb vst" and r.epi == "abBm" and not r.opts and r.ws == "full")
_DEEP = next(r for r in T.DENSE if (r.M, r.N, r.K) == (196, 512, 2048) and r.epi == "abBm")


_TILE = next(r for r in T.DENSE if r.inst == "cgemm mi4 S2 comb vst" and r.epi == "abBm")


@pytest.mark.parametrize("r", [_FULL, _TILE, _DEEP], ids=["129x128x512", "196x60x256", "196x512x2048"])
def test_judge_rejects_planted_defects_in_a_dense_product(r):
    """The bound is relative to n * S, so what it can see shrinks with K: at K = 2048 it is ~0.3 absolute here and a lost
    bias of that size passes (which is why the tables put every epilogue term on short products as well); the bias defect
    is planted at K <= 512 only, the others at every depth."""
    got, ref, (a, b, alpha, beta, c0, bias, mask) = _dense_fp32(r)
    _sum_ok("cpu fp32 gemm", "c", got, ref)
    M, N, K = r.M, r.N, r.K
    row = 5
    assert mask[row] != 0
    A = a.transpose(1, 2) if r.ta else a          # [1, M, K]
    Bm = b.transpose(1, 2) if r.tb else b         # [1, K, N]
    # the last k term of one row dropped
    bad = got.clone()
    bad[0, row] -= alpha * A[0, row, K - 1] * Bm[0, K - 1]
    _fails("defect", "c", bad, ref)
    # bias missing on the last column only
    if K <= 512:
        bad = got.clone()
        bad[0, :, N - 1] -= bias[N - 1] * mask
        _fails("defect", "c", bad, ref)
    # one masked row left at beta * c0 (C0 there is finite in this variant)
    bad = got.clone()
    bad[0, 64] = beta * torch.randn(N, generator=torch.Generator().manual_seed(3))
    _fails("defect", "c", bad, ref)
    # one element of the last column tile taken from its neighbour
    bad = got.clone()
    bad[0, row, N - 1] = got[0, row, N - 2]
    _fails("defect", "c", bad, ref)
    # one element off by twice its bound
    bad = got.clone().double()
    bad[0, row, 7] = ref["c"][0, row, 7] + 2.0 * (ref["c_n"] + 8) * U * ref["c_abs"][0, row, 7]
    _fails("defect", "c", bad, ref)


def test_judge_rejects_planted_defects_in_skinny_slabs():
    r = next(r for r in T.SKINNY if (r.form, r.rows, r.N, r.K, r.ks) == ("f32", 32, 512, 4608, 16))
    Y, ref, slices = _skinny_fp32(r)
    for s in range(len(slices)):
        _sum_ok("cpu fp32 skinny", "y", Y[s], R.slab(ref, s))
    # slab s and s + 1 swapped, judged per slab
    _fails("defect", "y", Y[4], R.slab(ref, 3))
    _fails("defect", "y", Y[3], R.slab(ref, 4))
    # the last k of a slice dropped in one row
    X, W = T._skinny_inputs(r)
    kb, ke = slices[2]
    bad = Y[2].clone()
    bad[0, 9] -= X[9, 0, ke - 1] * W[0, ke - 1]
    _fails("defect", "y", bad, R.slab(ref, 2))
    # one element of the last column tile taken from its neighbour
    bad = Y[2].clone()
    bad[0, 9, r.N - 1] = Y[2][0, 9, r.N - 2]
    _fails("defect", "y", bad, R.slab(ref, 2))
    # one element off by twice its bound
    bad = Y[2].clone().double()
    bad[0, 9, 7] = ref["y"][2][0, 9, 7] + 2.0 * (ref["y_n"][2] + 8) * U * ref["y_abs"][2][0, 9, 7]
    _fails("defect", "y", bad, R.slab(ref, 2))
    # an empty slice must be zeros: the GPU test compares with == 0, a non-zero there has no bound to hide under
    r = next(r for r in T.SKINNY if r.K == 33 and r.ks == 16)
    Y, ref, slices = _skinny_fp32(r)
    assert slices[2] == (33, 33) and float(ref["y_abs"][2].max()) == 0.0
    _fails("defect", "y", Y[2] + 1e-30, R.slab(ref, 2))
