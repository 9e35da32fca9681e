"""CPU tests of tests/conv16_refs.py, the yardstick of tests/test_gpu_conv16_kernels.py (no GPU needed):
  1. every index-arithmetic reference matches torch's own fp64 operators (F.conv2d, conv_transpose2d,
     aten.convolution_backward, strided views) to 1e-12 at every case shape;
  2. torch's own CPU fp32 evaluation passes every judge at every case -- the inputs keep the reference alone inside the
     derived bounds -- and its worst err / bound per kind of output goes to the run's parity report;
  3. every planted defect fails;
  4. the case table reaches every training instance of cgemm16_kernel (26), the four creduce16<OBF, STATS> and w9 / w1
     with S = 1 and S > 1 -- asserted against a literal list, the instance of each case being what the library plans for
     the case's own call (test_gpu_conv16_kernels.dispatch: scnattn_plan_next on host windows);
  5. the library's S / kper and wave-split policy against rows worked by hand."""
import pytest
import torch

import conv16_refs as R
import conv_refs as CR
import test_gpu_conv16_kernels as T

_PRODUCTS = {}


def _product_cases():
    """one case per distinct product (op, shape): what reference() caches"""
    if not _PRODUCTS:
        for c in R.CASES:
            _PRODUCTS.setdefault((c.op, c.N, c.Hi, c.Wi, c.Cin, c.Cout, c.s, "t" in c.var), c)
    return list(_PRODUCTS.values())


def test_case_ids_are_unique_and_no_case_is_large():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:
        rows, cols = R.out_shape(c)
        depth = R.rows_out(c) if c.op in ("w9", "w1") else R.gemm_of(c)["K"]
        assert rows * cols * depth <= 200 * 1024 * 256, R.case_id(c)       # multiply-adds: none above 200 x 1024 x 256


def test_references_match_torch_fp64_operators():
    for c in _product_cases():
        I = R.inputs(c)
        ref = R.product(c, I)["out"]
        tor = R.torch_product(c, I, torch.float64)
        assert ref.shape == tor.shape, R.case_id(c)
        assert float((ref - tor).abs().max()) <= 1e-12 * max(float(tor.abs().max()), 1.0), R.case_id(c)


def test_single_tap_index_reference():
    """tap_rows (the source row of scnattn_wgrad16_rows) is the column of conv_refs.fwd_taps, on the odd map and an even one"""
    for (N, H, W, s) in ((3, 7, 5, 2), (2, 4, 6, 2), (2, 3, 5, 1)):
        taps = CR.fwd_taps(N, H, W, s)
        for t in range(9):
            assert torch.equal(R.tap_rows(N, H, W, s, t // 3 - 1, t % 3 - 1), taps[:, t])
        assert torch.equal(R.tap_rows(N, H, W, s, 0, 0), CR.gather_rows(N, H, W, s))


def test_planted_mask_edges_are_bf16_and_hit_the_edges():
    n = 0
    for c in R.CASES:
        if c.epi != 2 or c.Cin < 8:
            continue
        I = R.inputs(c)
        assert I["z"].dtype == torch.bfloat16 and R.is_bf16(I["mean"][:4])
        on, xhat = CR.bn_mask(I["z"].float(), I["mean"], I["invstd"], I["gamma"], I["beta"], False)
        z, m = I["z"].float(), I["mean"]
        assert bool((z[0, :4] == m[:4]).all()) and not bool(on[0, :4].any()), "an expression that is exactly 0 must be masked"
        if z.shape[0] > 2:
            assert bool((z[1, :4] > m[:4]).all()) and bool((z[2, :4] < m[:4]).all())
            assert bool((on[1, :4] == (I["gamma"][:4] > 0)).all()) and bool((on[2, :4] == (I["gamma"][:4] < 0)).all())
            n += 1
    assert n >= 10


def test_torch_cpu_fp32_evaluation_passes_every_judge():
    worst = {}
    for c in R.CASES:
        I = R.inputs(c)
        ok, ratios, fails = R.judge(c, I, R.cpu_eval(c, I))
        assert ok, "%s: %s" % (R.case_id(c), "; ".join(fails))
        for k, v in ratios.items():
            key = ("bf16 " if c.obf else "fp32 ") + ("weight gradient" if c.op in ("w9", "w1") else k)
            worst[key] = max(worst.get(key, 0.0), v)
    for w in R.cv_masters():
        assert R.cv_judge(w, R.cv_eval(w))
    lines = ["%-24s %.3f" % (k, v) for k, v in sorted(worst.items())]
    print("\n".join(lines))
    from test_gpu_parity import _report
    _report(lines, "bf16 convolution kernels: torch's CPU fp32 evaluation against the same judges, worst err/bound over %d cases"
            % len(R.CASES))
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_fails(defect):
    hit = [c for c in R.CASES if R.applies(defect, c)]
    assert len(hit) >= 2, "%s applies to %d cases only" % (defect, len(hit))
    step = max(1, len(hit) // 24)
    for c in hit[::step]:
        I = R.inputs(c)
        ok, ratios, _ = R.judge(c, I, R.cpu_eval(c, I, defect))
        assert not ok, "%s slipped through at %s (%s)" % (defect, R.case_id(c), ratios)
    if defect == "pad_row_stats":       # the shape the defect is named for: M = 65 with a non-zero shift
        assert any(R.out_shape(c)[0] == 65 and float(R.inputs(c)["shift"].abs().min()) > 0 for c in hit)


@pytest.mark.parametrize("defect", ("truncate", "wt_swap"))
def test_planted_defect_of_the_weight_copies_fails(defect):
    bad = [not R.cv_judge(w, R.cv_eval(w, defect)) for w in R.cv_masters()]
    if defect == "wt_swap":             # taps and cout swapped is the same layout with one tap
        assert bad == [taps > 1 for (_, taps, _) in R.CV_WEIGHTS]
    else:
        assert all(bad)


def test_weight_masters_hold_the_rounding_edges():
    for w in R.cv_masters():
        (a, at), (b2, bt) = R.cv_expected(w)        # torch's two routes agree on every number: they may differ at a NaN only
        assert bool(((a == b2) | w.isnan()).all()) and bool(((at == bt) | w.permute(2, 1, 0).isnan()).all())
        b = w.to(torch.bfloat16).float()
        assert bool(((w == 1 + 2.0 ** -8) & (b == 1)).any()) and bool(((w == 1 + 3 * 2.0 ** -8) & (b == 1 + 2.0 ** -6)).any())
        assert bool((w.isfinite() & b.isinf()).any()) and bool(w.isnan().any())
        assert bool(((w != 0) & (w.abs() < 2.0 ** -126)).any()) and bool(((w == 0) & torch.signbit(w)).any())


TRAINING_INSTANCES = [
    "cgemm16<MI 1, EPI 0, plain, bf16, C3 0>", "cgemm16<MI 1, EPI 0, plain, fp32, C3 0>",
    "cgemm16<MI 1, EPI 1, plain, bf16, C3 0>", "cgemm16<MI 1, EPI 1, plain, fp32, C3 0>",
    "cgemm16<MI 1, EPI 2, plain, bf16, C3 0>",
    "cgemm16<MI 1, EPI 0, gather, bf16, C3 0>", "cgemm16<MI 1, EPI 0, gather, fp32, C3 0>",
    "cgemm16<MI 1, EPI 1, gather, bf16, C3 0>", "cgemm16<MI 1, EPI 1, gather, fp32, C3 0>",
    "cgemm16<MI 1, EPI 0, plain, bf16, C3 1>", "cgemm16<MI 1, EPI 1, plain, bf16, C3 1>", "cgemm16<MI 1, EPI 2, plain, bf16, C3 1>",
    "cgemm16<MI 1, EPI 0, plain, bf16, C3 4>",
    "cgemm16<MI 2, EPI 0, plain, bf16, C3 0>", "cgemm16<MI 2, EPI 0, plain, fp32, C3 0>",
    "cgemm16<MI 2, EPI 1, plain, bf16, C3 0>", "cgemm16<MI 2, EPI 1, plain, fp32, C3 0>",
    "cgemm16<MI 2, EPI 2, plain, bf16, C3 0>",
    "cgemm16<MI 2, EPI 0, gather, bf16, C3 0>", "cgemm16<MI 2, EPI 0, gather, fp32, C3 0>",
    "cgemm16<MI 2, EPI 1, gather, bf16, C3 0>", "cgemm16<MI 2, EPI 1, gather, fp32, C3 0>",
    "cgemm16<MI 2, EPI 0, plain, bf16, C3 1>", "cgemm16<MI 2, EPI 1, plain, bf16, C3 1>", "cgemm16<MI 2, EPI 2, plain, bf16, C3 1>",
    "cgemm16<MI 2, EPI 0, plain, bf16, C3 4>",
]
REDUCERS = ["creduce16<bf16, plain>", "creduce16<bf16, stats>", "creduce16<fp32, plain>", "creduce16<fp32, stats>"]
WGRADS = ["wgrad16_w9 (S = 1)", "wgrad16_w9 (S > 1)", "wgrad16_w1 (S = 1)", "wgrad16_w1 (S > 1)"]


def test_case_table_reaches_every_training_instance():
    assert len(TRAINING_INSTANCES) == 26 and len(set(TRAINING_INSTANCES)) == 26
    m = [(c, T.dispatch(c)) for c in R.CASES]
    reached = {n for _, d in m for n in d["names"]}
    assert reached == set(TRAINING_INSTANCES + REDUCERS + WGRADS), sorted(reached ^ set(TRAINING_INSTANCES + REDUCERS + WGRADS))
    gem = [(c, d) for c, d in m if c.op not in ("w9", "w1")]
    # the splits the table promises: forced 2 at K = 40 and K = 72, forced 2 / 4 at K = 1024, one the policy chose; a split
    # 3x3 and a split gather; beta = 1 through each plain reducer; both statistics reducers with and without a shift
    for K, S in ((40, 2), (72, 2), (1024, 2), (1024, 4)):
        assert any(c.split == S and d["S"] == S and R.gemm_of(c)["K"] == K for c, d in gem), (K, S)
    assert any(c.split == 0 and d["S"] > 1 for c, d in gem)
    assert any(d["S"] > 1 and d["inst"][4] == 1 for c, d in gem) and any(d["S"] > 1 and d["inst"][2] for c, d in gem)
    for obf in (True, False):
        assert any(d["reduce"] == (obf, False) and "b" in c.var for c, d in gem)
        for var in ("", "s"):
            assert any(d["reduce"] == (obf, True) and c.var == var for c, d in gem)
    for c, d in gem:
        p = R.gemm_of(c)
        assert d["kper"] % 32 == 0 and (d["S"] - 1) * d["kper"] < p["K"] <= d["S"] * d["kper"], R.case_id(c)
        assert d["S"] * p["M"] * p["N"] <= R.WS_FLOATS
        assert d["S"] == 1 or (c.epi != 2 and p["c3"] != 4)
    # the stride-2 d input leaves no class out: every class has rows at every map
    assert all(c.Hi % 2 == 0 and c.Wi % 2 == 0 for c in R.CASES if c.op == "s3")


def _plan_of(c, wsf=R.WS_FLOATS):
    """the library's plan for a case outside the table, as conv16_refs.names renders it"""
    return R.names(T._run(c, R.inputs(c), T.CPU, torch.empty(R.WS_FLOATS + 64), wsf=wsf))


def test_policy_mirror_against_hand_worked_rows():
    def mc(M, N, K, c3=0, epi=0, obf=True, force_mi=0, force_split=0, ws_floats=R.WS_FLOATS):
        """the plan of the M x N x K product: scnattn_cgemm16 (1x1 forward; the mask epilogue as a 1x1 d input), or with
        c3 = 4 scnattn_conv3x3_dgrad16 at stride 2 on M maps of 2 x 2 (K = 9 * Cout)"""
        if c3 == 4:
            c = R.case("s3", M, 2, 2, N, K // 9, s=2, mi=force_mi, split=force_split)
        elif epi == 2:
            c = R.case("d1", M, 1, 1, N, K, epi=2, mi=force_mi, split=force_split)
        else:
            c = R.case("f1", M, 1, 1, K, N, epi=epi, mi=force_mi, split=force_split, obf=int(obf))
        assert (R.gemm_of(c)["M"], R.gemm_of(c)["N"], R.gemm_of(c)["K"], R.gemm_of(c)["c3"]) == (M, N, K, c3)
        return _plan_of(c, ws_floats)

    # K = 40 forced to 2 slabs: ceil(20 / 32) * 32 = 32 per slab, the second one 8 deep
    d = mc(65, 72, 40, force_split=2)
    assert (d["S"], d["kper"], 40 - d["kper"]) == (2, 32, 8)
    # K = 72 forced to 2: ceil(36 / 32) * 32 = 64, slabs of 64 and 8
    d = mc(65, 72, 72, force_split=2)
    assert (d["S"], d["kper"]) == (2, 64)
    # K = 72 forced to 3: 24 -> 32 per slab -> 3 slabs (32, 32, 8);  K = 64 forced to 4: 16 -> 32 -> only 2 slabs survive
    assert (mc(65, 72, 72, force_split=3)["S"], mc(65, 72, 64, force_split=4)["S"]) == (3, 2)
    # policy: 200 x 256 x 1024, M > 64 and 2 x 2 128-row tiles -> mi 1, 4 x 2 = 8 tiles, ceil(512 / 8) = 64 -> K / 256 = 4
    d = mc(200, 256, 1024)
    assert (d["mi"], d["tiles"], d["S"], d["kper"], d["reduce"]) == (1, 8, 4, 256, (True, False))
    # the same without a workspace, and below K = 512: one launch
    assert mc(200, 256, 1024, ws_floats=0)["S"] == 1 and mc(200, 256, 480)["S"] == 1
    # M = 64 keeps the 128-row tile (M > 64 fails); force_mi wins
    assert mc(64, 72, 64)["mi"] == 2 and mc(64, 72, 64, force_mi=1)["mi"] == 1 and mc(65, 72, 64)["mi"] == 1
    # the mask epilogue is never split, forced or not; the statistics of a split product move to the reducer
    d = mc(200, 256, 1024, epi=2, force_split=4)
    assert (d["S"], d["inst"][1], d["reduce"]) == (1, 2, None)
    d = mc(200, 256, 1024, epi=1, obf=False, force_split=2)
    assert (d["S"], d["kper"], d["inst"][1], d["reduce"]) == (2, 512, 0, (False, True))
    # the stride-2 d input: four classes per tile in the row-tile choice, never split, EPI 0
    d = mc(24, 72, 576, c3=4, force_split=4)
    assert (d["mi"], d["S"], d["inst"]) == (2, 1, (2, 0, False, True, 4))
    assert mc(65, 72, 576, c3=4)["mi"] == 1
    # a forced split the workspace cannot hold is refused
    with pytest.raises(RuntimeError, match="cgemm16: forced split does not fit"):
        mc(64, 64, 64, force_split=2, ws_floats=16)

    # ---- wgrad_split: aim 512 workgroups over ntiles blocks, at least 16 of the Q lines per slab, what the workspace holds.
    # One 32 x 32 block (ntiles = 1, a slab of 32 * 9 * 32 = 9216 floats) is scnattn_wgrad16_3x3 on a 1 x Q x 16 map; many
    # blocks are scnattn_wgrad16_rows on 16 * Q rows with Cin = 640 (10 blocks wide) and Cout = 64 * ntiles / 10 ----
    def ws(ntiles, Q, ws_floats=R.WS_FLOATS, force=0):
        if ntiles == 1:
            c = R.case("w9", 1, Q, 16, 32, 32, split=force, obf=0)
        else:
            c = R.case("w1", 16 * Q, 1, 1, 640, 64 * (ntiles // 10), split=force, obf=0)
        d = _plan_of(c, ws_floats)
        assert (d["ntiles"], d["Q"]) == (ntiles, Q)
        return d["S"]

    assert ws(1, 36) == 2                                           # aim 512, at least 16 lines per slab: 36 // 16 = 2
    assert ws(1, 31) == 1                                           # fewer than 32 lines: no split
    assert ws(1, 64, force=3) == 3
    with pytest.raises(RuntimeError, match="wgrad16_3x3: forced split does not fit"):
        ws(1, 36, force=3)                                          # a force clamped to 2: the entry point refuses it
    assert ws(1, 64, 0) == 1 and ws(1, 64, 2 * 9216) == 2           # what the workspace holds
    assert ws(600, 64) == 1                                         # (512 + 300) // 600 = 1
    assert ws(400, 64) == 1 and ws(300, 64) == 2                    # 712 // 400, 662 // 300 (two slabs of 1920 x 640 fit)
    # Q and ntiles as the two host functions form them
    d = _plan_of(R.case("w9", 2, 9, 20, 64, 96, obf=0))       # 2 segments of 16 per line: Q = 2 * 2 * 9, 3 x 2 blocks
    assert (d["Q"], d["ntiles"], d["S"]) == (36, 6, 2)
    d = _plan_of(R.case("w9", 1, 1, 3, 32, 32, obf=0))        # one line: three waves of the workgroup have none
    assert (d["Q"], d["S"]) == (1, 1)
    d = _plan_of(R.case("w1", 500, 1, 1, 128, 64, split=2, obf=0))    # 32 lines of 16 rows, the last one 4 deep
    assert (d["Q"], d["ntiles"], d["S"]) == (32, 2, 2)
    with pytest.raises(RuntimeError, match="wgrad16_rows: forced split does not fit"):
        _plan_of(R.case("w1", 257, 1, 1, 64, 64, split=2, obf=0))     # 17 lines: the clamp reduces a forced 2
