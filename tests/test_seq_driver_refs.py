"""The driver tier without a GPU (tests/seq_driver_refs.py): the row judge's precondition for every case of the GPU table,
its sensitivity -- shown on perturbed copies of the CPU-fp32 results, which is what the whole-tensor `rel_err` of the older
driver tests lets through --, and the oracle's own reading of the exact invariants the GPU tests pin on the drivers."""
import pytest
import torch

import seq_driver_refs as S
from helpers import rel_err


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_row_yardstick_precondition(cid):
    """rho <= tol / 4 for every result of every case, from the references alone; CPU fp32 itself passes the judge"""
    c = S.case(cid)
    worst = {}
    for name, ref64 in c.ref64.items():
        if name == S.ZERO_BIAS:
            assert float(ref64.abs().max()) < 1e-12 and float(c.ref32[name].abs().max()) < S.ZERO_BIAS_TOL / 4
            continue
        rho, dead = S.row_precondition(name, ref64, c.ref32[name], S.tol_of(name))
        rows = S._rows(ref64).shape[0]
        print("%-28s %-38s rho %.3e   rows %5d, not live %5d" % (cid, name, rho, rows, dead))
        worst[name] = rho
        S.row_ok("cpu-fp32", name, c.ref32[name], ref64, c.ref32[name], S.tol_of(name))
    assert max(v for k, v in worst.items() if k in ("preds", "alphas")) <= S.TOL_OUT / 4
    # the exact zeros the GPU test asks for are zeros of the oracle too
    dead = ~c.live
    assert float(c.ref64["preds"][dead].abs().max() if dead.any() else 0.0) == 0.0
    if c.has_att:
        assert float(c.ref64["alphas"][dead].abs().max() if dead.any() else 0.0) == 0.0
    assert float(c.ref64["g.embedding.weight"][~S.tokens_present(c)].abs().max()) == 0.0


def _rejects(name, got, c):
    with pytest.raises(AssertionError, match="worst err/bound"):
        S.row_ok("perturbed", name, got, c.ref64[name], c.ref32[name], S.tol_of(name))


def test_judge_rejects_a_scaled_small_row_that_rel_err_accepts():
    """A unit whose full_att weight is 3e-4 of the others' has a d decoder_att.weight row that small (d att2[a] carries the
    factor full_att.weight[a]) and as well conditioned as any other: with random weights a row that small is mostly
    cancellation noise, which the precondition refuses (seq_driver_refs.CASES)."""
    c0 = S.case("att-m4-B6-ragged")
    sd = {k: v.clone() for k, v in c0.sd.items()}
    sd["attention.full_att.weight"][0, 5] *= 3e-4
    c = c0.variant(sd=sd)
    c.ref64, c.ref32 = S.oracle(c, torch.float64), S.oracle(c, torch.float32)
    name = "g.attention.decoder_att.weight"
    S.row_precondition(name, c.ref64[name], c.ref32[name], S.TOL_GRAD)
    want, got = c.ref64[name], c.ref32[name].clone()
    rmax = want.abs().amax(dim=1)
    live = rmax >= S.LIVE * want.abs().max()
    r = int(torch.where(live, rmax, torch.full_like(rmax, float("inf"))).argmin())
    print("smallest live row %d: row max / tensor max %.3e" % (r, float(rmax[r] / want.abs().max())))
    assert r == 5
    got[r] *= 1.5
    assert rel_err(got, want) <= 2e-4, "the planted row is not small enough to pass the tensor-level bar"
    _rejects(name, got, c)


def test_judge_rejects_a_dropped_last_step():
    """the last step of the shortest caption left out of g.fc.bias and g.decode_step.bias_ih"""
    c = S.case("att-m4-B6-ragged")
    b, t = c.B - 1, c.dl[-1] - 1
    assert c.dl[-1] == min(c.dl)
    got = c.ref32["g.fc.bias"].clone() - c.dpreds[b, t]           # d fc.bias = sum of dpreds over decoded cells
    _rejects("g.fc.bias", got, c)
    # d bias_ih = sum over decoded cells of d r: the contribution of one cell is the difference to the problem without it
    short = c.variant(dpreds=c.dpreds.clone(), dalphas=c.dalphas.clone())
    short.dpreds[b, t] = 0
    short.dalphas[b, t] = 0
    assert t == 0 and c.dl[-1] == 1       # the only step of that caption: zero upstream removes its whole contribution
    got = S.oracle(short, torch.float32)["g.decode_step.bias_ih"]
    _rejects("g.decode_step.bias_ih", got, c)


def test_judge_rejects_a_shifted_alphas_row():
    c = S.case("att-m4-B6-ragged")
    got = c.ref32["alphas"].clone()
    got[2, 3] = got[2, 3].roll(1)
    _rejects("alphas", got, c)


def test_judge_rejects_one_element_of_a_small_row_that_rel_err_accepts():
    c = S.case("att-m4-B6-ragged")
    name = "g.attention.encoder_att.weight"
    want, got = c.ref64[name], c.ref32[name].clone()
    rmax, tmax = want.abs().amax(dim=1), float(want.abs().max())
    live = rmax >= S.LIVE * tmax
    r = int(torch.where(live, rmax, torch.full_like(rmax, float("inf"))).argmin())
    print("small row %d: row max / tensor max %.3e" % (r, float(rmax[r]) / tmax))
    got[r, 5] += 1e-4 * tmax
    assert rel_err(got, want) <= 2e-4
    _rejects(name, got, c)


def test_judge_rejects_a_nan_and_a_nonzero_in_a_zero_row():
    c = S.case("scn-m4-B6-ragged-k3")
    got = c.ref32["preds"].clone()
    got[0, 0, 0] = float("nan")
    _rejects("preds", got, c)
    got = c.ref32["preds"].clone()
    got[c.B - 1, c.T - 1, 3] = 1e-3       # a dead cell: its row is all zeros in the oracle
    _rejects("preds", got, c)


# ---- the oracle has the invariants the GPU tests pin on the drivers (tests/test_gpu_seq_driver.py, section c) --------------
def _close(a, b, what):
    for k in a:
        err = float((a[k] - b[k]).abs().max()) if a[k].numel() else 0.0
        assert err <= 1e-12, "%s: %s moves by %.3e" % (what, k, err)


@pytest.mark.parametrize("cid", ["att-m4-pool-B6-ragged-k3", "scn-m4-B6-ragged-k3"])
def test_oracle_has_the_invariants(cid):
    c = S.case(cid)
    base = S.oracle(c, torch.float64)
    g = torch.Generator().manual_seed(7)
    others = lambda r, b: {k: v[torch.arange(c.B) != b] for k, v in r.items() if k in ("preds", "alphas")}      # noqa: E731
    # 1. row isolation
    b = 1
    enc, tags, caps = c.enc.clone(), c.tags.clone(), c.caps.clone()
    enc[b], tags[b], caps[b] = torch.rand(enc[b].shape, generator=g), torch.rand(tags[b].shape, generator=g), \
        torch.randint(1, c.V - 3, caps[b].shape, generator=g)
    moved = S.oracle(c.variant(enc=enc, tags=tags, caps=caps), torch.float64)
    _close(others(base, b), others(moved, b), "row isolation")
    assert float((moved["preds"][b] - base["preds"][b]).abs().max()) > 1e-3
    # 2. causality
    t = 3
    caps = c.caps.clone()
    caps[0, t] = (caps[0, t] % (c.V - 4)) + 1
    assert caps[0, t] != c.caps[0, t]
    moved = S.oracle(c.variant(caps=caps), torch.float64)
    _close({k: v[0, :t] for k, v in base.items() if k in ("preds", "alphas")},
           {k: v[0, :t] for k, v in moved.items() if k in ("preds", "alphas")}, "causality")
    assert float((moved["preds"][0, t] - base["preds"][0, t]).abs().max()) > 1e-4
    # 3. padding tokens, 4. dead upstream cells
    caps, dpreds = c.caps.clone(), c.dpreds.clone()
    pad = torch.ones(c.B, c.L, dtype=torch.bool)
    pad[:, :c.T] = ~c.live
    caps[pad] = torch.randint(1, c.V - 3, (int(pad.sum()),), generator=g)
    dpreds[~c.live] = 1e3
    kw = {"dalphas": torch.where(c.live.unsqueeze(2), c.dalphas, torch.full_like(c.dalphas, -1e3))} if c.has_att else {}
    _close(base, S.oracle(c.variant(caps=caps, dpreds=dpreds, **kw), torch.float64), "padding / dead cells")
    # 5. zero upstream for one image
    for b in (0, c.B - 1):
        dpreds = c.dpreds.clone()
        dpreds[b] = 0
        kw = {}
        if c.has_att:
            kw["dalphas"] = c.dalphas.clone()
            kw["dalphas"][b] = 0
        r1 = S.oracle(c.variant(dpreds=dpreds, **kw), torch.float64)
        assert float(r1["denc"][b].abs().max()) == 0.0 and float(r1["dtags"][b].abs().max()) == 0.0
        enc, tags = c.enc.clone(), c.tags.clone()
        enc[b], tags[b] = torch.rand(enc[b].shape, generator=g), torch.rand(tags[b].shape, generator=g)
        r2 = S.oracle(c.variant(enc=enc, tags=tags, dpreds=dpreds, **kw), torch.float64)
        _close({k: v for k, v in r1.items() if k not in ("preds", "alphas")},
               {k: v for k, v in r2.items() if k not in ("preds", "alphas")}, "zero upstream")


def test_saved_layout_is_dense_and_aligned():
    for cid in S.CASE_IDS:
        c = S.case(cid)
        layout, total = S.saved_layout(c)
        assert all(off % 64 == 0 for _, off, _, _ in layout) and total % 64 == 0
        assert [off for _, off, _, _ in layout] == sorted(off for _, off, _, _ in layout)


@pytest.mark.parametrize("kind", S.MODULE_KINDS)
def test_row_yardstick_precondition_of_the_module_cases(kind):
    _, _, _, ref64, ref32 = S.module_case(kind)
    for name in ref64:
        if name != S.ZERO_BIAS:
            rho, dead = S.row_precondition(name, ref64[name], ref32[name], S.tol_of(name))
            print("%-16s %-38s rho %.3e   not live %d" % (kind, name, rho, dead))
