"""Scheduled sampling on the GPU, from the driver up (csrc/beam_search.cpp: scnattn_rollout_*_ss, scnattn.functional.mix_run,
the decoders' mix_batch) against the CPU reference of tests/scheduled_refs.py in fp64, against the rollout's and the scoring
driver's own words, and for what it writes.

A mixed run is a chain of discrete choices at its REPLACED positions, so the rule of tests/test_gpu_rollout.py applies per
row, with only those positions entering it (rollout_refs.decidable_rows on scheduled_refs.mix_rollout): rows that do not
count are left out under the same asserted caps, at most 1/4 of all rows of the table and at most 1/2 of any fixture's; the
decision comes from the CPU reference alone, which leaves out 0 of the 90 rows (tests/test_scheduled_refs.py shows the same
without a GPU).  Bars (those of the rollout tests): words, coins and samples equal, logp and sum_logp within
1e-4 * max(1, |x|), alphas within 1e-4 of the row's largest.  The cases: tests/scheduled_refs.py (MIXES, gold_of)."""
import pytest
import torch

import beam_refs as BR
import scheduled_refs as SS
from helpers import t

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
GUARD = 0x7FC5A5A5
TEMPERATURE = 1.0 / SS.INV_TEMP          # 1 / (1 / x) rounds back to the fp32 number x


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def near(got, want):
    return abs(got - want) <= TOL_OUT * max(1.0, abs(want))


def _bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def _model(kind, d, dev):
    from test_gpu_parity import _build_decoder
    return _build_decoder(kind, d, dev).eval()


def _device(m, kind, case, dev, prob=None, draw=SS.DRAW, **kw):
    """SF.mix_run on the case's gold words -> (results, steps)"""
    from models.decoders import _common
    from scnattn import functional as SF
    wm, enc, tags = case["wm"], case["enc"], case["tags"]
    gold = torch.zeros(case["gold"].shape[0], SF.BEAM_MAX_STEPS, dtype=torch.int32)
    gold[:, :case["gold"].shape[1]] = case["gold"]
    with torch.no_grad():
        dims, weights, e, tg = _common._search_operands(m, len(wm), enc.to(dev), None if tags is None else tags.to(dev),
                                                        kind != "pure_scn", kind != "pure_attention")
        return SF.mix_run(dims, case["K"], weights, e, tg, wm["<start>"], gold.to(dev), case["nmix"].to(torch.int32).to(dev),
                          case["prob"] if prob is None else prob, SS.SEED, draw, inv_temp=SS.INV_TEMP, greedy=case["greedy"],
                          **kw)


def _batch(m, case, dev, prob=None, **kw):
    """decoder.mix_batch on the case as captions -> (result, caps, caplens) on the device"""
    caps, caplens = SS.as_caps(case["wm"], case["gold"], case["nmix"])
    caps, caplens = caps.to(dev), caplens.to(dev)
    tags = None if case["tags"] is None else case["tags"].to(dev)
    args = dict(per_image=case["K"], seed=SS.SEED, draw=SS.DRAW, temperature=TEMPERATURE, greedy=case["greedy"])
    args.update(kw)
    with torch.no_grad():
        out = m.mix_batch(case["wm"], case["enc"].to(dev), tags, caps, caplens, case["prob"] if prob is None else prob, **args)
    return out, caps, caplens


# ---- (1) against the fp64 reference ---------------------------------------------------------------------------------------
_LEFT = {}


@pytest.mark.parametrize("mix", SS.MIXES, ids=lambda x: "K%d-p%g-%s" % (x[0], x[1], "greedy" if x[2] else "sampled"))
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_fixture_mix_vs_reference(dev, name, kind, mix):
    case = SS.driver_case(name, kind, mix)
    ref, ok, nmix, gold, wm = case["ref"], case["ok"], case["nmix"].tolist(), case["gold"], case["wm"]
    m = _model(kind, case["d"], dev)
    res, steps = _device(m, kind, case, dev, want_alpha=True)
    use_att = kind != "pure_scn"
    tok, rep, smp, lp = (res[k].cpu() for k in ("tokens", "replaced", "sample", "logp"))
    slp = res["sum_logp"].cpu().tolist()
    alpha = res["alpha"].cpu() if res["alpha"] is not None else None
    assert use_att == (alpha is not None)
    assert steps == max(nmix) == ref["steps"] and tuple(tok.shape) == (len(nmix), steps)
    assert res["nmix"].cpu().tolist() == nmix and torch.equal(res["gold"].cpu(), gold[:, :steps].to(torch.int32))
    assert int(res["open_rows"]) == 0 and not bool(res["nopen"].any()) and not bool(res["nsrc"].any())
    out, caps, caplens = _batch(m, case, dev)
    inputs, replaced = out["inputs"].cpu(), out["replaced"].cpu()
    assert inputs.dtype == torch.int64 and replaced.dtype == torch.bool and out["sample"].dtype == torch.int32
    assert out["n_replaced"].dtype == torch.int32 and tuple(inputs.shape) == tuple(caps.shape) == tuple(replaced.shape)
    # the coin is exact on EVERY row, decidable or not: it does not depend on the model
    left = 0
    for r, n in enumerate(nmix):
        assert rep[r, :n].tolist() == [int(x) for x in ref["replaced"][r]], r
        for rec in (tok, rep, lp):                                          # the records behind the row
            assert not bool(_bits(rec[r, n:]).any()), r
        assert bool(((smp[r, n:] == -1) | (smp[r, n:] == 0)).all()), r      # -1 while the image is open, then the zero-fill
        assert bool((out["sample"][r, n:] == -1).all()), r
        assert replaced[r, 1:1 + n].tolist() == ref["replaced"][r] and not bool(replaced[r, 1 + n:].any()) and not replaced[r, 0]
        assert int(out["n_replaced"][r]) == sum(ref["replaced"][r])
        kept = ~replaced[r]
        assert torch.equal(inputs[r][kept], caps[r].cpu()[kept]), r           # <start>, the kept gold words, the tail
        if not ok[r]:
            left += 1
            continue
        assert tok[r, :n].tolist() == ref["tokens"][r] and smp[r, :n].tolist() == ref["sample"][r], r
        assert inputs[r, 1:1 + n].tolist() == ref["tokens"][r] and out["sample"][r, :n].cpu().tolist() == ref["sample"][r], r
        assert near(slp[r], ref["sum_logp"][r]) and near(float(out["sum_logp"][r]), ref["sum_logp"][r]), r
        for s in range(n):
            assert near(float(lp[r, s]), ref["logp"][r][s]), (r, s, float(lp[r, s]), ref["logp"][r][s])
            if not ref["replaced"][r][s]:
                assert int(_bits(lp)[r, s]) == 0
            if use_att:
                a, b = alpha[s, r].double(), ref["alpha"][s][r].double()
                assert float((a - b).abs().max()) <= TOL_OUT * float(b.abs().max()), (r, s)
    # mix_batch is mix_run in the caller's form: the same bits
    assert torch.equal(_bits(out["logp"][:, :steps]), _bits(res["logp"])) and torch.equal(out["sum_logp"], res["sum_logp"])
    n_rep = int(rep.sum())
    print("%s %s: %d of %d rows left out; %d positions replaced of %d" % (name, mix, left, len(ok), n_rep, sum(nmix)))
    assert 2 * left <= len(ok)
    _LEFT[(name, mix)] = (left, len(ok))
    if len(_LEFT) == len(SS.MIXES) * len(BR.FIXTURES):
        rows, gone = sum(n for _, n in _LEFT.values()), sum(o for o, _ in _LEFT.values())
        assert 4 * gone <= rows, _LEFT


# ---- (2) the two ends -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_prob_zero_returns_the_captions(dev, name, kind):
    case = SS.driver_case(name, kind, SS.MIXES[1])
    m = _model(kind, case["d"], dev)
    out, caps, caplens = _batch(m, case, dev, prob=0.0)
    assert torch.equal(out["inputs"], caps) and not bool(out["replaced"].any()) and not bool(out["n_replaced"].any())
    assert bool((out["sample"] == -1).all()) and not bool(_bits(out["logp"]).any()) and not bool(_bits(out["sum_logp"]).any())


@pytest.mark.parametrize("K", (1, 2))
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_prob_one_is_the_rollout_until_it_ends(dev, name, kind, K):
    """device against device, exact: the same (seed, draw) is the same noise, so the words are rollout_batch's up to its
    first <end> or nmix, whichever comes first"""
    case = dict(SS.driver_case(name, kind, SS.MIXES[0 if K == 1 else 1]), greedy=False)
    m = _model(kind, case["d"], dev)
    out, caps, caplens = _batch(m, case, dev, prob=1.0)
    tags = None if case["tags"] is None else case["tags"].to(dev)
    with torch.no_grad():
        rcaps, rlens, _ = m.rollout_batch(case["wm"], case["enc"].to(dev), tags, samples=K, seed=SS.SEED, draw=SS.DRAW,
                                          temperature=TEMPERATURE)
    inputs, rcaps, rlens = out["inputs"].cpu(), rcaps.cpu(), rlens.view(-1).tolist()
    compared = 0
    for r, n in enumerate(case["nmix"].tolist()):
        k = min(n, rlens[r] - 1)
        assert inputs[r, 1:1 + k].tolist() == rcaps[r, 1:1 + k].tolist(), (r, k)
        assert int(out["n_replaced"][r]) == n and bool(out["replaced"][r, 1:1 + n].all())
        compared += k
    print("%s K=%d: %d words compared" % (name, K, compared))
    assert compared >= 10 * K


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_greedy_samples_are_the_scoring_drivers_best_words(dev, name, kind):
    """device against device, exact: at every replaced position the input is the arg-max after the mixed inputs before it,
    which is what score_batch reports as `best` when it is given those inputs"""
    case = SS.driver_case(name, kind, SS.MIXES[2])
    assert case["greedy"] and case["prob"] == 0.5
    m = _model(kind, case["d"], dev)
    out, caps, caplens = _batch(m, case, dev)
    tags = None if case["tags"] is None else case["tags"].to(dev)
    with torch.no_grad():
        sc = m.score_batch(case["wm"], case["enc"].to(dev), tags, out["inputs"], caplens, per_image=case["K"],
                           temperature=TEMPERATURE)
    rep = out["replaced"][:, 1:]
    assert int(rep.sum()) >= 20
    assert torch.equal(out["inputs"][:, 1:][rep], sc["best"].to(torch.int64)[rep])
    assert torch.equal(out["sample"][rep], sc["best"][rep])
    # and its log-probability is the score of that word: two kernels, two summation orders
    a, b = out["logp"][rep].double(), sc["logp"][rep].double()
    assert bool(((a - b).abs() <= TOL_OUT * b.abs().clamp_min(1.0)).all())


# ---- (3) driver mechanics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [BR.FIXTURES[0], BR.FIXTURES[2]])
def test_chunks_guard_band_repeats_and_the_next_draw(dev, name, kind):
    case = SS.driver_case(name, kind, SS.MIXES[1])
    m = _model(kind, case["d"], dev)
    keys = ("tokens", "replaced", "sample", "logp", "sum_logp", "nmix", "gold", "alpha")
    for want_alpha in (False, True):
        a, steps = _device(m, kind, case, dev, want_alpha=want_alpha, guard=4096)
        a = {k: None if a[k] is None else a[k].clone() for k in keys + ("guard",)}
        assert bool((a["guard"] == GUARD).all()), "words behind the workspace were overwritten"
        assert (a["alpha"] is not None) == (want_alpha and kind != "pure_scn")
        for chunk in (1, 7, None):              # other chunkings, and the same call again: equal bits
            kw = {} if chunk is None else {"chunk": chunk}
            b, steps_b = _device(m, kind, case, dev, want_alpha=want_alpha, guard=4096, **kw)
            assert steps_b == steps and bool((b["guard"] == GUARD).all())
            for k in keys:
                assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), (want_alpha, chunk, k)
    c, _ = _device(m, kind, case, dev, draw=SS.DRAW + 1)
    assert not torch.equal(c["replaced"], a["replaced"])
    d, _ = _device(m, kind, case, dev, prob=0.5)                # a coin that fell below 0.25 falls below 0.5
    assert bool((d["replaced"] >= a["replaced"]).all()) and int(d["replaced"].sum()) > int(a["replaced"].sum())


@pytest.mark.parametrize("name,kind", [BR.FIXTURES[1], BR.FIXTURES[3]])
def test_empty_slots_write_nothing_but_their_zero_records(dev, name, kind):
    """caplens <= 2: nothing can be replaced.  A slot, a whole image (closed from the start: no kernel visits its rows), all."""
    case = SS.driver_case(name, kind, SS.MIXES[1])
    K, R = case["K"], case["gold"].shape[0]
    m = _model(kind, case["d"], dev)
    full, caps, caplens = _batch(m, case, dev)
    tags = None if case["tags"] is None else case["tags"].to(dev)
    keys = ("inputs", "replaced", "sample", "logp", "sum_logp", "n_replaced")
    for emptied in ([3], [2, 3], list(range(R))):
        lens = caplens.clone()
        for i, r in enumerate(emptied):
            lens[r] = (2, 1, 0)[i % 3]
        with torch.no_grad():
            got = m.mix_batch(case["wm"], case["enc"].to(dev), tags, caps, lens, case["prob"], per_image=K, seed=SS.SEED,
                              draw=SS.DRAW, temperature=TEMPERATURE)
        for r in range(R):
            if r in emptied:
                assert torch.equal(got["inputs"][r], caps[r]) and not bool(got["replaced"][r].any()), (emptied, r)
                assert bool((got["sample"][r] == -1).all()) and not bool(_bits(got["logp"][r]).any()), (emptied, r)
                assert int(_bits(got["sum_logp"])[r]) == 0 and int(got["n_replaced"][r]) == 0, (emptied, r)
            else:
                for k in keys:
                    assert torch.equal(_bits(got[k][r]), _bits(full[k][r])), (emptied, r, k)
    # the raw records of an image that is closed from the start: the zero-fill of the set-up and nothing else
    closed = dict(case, nmix=case["nmix"].clone())
    closed["nmix"][2:4] = 0
    res, steps = _device(m, kind, closed, dev, guard=256)
    assert steps == int(closed["nmix"].max()) and bool((res["guard"] == GUARD).all())
    for k in ("tokens", "replaced", "sample", "logp"):
        assert not bool(_bits(res[k][2:4]).any()), k
    assert not bool(_bits(res["sum_logp"][2:4]).any())
    res, steps = _device(m, kind, dict(case, nmix=torch.zeros_like(case["nmix"])), dev)
    assert steps == 0 and tuple(res["tokens"].shape) == (R, 0) and not bool(_bits(res["sum_logp"]).any())
