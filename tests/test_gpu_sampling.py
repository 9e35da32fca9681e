"""Truncated sampling resident on the GPU: the driver (csrc/beam_search.cpp: scnattn_rollout_*_f, scnattn.functional.rollout_run
with top_k / top_p), `rollout_batch(top_k=, top_p=)` and `Captioner.sample` against the fp64 reference of tests/sampling_refs.py,
per row, under its EXTENDED decidability rule (its docstring), all from the CPU reference alone.  The cases and their
(seed, draw) are stated in tests/sampling_cases.py; tests/test_sampling_refs.py asserts the caps on rows left out there, without
a GPU: at most 1/4 of the table and at most 1/2 of any fixture.  Bars (those of tests/test_gpu_rollout.py): tokens, lengths and
nkeep equal, sum_logp and logp within 1e-4 * max(1, |.|)."""
import pytest
import torch

import beam_refs as BR
import rollout_refs as RR
import sampling_cases as SC
import sampling_refs as SR
from helpers import t

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _device(m, kind, wm, enc, tags, K, seed, draw, inv_temp, greedy_first, dev, top_k=0, top_p=1.0, want_alpha=False, guard=0,
            force_filtered=False, chunk=None):
    from models.decoders import _common
    from scnattn import functional as SF
    V = len(wm)
    kw = {} if chunk is None else {"chunk": chunk}
    with torch.no_grad():
        dims, weights, e, tg = _common._search_operands(m, V, enc.to(dev), None if tags is None else tags.to(dev),
                                                        kind != "pure_scn", kind != "pure_attention")
        return SF.rollout_run(dims, K, weights, e, tg, wm["<start>"], wm["<end>"], seed, draw, inv_temp=inv_temp,
                              greedy_first=greedy_first, want_alpha=want_alpha, guard=guard, top_k=top_k, top_p=top_p,
                              force_filtered=force_filtered, **kw)


def _compare(res, steps, ref, ok):
    """-> rows left out"""
    tok, lp, nk = res["tokens"].cpu(), res["logp"].cpu(), res["nkeep"].cpu()
    length, slp = res["length"].cpu().tolist(), res["sum_logp"].cpu().tolist()
    left = 0
    for r, good in enumerate(ok):
        if not good:
            left += 1
            continue
        n = ref["length"][r] or ref["steps"]
        assert steps >= n and length[r] == ref["length"][r], (r, length[r], ref["length"][r])
        assert tok[r, :n].tolist() == ref["tokens"][r][:n], (r, tok[r, :n].tolist(), ref["tokens"][r][:n])
        assert nk[r, :n].tolist() == [ref["nkeep"][s][r] for s in range(n)], (r, nk[r, :n].tolist())
        assert bool((tok[r, n:] == 0).all()) and bool((lp[r, n:] == 0).all()) and bool((nk[r, n:] == 0).all()), \
            "records behind <end> are not <pad> / 0.0 / 0"
        assert abs(slp[r] - ref["sum_logp"][r]) <= TOL_OUT * max(1.0, abs(ref["sum_logp"][r])), (r, slp[r], ref["sum_logp"][r])
        for s in range(n):
            assert abs(float(lp[r, s]) - ref["logp"][r][s]) <= TOL_OUT * max(1.0, abs(ref["logp"][r][s])), (r, s)
    return left


# ---- (a) the four fixtures, three filters ----------------------------------------------------------------------------------
_LEFT = {}


@pytest.mark.parametrize("filt", sorted(SC.DRIVER_FILTERS))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_fixture_filtered_rollout_vs_reference(dev, name, kind, K, filt):
    """K = 1: one sampled caption per image; K = 3: the arg-max caption and two sampled ones; temperature 0.7"""
    from test_gpu_parity import _build_decoder
    d, wm, enc, tags, seed, draw, ref, ok = SC.fixture_case(name, kind, K, filt)
    top_k, top_p = SC.DRIVER_FILTERS[filt]
    m = _build_decoder(kind, d, dev).eval()
    res, steps = _device(m, kind, wm, enc, tags, K, seed, draw, SC.DRIVER_INV_TEMP, K > 1, dev, top_k, top_p)
    left = _compare(res, steps, ref, ok)
    print("%s K=%d %s: %d of %d rows left out; lengths %s" % (name, K, filt, left, len(ok), ref["length"]))
    assert 2 * left <= len(ok)
    if top_k:
        # every sampled token of a top_k = k rollout is among the k best of its row's logits, as the reference recomputes them
        # on the decidable rows: its kept set at that step holds at most k words and holds the device's token
        tok = res["tokens"].cpu()
        for r, good in enumerate(ok):
            for s in range(SR.open_steps(ref, r) if good else 0):
                assert ref["nkeep"][s][r] <= top_k and int(tok[r, s]) == ref["tokens"][r][s]
                assert ref["rank"][s][r] < top_k, (r, s, ref["rank"][s][r])
    _LEFT[(name, K, filt)] = (left, len(ok))
    if len(_LEFT) == 2 * len(BR.FIXTURES) * len(SC.DRIVER_FILTERS):
        rows, out = sum(n for _, n in _LEFT.values()), sum(o for o, _ in _LEFT.values())
        assert 4 * out <= rows, _LEFT


# ---- (b) the vector-width shape --------------------------------------------------------------------------------------------
def test_vector_width_filtered_rollout_vs_reference(dev):
    """E=256, A=128, D=F=128, M=64, S=40, 7x7, V=1003, N=3, K=3 with (50, 0.9): ld = V = 1003 is the filtered pick's scalar
    staging path inside the driver"""
    from test_gpu_parity import _build_decoder
    kind, K = "attention_scn", 3
    d, wm, enc, tags, seed, draw, ref, ok = SC.vector_case(kind, K)
    m = _build_decoder(kind, d, dev).eval()
    res, steps = _device(m, kind, wm, enc, tags, K, seed, draw, 1.0, True, dev, *SC.VECTOR_FILTER)
    left = _compare(res, steps, ref, ok)
    print("vector %s K=%d: %d of %d rows left out; lengths %s" % (kind, K, left, len(ok), ref["length"]))
    assert 4 * left <= len(ok)
    # the same bits for another chunking of the steps
    res2, steps2 = _device(m, kind, wm, enc, tags, K, seed, draw, 1.0, True, dev, *SC.VECTOR_FILTER, chunk=3)
    n = min(steps, steps2)
    for k in ("tokens", "logp", "nkeep"):
        a, b = res[k][:, :n].cpu().contiguous(), res2[k][:, :n].cpu().contiguous()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert torch.equal(res["sum_logp"].cpu().view(torch.int32), res2["sum_logp"].cpu().view(torch.int32))


# ---- (c) filter off: the plain run, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_filter_off_run_of_the_filtered_entry_points_equals_the_plain_run(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    enc = t(d["enc"])
    tags = t(d["tags"]) if kind != "pure_attention" else None
    a, sa = _device(m, kind, wm, enc, tags, 3, 5, 1, SC.DRIVER_INV_TEMP, True, dev, want_alpha=True)
    assert a["nkeep"] is None
    for top_k in (0, V, V + 5):             # off by default, and off because top_k covers the vocabulary
        b, sb = _device(m, kind, wm, enc, tags, 3, 5, 1, SC.DRIVER_INV_TEMP, True, dev, top_k=top_k, want_alpha=True,
                        force_filtered=True)
        assert sa == sb
        for k in ("open_rows", "nsrc", "nopen", "length", "sum_logp", "tokens", "logp", "alpha"):
            if a[k] is None:
                assert b[k] is None
                continue
            x, y = a[k].cpu().contiguous(), b[k].cpu().contiguous()
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
        assert bool((b["nkeep"] == 0).all()), "nothing writes nkeep when the filter is off: the zeros of _init_f"


# ---- (d) nothing is written behind the workspace ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [BR.FIXTURES[0], BR.FIXTURES[2]])
def test_workspace_guard_band(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    enc, tags = t(d["enc"]), t(d["tags"])
    K = 5
    for want_alpha in (False, True):
        res, steps = _device(m, kind, wm, enc, tags, K, 21, 2, 1.0, True, dev, top_k=4, top_p=0.9, want_alpha=want_alpha,
                             guard=4096)
        assert steps >= 1 and bool((res["guard"] == 0x7FC5A5A5).all()), "words behind the workspace were overwritten"
        assert (res["alpha"] is not None) == (want_alpha and kind != "pure_scn")
        nopen, nsrc, length = res["nopen"].cpu(), res["nsrc"].cpu(), res["length"].cpu()
        assert int(res["open_rows"]) == int(nopen.sum()) == int((length == 0).sum())
        assert torch.equal(nsrc, torch.where(nopen > 0, torch.full_like(nsrc, K), torch.zeros_like(nsrc)))
        assert torch.equal(nopen, (length.view(-1, K) == 0).sum(dim=1).to(torch.int32))
        assert bool(torch.isfinite(res["sum_logp"]).all()) and bool((res["sum_logp"] <= 0).all())
        nk, tok = res["nkeep"].cpu(), res["tokens"].cpu()
        assert tuple(nk.shape) == (enc.shape[0] * K, steps) and bool(((nk >= 0) & (nk <= 4)).all())
        n_tok = torch.where(length > 0, length, torch.full_like(length, steps)).unsqueeze(1)
        live = torch.arange(steps).unsqueeze(0) < n_tok
        assert bool((nk[live] >= 1).all()) and bool((nk[~live] == 0).all()) and bool((tok[~live] == 0).all())


# ---- (e) the public forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_rollout_batch_with_a_filter_is_the_driver_run(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, wm, enc, tags, seed, draw, ref, ok = SC.fixture_case(name, kind, 3, "k4p0.9")
    m = _build_decoder(kind, d, dev).eval()
    res, steps = _device(m, kind, wm, enc, tags, 3, seed, draw, SC.DRIVER_INV_TEMP, True, dev, 4, 0.9)
    with torch.no_grad():
        caps, caplens, sum_logp = m.rollout_batch(wm, enc.to(dev), None if tags is None else tags.to(dev), samples=2, seed=seed,
                                                  draw=draw, temperature=1.0 / SC.DRIVER_INV_TEMP, greedy_first=True, top_k=4,
                                                  top_p=0.9)
    V = len(wm)
    tok, length = res["tokens"].cpu(), res["length"].cpu().tolist()
    assert caps.is_cuda and caps.dtype == torch.int64 and tuple(caplens.shape) == (len(ok), 1)
    for r in range(len(ok)):
        n = length[r] or steps
        assert int(caplens[r]) == n + 1 and caps[r, :n + 1].tolist() == [V - 2] + tok[r, :n].tolist()
        assert bool((caps[r, n + 1:] == 0).all())
    # 1 / (1 / 0.7) need not round back to the driver's inv_temp: the likelihoods agree to fp32 rounding, the tokens above exactly
    assert torch.allclose(sum_logp.cpu(), res["sum_logp"].cpu(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ("attention_scn", "pure_scn", "pure_attention"))
def test_captioner_sample(dev, kind):
    """the stand-in trunks of tests/test_gpu_captioner.py: record shapes, words match tokens, (seed, draw) repeats, the next
    draw differs, and the records are those of rollout_batch on the same batch"""
    import test_gpu_captioner as TC
    from scnattn.inference import Captioner
    wm = BR.word_map(TC.V)
    rev = {v: k for k, v in wm.items()}
    enc, tag, dec = TC._modules(kind, dev)
    images = TC._images()
    cap = Captioner(enc, dec, wm, tagger=tag)
    a = cap.sample(images, samples=3, temperature=0.9, top_k=5, top_p=0.95, seed=7, draw=0, greedy_first=True)
    b = cap.sample(images, samples=3, temperature=0.9, top_k=5, top_p=0.95, seed=7, draw=0, greedy_first=True)
    c = cap.sample(images, samples=3, temperature=0.9, top_k=5, top_p=0.95, seed=7, draw=1, greedy_first=True)
    special = {wm["<start>"], wm["<end>"], wm["<pad>"]}
    assert len(a) == len(images) and all(len(recs) == 4 for recs in a)
    for recs in a:
        for rec in recs:
            assert sorted(rec) == ["logp", "tokens", "words"]
            seq = rec["tokens"]
            assert seq[0] == wm["<start>"] and wm["<end>"] not in seq[1:-1]        # <start> is a word a sample may draw
            assert len(seq) <= 52 and (seq[-1] == wm["<end>"] or len(seq) == 52)
            assert rec["words"] == [rev[w] for w in seq if w not in special]
            assert isinstance(rec["logp"], float) and rec["logp"] <= 0.0
    assert a == b
    assert [[r["tokens"] for r in recs[1:]] for recs in a] != [[r["tokens"] for r in recs[1:]] for recs in c]
    assert [recs[0]["tokens"] for recs in a] == [recs[0]["tokens"] for recs in c]          # the arg-max slot has no noise
    # the same batch by hand
    import resize_refs as RZ
    from oracle import data_ref as DR
    batch = torch.stack([DR.image_item(RZ.rows(im, TC.SIZE)) for im in images]).to(dev)
    with torch.no_grad():
        eo, tg = enc(batch).float(), tag(batch).float()
        caps, caplens, slp = dec.rollout_batch(wm, eo, None if kind == "pure_attention" else tg, samples=3, seed=7, draw=0,
                                               temperature=0.9, greedy_first=True, top_k=5, top_p=0.95)
    caps, caplens, slp = caps.cpu(), caplens.cpu(), slp.cpu()
    flat = [rec for recs in a for rec in recs]
    for r, rec in enumerate(flat):
        assert rec["tokens"] == caps[r, :int(caplens[r])].tolist() and rec["logp"] == float(slp[r])
    with pytest.raises(ValueError, match="top_p"):
        cap.sample(images, top_p=0.0)
    with pytest.raises(ValueError, match="slots per image"):
        cap.sample(images, samples=8, greedy_first=True)
