"""The rollout driver resident on the GPU (csrc/beam_search.cpp: scnattn_rollout_*, scnattn.functional.rollout_run,
models/decoders/_common.rollout_batched) against the CPU reference of tests/rollout_refs.py in fp64, against sample_batch(1)
for the arg-max rollout, and for what it writes.

A rollout is a chain of discrete choices, so the rule of tests/test_gpu_beam_search.py applies per ROW: a row counts when (1)
the CPU reference run in fp32 picks the fp64 reference's token at every step and (2) every step's fp64 gap between the picked
key and the best other key is at least max(8 x the worst fp32-vs-fp64 key difference of that row, 1e-5); both from the CPU
reference alone (rollout_refs.decidable_rows).  Rows that do not count are left out under asserted caps: at most 1/4 of all
rows of a table, at most 1/2 of any fixture's.  Bars (those of the beam tests): tokens and lengths equal, sum_logp within
1e-4 * max(1, |s|), alphas within 1e-4 of the row's largest."""
import pytest
import torch

import beam_refs as BR
import rollout_refs as RR
from helpers import params_from, t

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
INV_TEMP = float(torch.tensor(1.0 / 0.7, dtype=torch.float32))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def reference(kind, d, wm, enc, tags, K, seed, draw, inv_temp, greedy_first):
    """-> (fp64 rollout, per-row decidability); CPU only"""
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    tg = None if kind == "pure_attention" else tags
    r64 = RR.rollout(kind, P64, K, wm, enc.double(), None if tg is None else tg.double(), seed, draw, inv_temp, greedy_first)
    r32 = RR.rollout(kind, P32, K, wm, enc.float(), None if tg is None else tg.float(), seed, draw, inv_temp, greedy_first,
                     tokens=r64["tokens"])
    return r64, RR.decidable_rows(r64, r32)


def _device(m, kind, wm, enc, tags, K, seed, draw, inv_temp, greedy_first, dev, want_alpha=True, guard=0):
    from models.decoders import _common
    from scnattn import functional as SF
    V = len(wm)
    with torch.no_grad():
        dims, weights, e, tg = _common._search_operands(m, V, enc.to(dev), None if tags is None else tags.to(dev),
                                                        kind != "pure_scn", kind != "pure_attention")
        return SF.rollout_run(dims, K, weights, e, tg, wm["<start>"], wm["<end>"], seed, draw, inv_temp=inv_temp,
                              greedy_first=greedy_first, want_alpha=want_alpha, guard=guard)


def _compare(res, steps, ref, ok, use_att):
    """-> rows left out"""
    tok, lp = res["tokens"].cpu(), res["logp"].cpu()
    length, slp = res["length"].cpu().tolist(), res["sum_logp"].cpu().tolist()
    alpha = res["alpha"].cpu() if res["alpha"] is not None else None
    assert use_att == (alpha is not None)
    left = 0
    for r, good in enumerate(ok):
        if not good:
            left += 1
            continue
        n = ref["length"][r] or ref["steps"]
        assert steps >= n and length[r] == ref["length"][r], (r, length[r], ref["length"][r])
        assert tok[r, :n].tolist() == ref["tokens"][r][:n], (r, tok[r, :n].tolist(), ref["tokens"][r][:n])
        assert bool((tok[r, n:] == 0).all()) and bool((lp[r, n:] == 0).all()), "records behind <end> are not <pad> / 0.0"
        assert abs(slp[r] - ref["sum_logp"][r]) <= TOL_OUT * max(1.0, abs(ref["sum_logp"][r])), (r, slp[r], ref["sum_logp"][r])
        for s in range(n):
            assert abs(float(lp[r, s]) - ref["logp"][r][s]) <= TOL_OUT * max(1.0, abs(ref["logp"][r][s])), (r, s)
            if use_att:
                a, b = alpha[s, r].double(), ref["alpha"][s][r].double()
                assert float((a - b).abs().max()) <= TOL_OUT * float(b.abs().max()), (r, s)
    return left


# ---- (a) the four fixtures ----------------------------------------------------------------------------------------------
# (seed, draw) picked on the CPU reference alone, one per fixture and slot count.  Lengths they exercise (0: a row that uses all
# 51 steps): odd K=1 18 19 6 14 0 2; odd K=3 1 .. 35; distinct K=1 50 19 1 28; distinct K=3 0 .. 45 with two cut-off rows;
# pure_scn K=1 0 2 11 20; pure_scn K=3 0 .. 38; pure_attention K=1 1 2 11 28; pure_attention K=3 0 .. 38 with five cut-off
# rows.  None leaves a row out on the CPU reference.
SEEDS = {("attention_scn_odd", 1): (5, 0), ("attention_scn_odd", 3): (3, 1),
         ("attention_scn_distinct", 1): (5, 0), ("attention_scn_distinct", 3): (3, 0),
         ("pure_scn_distinct", 1): (3, 0), ("pure_scn_distinct", 3): (3, 1),
         ("pure_attention_distinct", 1): (3, 0), ("pure_attention_distinct", 3): (3, 1)}
_LEFT = {}


def fixture_case(name, kind, K):
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    enc = t(d["enc"])
    tags = t(d["tags"]) if kind != "pure_attention" else None
    seed, draw = SEEDS[(name, K)]
    ref, ok = reference(kind, d, wm, enc, tags, K, seed, draw, INV_TEMP, K > 1)
    return d, wm, enc, tags, seed, draw, ref, ok


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_fixture_rollout_vs_reference(dev, name, kind, K):
    """K = 1: one sampled caption per image; K = 3: the arg-max caption and two sampled ones; temperature 0.7"""
    from test_gpu_parity import _build_decoder
    d, wm, enc, tags, seed, draw, ref, ok = fixture_case(name, kind, K)
    m = _build_decoder(kind, d, dev).eval()
    res, steps = _device(m, kind, wm, enc, tags, K, seed, draw, INV_TEMP, K > 1, dev)
    left = _compare(res, steps, ref, ok, kind != "pure_scn")
    print("%s K=%d: %d of %d rows left out; lengths %s" % (name, K, left, len(ok), ref["length"]))
    assert 2 * left <= len(ok)
    _LEFT[(name, K)] = (left, len(ok), ref["length"])
    if len(_LEFT) == 2 * len(BR.FIXTURES):
        rows, out = sum(n for _, n, _ in _LEFT.values()), sum(o for o, _, _ in _LEFT.values())
        assert 4 * out <= rows, _LEFT
        lens = [l for _, _, ls in _LEFT.values() for l in ls]
        assert 0 in lens and (1 in lens or 2 in lens), "the table must hold a row that uses all steps and one that ends at once"


# ---- (b) vector-width shapes --------------------------------------------------------------------------------------------
VECTOR_SEEDS = {("attention_scn", 1): (6, 5, 0), ("attention_scn", 3): (6, 5, 1), ("pure_scn", 1): (78, 5, 0),
                ("pure_scn", 3): (78, 5, 1)}      # (parameter seed, rollout seed, draw)
# lengths on the CPU reference: K = 1 every row uses all 51 steps (both kinds); attention_scn K = 3: 6 26 0 1 16 38 4 0 6;
# pure_scn K = 3: 1 28 0 1 16 0 30 0 0; no row is left out


def vector_case(kind, K):
    from test_gpu_beam_search import _uniform_params
    pseed, seed, draw = VECTOR_SEEDS[(kind, K)]
    g = torch.Generator().manual_seed(pseed)
    d, V, E, S = _uniform_params(kind, g)
    enc, tags = torch.rand(3, 7, 7, E, generator=g), torch.rand(3, S, generator=g)
    wm = BR.word_map(V)
    ref, ok = reference(kind, d, wm, enc, tags, K, seed, draw, 1.0, K > 1)
    return d, wm, enc, tags, seed, draw, ref, ok


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("kind", ("attention_scn", "pure_scn"))
def test_vector_width_rollout_vs_reference(dev, kind, K):
    """E=256, A=128, D=F=128, M=64, S=40, 7x7, V=1003, N=3: the 16-byte paths of the two attention kernels; ld = V = 1003 is
    the pick's scalar path (its vector path: tests/test_gpu_rollout_kernels.py)"""
    from test_gpu_parity import _build_decoder
    d, wm, enc, tags, seed, draw, ref, ok = vector_case(kind, K)
    m = _build_decoder(kind, d, dev).eval()
    res, steps = _device(m, kind, wm, enc, tags, K, seed, draw, 1.0, K > 1, dev)
    left = _compare(res, steps, ref, ok, kind != "pure_scn")
    print("%s K=%d: %d of %d rows left out; lengths %s" % (kind, K, left, len(ok), ref["length"]))
    assert 4 * left <= len(ok)


# ---- (c) the arg-max rollout is the search of width one -------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_greedy_rollout_equals_sample_batch_of_one(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    cases = BR.oracle_cases(name, kind)
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    with torch.no_grad():
        beams = m.sample_batch(1, wm, enc, tags) if use_tags else m.sample_batch(1, wm, enc)
        caps, caplens, sum_logp = m.rollout_batch(wm, enc, tags, samples=1, seed=9, draw=0, greedy_first=True)
    res, steps = _device(m, kind, wm, enc, tags, 1, 9, 0, 1.0, True, dev, want_alpha=False)
    tok, length = res["tokens"].cpu(), res["length"].cpu().tolist()
    N = enc.shape[0]
    assert caps.dtype == torch.int64 and tuple(caplens.shape) == (2 * N, 1) and caps.is_cuda and sum_logp.is_cuda
    assert tuple(caps.shape) == (2 * N, caps.shape[1]) and tuple(sum_logp.shape) == (2 * N,)
    compared = 0
    for b in range(N):
        n = length[b] or steps
        mine = [V - 2] + tok[b, :n].tolist()
        # the public form: slot 0 of the K = 2 rollout is the same arg-max caption, <pad> behind it, caplens counts <start>
        assert int(caplens[2 * b]) == n + 1 and caps[2 * b, :n + 1].tolist() == mine and bool((caps[2 * b, n + 1:] == 0).all())
        assert abs(float(sum_logp[2 * b]) - float(res["sum_logp"][b])) <= 1e-5 * max(1.0, abs(float(sum_logp[2 * b])))
        if not cases[(b, 1)][1]:
            continue
        seq = beams[b][0] if use_att else beams[b]
        assert mine == seq, (b, mine, seq)
        compared += 1
    print("%s: %d of %d images compared" % (name, compared, enc.shape[0]))
    _GREEDY[name] = compared
    if len(_GREEDY) == len(BR.FIXTURES):
        assert sum(_GREEDY.values()) >= 8, _GREEDY


_GREEDY = {}


# ---- (d) nothing is written behind the workspace --------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [BR.FIXTURES[0], BR.FIXTURES[2]])
def test_workspace_guard_band(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    enc, tags = t(d["enc"]), t(d["tags"])
    K = 5
    for want_alpha in (False, True):
        res, steps = _device(m, kind, wm, enc, tags, K, 21, 2, 1.0, True, dev, want_alpha=want_alpha, guard=4096)
        assert steps >= 1 and bool((res["guard"] == 0x7FC5A5A5).all()), "words behind the workspace were overwritten"
        assert (res["alpha"] is not None) == (want_alpha and kind != "pure_scn")
        nopen, nsrc, length = res["nopen"].cpu(), res["nsrc"].cpu(), res["length"].cpu()
        assert int(res["open_rows"]) == int(nopen.sum()) == int((length == 0).sum())
        assert torch.equal(nsrc, torch.where(nopen > 0, torch.full_like(nsrc, K), torch.zeros_like(nsrc)))
        assert torch.equal(nopen, (length.view(-1, K) == 0).sum(dim=1).to(torch.int32))
        assert bool(torch.isfinite(res["sum_logp"]).all()) and bool((res["sum_logp"] <= 0).all())
        assert tuple(res["tokens"].shape) == (enc.shape[0] * K, steps) and res["tokens"].is_cuda
