"""CPU tests of tests/rollout_refs.py -- the references the GPU rollout / weighted-loss tests are judged by -- and of the
host-side refusals of the self-critical training surface (scnattn.functional.rollout_run, CaptionScorer.score_rows,
trains.harness.SCSTTrainStep, the C entry points' argument checks, which run before anything is launched)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import beam_refs as BR
import rollout_refs as RR
from helpers import params_from, t

F64 = torch.float64


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = RR.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want


def test_noise_is_a_function_of_seed_draw_row_step_word():
    seed = 0x0123456789abcdef
    a = RR.noise_bits(seed, 3, 5, 7, 11)
    assert a.dtype == np.uint32 and a.shape == (11,)
    w = RR.philox4x32_10((2, 5, 7, 3), (0x89abcdef, 0x01234567))        # word v = 9: counter (9 >> 2, row, t, draw), word 9 & 3
    assert int(a[9]) == int(w[1])
    assert np.array_equal(RR.noise_bits(seed, 3, 5, 7, 2051)[:11], a)    # not of V
    for other in (RR.noise_bits(seed + 1, 3, 5, 7, 11), RR.noise_bits(seed, 4, 5, 7, 11), RR.noise_bits(seed, 3, 6, 7, 11),
                  RR.noise_bits(seed, 3, 5, 8, 11), RR.noise_bits(seed ^ (1 << 40), 3, 5, 7, 11)):
        assert not np.array_equal(other, a)


def test_uniform_is_exact_and_inside_the_unit_interval():
    bits = np.array([0, 0x1ff, 0x200, 0xffffffff, 0x80000000], dtype=np.uint32)
    u32, u64 = RR.uniform(bits, torch.float32), RR.uniform(bits, F64)
    assert torch.equal(u32.double(), u64)
    assert float(u64.min()) == 2.0 ** -24 and float(u64.max()) == 1.0 - 2.0 ** -24
    g = -torch.log(-torch.log(u64))
    assert -2.82 < float(g.min()) and float(g.max()) < 16.64


# ---- the sampler --------------------------------------------------------------------------------------------------------
def test_sampler_follows_softmax():
    """R = 4000 rows x 2 steps at V = 8: every token's count within 4.5 binomial standard deviations of n * softmax(y)[v]
    (fixed seeds: deterministic); P(|z| > 4.5) = 7e-6 per token"""
    V, R = 8, 4000
    x = torch.tensor([0.3, -1.2, 2.0, 0.0, 1.1, -0.4, 0.7, 1.9], dtype=F64)
    for inv_temp in (1.0, 1.0 / 0.7):
        counts = torch.zeros(V, dtype=F64)
        for step in (0, 5):
            p = RR.pick(x.expand(R, V).contiguous(), 1, inv_temp, 99, 2, step, False)
            counts += torch.bincount(p["token"], minlength=V).double()
        n = 2 * R
        prob = torch.softmax(x * inv_temp, dim=0)
        z = (counts - n * prob) / torch.sqrt(n * prob * (1 - prob))
        print("inv_temp %.3f: z = %s" % (inv_temp, [round(float(v), 2) for v in z]))
        assert float(z.abs().max()) <= 4.5
        lp = torch.log_softmax(x * inv_temp, dim=0)
        assert torch.allclose(p["logp"], lp[p["token"]], rtol=0, atol=1e-12)


def test_greedy_slot_takes_the_lowest_index_among_equal_maxima():
    x = torch.tensor([[0.5, 2.0, 2.0, -1.0, 2.0], [1.0, 1.0, 1.0, 1.0, 1.0], [0.0, 0.1, 0.2, 0.3, 3.0]], dtype=F64)
    p = RR.pick(x, 1, 1.0, 5, 0, 0, True)             # K = 1 with greedy_first: every row is an arg-max row
    assert p["token"].tolist() == [1, 0, 4] and float(p["g"].abs().max()) == 0.0
    p = RR.pick(x, 3, 1.0, 5, 0, 0, True)             # K = 3: only rows 0, 3, ... are
    assert float(p["g"][0].abs().max()) == 0.0 and float(p["g"][1].abs().min()) > 0.0 and float(p["g"][2].abs().min()) > 0.0
    assert RR.token_ok(p, 0, 1) and not RR.token_ok(p, 0, 2) and not RR.token_ok(p, 0, 0)


def test_band_leaves_almost_no_row_ambiguous():
    """the GPU test's case cap (1 % of the rows) on rows like its own: 1 of 2000 at V = 1003 (a top-2 gap is below 2e-5 about once in
    50 000 rows)"""
    g = torch.Generator().manual_seed(1)
    x = ((torch.rand(2000, 1003, generator=g) * 6 - 3).float()).double()
    p = RR.pick(x, 1, 1.0 / 0.7, 7, 1, 3, False)
    n = int(RR.ambiguous(p).sum())
    print("ambiguous rows: %d of 2000, widest band %.3e, narrowest gap %.3e" % (n, float(RR.band(p).max()), float(p["gap"].min())))
    assert n <= 20
    p32 = RR.pick(x.float(), 1, 1.0 / 0.7, 7, 1, 3, False)
    assert all(RR.token_ok(p, i, int(p32["token"][i])) for i in range(2000))      # torch's CPU fp32 passes the judge
    for i in range(0, 2000, 97):
        want, bound = RR.logp_at(p, i, int(p32["token"][i]))
        assert abs(float(p32["logp"][i]) - want) <= bound


# ---- the weighted loss --------------------------------------------------------------------------------------------------
def _loss_case(V, lens, seed=0):
    g = torch.Generator().manual_seed(40 + V + seed)
    B, T, P = len(lens), 4, 9
    scores = (torch.randn(B, T, V, generator=g) * 2.0).double()
    targets = torch.randint(0, V, (B, T + 2), generator=g)
    alphas = (torch.rand(B, T, P, generator=g) * 0.5).double()
    return scores, targets, alphas


def test_weighted_loss_reference_equals_autograd():
    lens = (4, 0, 2)
    scores, targets, alphas = _loss_case(37, lens)
    w = torch.tensor([-1.5, 3.0, 0.0], dtype=F64)
    scores.requires_grad_(True)
    n = sum(lens)
    nll = sum(w[b] * (torch.logsumexp(scores[b, tt], 0) - scores[b, tt, targets[b, tt]]) for b in range(3) for tt in range(lens[b]))
    want = nll / n + 0.7 * ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    want.backward()
    want = want.detach()
    ref = RR.weighted_loss(scores.detach(), targets, lens, w, alphas, 0.7)
    assert abs(float(ref["loss"]) - float(want)) <= 1e-13 * max(1.0, abs(float(want)))
    assert float(ref["row_loss"][1].abs().max()) == 0.0 and float(ref["row_loss"][2].abs().max()) == 0.0
    dwant, bound = RR.weighted_bwd(scores.detach().float(), targets, ref["row_lse"], w, lens, 1.0)     # the scores are fp32 values
    assert torch.allclose(dwant, scores.grad, rtol=0, atol=1e-13)
    assert float(bound[1].abs().max()) == 0.0 and float(bound[2].abs().max()) == 0.0 and float(bound[0].min()) > 0.0


def test_weighted_loss_with_unit_weights_is_the_caption_loss():
    from oracle import scnattn_ref as R_
    lens = (4, 2, 1)
    scores, targets, alphas = _loss_case(37, lens, seed=1)
    caps = torch.cat([torch.zeros(3, 1, dtype=torch.long), targets], dim=1)       # targets = caps[:, 1:]
    want = R_.caption_loss(scores, caps, list(lens), alphas, 0.7)[0]
    ref = RR.weighted_loss(scores, targets, lens, torch.ones(3, dtype=F64), alphas, 0.7)
    assert abs(float(ref["loss"]) - float(want)) <= 1e-13
    want = R_.caption_loss(scores, caps, list(lens), None)[0]
    assert abs(float(RR.weighted_loss(scores, targets, lens, torch.ones(3, dtype=F64))["loss"]) - float(want)) <= 1e-13


# ---- whole rollouts -----------------------------------------------------------------------------------------------------
_COMPARED = {}


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_greedy_rollout_is_the_beam_search_of_width_one(name, kind):
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    cases = BR.oracle_cases(name, kind)
    P64 = params_from(d, dtype=F64)
    enc = t(d["enc"]).double()
    tags = t(d["tags"]).double() if kind != "pure_attention" else None
    res = RR.rollout(kind, P64, 1, wm, enc, tags, seed=1, draw=0, greedy_first=True)
    compared = 0
    for b in range(enc.shape[0]):
        ref, ok = cases[(b, 1)]
        if not ok or ref is None:
            continue
        seq = ref[0][0] if kind != "pure_scn" else ref[0]
        assert RR.caption_of(res, b, V - 2) == seq, (b, RR.caption_of(res, b, V - 2), seq)
        compared += 1
    print("%s: %d of %d images compared" % (name, compared, enc.shape[0]))
    _COMPARED[name] = compared
    if len(_COMPARED) == len(BR.FIXTURES):          # the oracle completes nothing with one beam on some fixtures
        assert sum(_COMPARED.values()) >= 4, _COMPARED


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_sampled_rollout_sum_logp_is_its_teacher_forced_likelihood(name, kind):
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    P64 = params_from(d, dtype=F64)
    enc = t(d["enc"]).double()[:2]
    tags = t(d["tags"]).double()[:2] if kind != "pure_attention" else None
    K, inv_temp = 2, 1.0 / 0.7
    res = RR.rollout(kind, P64, K, wm, enc, tags, seed=11, draw=4, inv_temp=inv_temp, greedy_first=True, max_steps=12)
    for r in range(2 * K):
        n = r // K
        seq = RR.caption_of(res, r, V - 2)
        want = RR.teacher_forced_logp(kind, P64, seq, enc[n:n + 1], None if tags is None else tags[n:n + 1], inv_temp)
        assert abs(res["sum_logp"][r] - want) <= 1e-9 * max(1.0, abs(want)), (r, res["sum_logp"][r], want)
        assert abs(sum(res["logp"][r]) - want) <= 1e-9 * max(1.0, abs(want))
        ln = res["length"][r]
        assert all(x == 0 for x in res["tokens"][r][ln:]) if ln else len(res["tokens"][r]) == 12
    r32 = RR.rollout(kind, params_from(d, dtype=torch.float32), K, wm, enc.float(), None if tags is None else tags.float(),
                     seed=11, draw=4, inv_temp=inv_temp, greedy_first=True, max_steps=12, tokens=res["tokens"])
    assert len(RR.decidable_rows(res, r32)) == 2 * K


# ---- refusals on the host -----------------------------------------------------------------------------------------------
def _dims(V=50):
    return (2, 4, 8, 8, 8, 8, 8, 3, V, 51, 51, 1)


def test_rollout_run_refuses_bad_arguments_before_touching_a_device():
    from scnattn import functional as SF
    x = torch.zeros(1)
    for K in (0, 9):
        with pytest.raises(ValueError, match="K must be in"):
            SF.rollout_run(_dims(), K, (), x, x, 48, 49, 0, 0)
    for it in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="inv_temp"):
            SF.rollout_run(_dims(), 2, (), x, x, 48, 49, 0, 0, inv_temp=it)
    with pytest.raises(ValueError, match="seed"):
        SF.rollout_run(_dims(), 2, (), x, x, 48, 49, -1, 0)
    with pytest.raises(ValueError, match="vocabulary"):
        SF.rollout_run(_dims(), 2, (), x, x, 48, 50, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.rollout_run(_dims(), 2, (), x, x, 48, 49, 0, 0)


def test_rollout_batch_and_scst_step_refuse_bad_arguments():
    from models.decoders._common import check_rollout_args
    from trains.harness import SCSTTrainStep
    assert check_rollout_args(5, 1.0, True) == 6 and check_rollout_args(8, 0.5) == 8
    for samples, greedy in ((0, False), (9, False), (8, True)):
        with pytest.raises(ValueError, match="slots per image"):
            check_rollout_args(samples, 1.0, greedy)
    for temp in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            check_rollout_args(2, temp)
    scorer = type("S", (), {"score_rows": None})()
    with pytest.raises(ValueError, match="samples >= 2"):
        SCSTTrainStep(scorer=scorer, samples=1, baseline="mean", device="cpu", encoder=False)
    with pytest.raises(ValueError, match="baseline"):
        SCSTTrainStep(scorer=scorer, baseline="median", device="cpu", encoder=False)
    with pytest.raises(ValueError, match="temperature"):
        SCSTTrainStep(scorer=scorer, temperature=0.0, device="cpu", encoder=False)
    with pytest.raises(ValueError, match="slots per image"):
        SCSTTrainStep(scorer=scorer, samples=8, baseline="greedy", device="cpu", encoder=False)
    with pytest.raises(ValueError, match="scorer"):
        SCSTTrainStep(scorer=None, device="cpu", encoder=False)
    small = dict(emb_dim=8, attention_dim=8, decoder_dim=8, factored_dim=8, semantic_dim=3, vocab_size=50, dropout=0.0)
    ts = SCSTTrainStep(scorer=scorer, samples=2, baseline="mean", device="cpu", encoder=False, **small)
    assert ts.K == 2 and ts.draw == 0 and len(ts.word_map) == 50 and ts.word_map["<end>"] == 49
    with pytest.raises(ValueError, match="image_index"):
        ts.step(None, torch.zeros(3, 3), torch.arange(2), encoder_out=torch.zeros(3, 2, 2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.step(None, torch.zeros(3, 3), torch.arange(3), encoder_out=torch.zeros(3, 2, 2, 8))


def test_score_rows_refuses_a_mismatched_image_index():
    from scnattn.textmetrics import CaptionScorer
    s = CaptionScorer.__new__(CaptionScorer)            # the constructor needs a device; the checks under test do not
    s.ref, s.ref_len = torch.zeros(4, 2, 5, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32)
    s.N, s.R, s.Lr, s.skip_ref = 4, 2, 5, ()
    hyp, hl = torch.zeros(3, 6, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="image_index"):
        s.score_rows(torch.arange(4), hyp, hl)
    with pytest.raises(ValueError, match="image_index"):
        s.score_rows(torch.zeros(3), hyp, hl)
    with pytest.raises(ValueError, match="outside"):
        s.score_rows(torch.tensor([0, 4, 1]), hyp, hl)
    with pytest.raises(ValueError, match="outside"):
        s.score_rows(torch.tensor([0, -1, 1]), hyp, hl)
    with pytest.raises(ValueError, match="hyp_len"):
        s.score_rows(torch.arange(3), hyp, hl[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.score_rows(torch.tensor([0, 3, 1]), hyp, hl)


# ---- refusals of the C entry points --------------------------------------------------------------------------------------
_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error().decode(), h.scnattn_last_error()


def test_entry_points_refuse_before_launching():
    from scnattn import _lib as L
    h = L.lib()
    d = L.Dims(*_dims())
    nbytes, off = C.c_size_t(), (C.c_long * L.ROLLOUT_NOFF)()
    for K in (0, 9):
        _refused(h, h.scnattn_rollout_workspace(C.byref(d), K, 51, 0, C.byref(nbytes)), "beam_size must be in [1, 8]")
    _refused(h, h.scnattn_rollout_workspace(C.byref(d), 2, 0, 0, C.byref(nbytes)), "max_steps")
    _refused(h, h.scnattn_rollout_layout(C.byref(d), 2, 51, 0, None), "offsets is NULL")
    assert h.scnattn_rollout_workspace(C.byref(d), 3, 51, 0, C.byref(nbytes)) == 0 and nbytes.value > 0
    small = nbytes.value
    assert h.scnattn_rollout_workspace(C.byref(d), 3, 51, 1, C.byref(nbytes)) == 0
    extra = 4 * 51 * 6 * 4                                          # the alpha records [max_steps][N*K][P], only when asked for
    assert extra <= nbytes.value - small < extra + 256
    assert h.scnattn_rollout_layout(C.byref(d), 3, 51, 0, off) == 0
    need = [1, 2, 2, 6, 6, 51 * 6, 51 * 6]                          # every result has its room and starts 16-byte aligned
    assert off[0] == 0 and off[7] == -1 and all(off[i + 1] - off[i] >= need[i] and off[i] % 4 == 0 for i in range(6))
    assert h.scnattn_rollout_layout(C.byref(d), 3, 51, 1, off) == 0 and off[7] - off[6] >= need[6] and off[7] % 4 == 0
    assert 4 * off[7] + extra <= nbytes.value
    w = L.Params()
    _refused(h, h.scnattn_rollout_init(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 50, _P), "start token")
    _refused(h, h.scnattn_rollout_init(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P + 4), "16-byte aligned")
    for it in (0.0, -1.0, float("inf"), float("nan")):
        _refused(h, h.scnattn_rollout_steps(None, C.byref(d), 2, 51, 0, C.byref(w), _P, 49, it, 1, 0, 0, 0, 1, _P), "inv_temp")
    _refused(h, h.scnattn_rollout_steps(None, C.byref(d), 2, 51, 0, C.byref(w), _P, 50, 1.0, 1, 0, 0, 0, 1, _P), "end token")
    _refused(h, h.scnattn_rollout_steps(None, C.byref(d), 2, 51, 0, C.byref(w), _P, 49, 1.0, 1, 0, 0, -1, 1, _P), "negative step")
    state = (C.c_void_p * 7)(*([_P] * 7))
    _refused(h, h.scnattn_rollout_pick(None, 2, 9, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, state), "slot count")
    _refused(h, h.scnattn_rollout_pick(None, 2, 2, 50, _P, 49, 1.0, 1, 0, 0, 0, 49, 51, state), "bad argument")
    _refused(h, h.scnattn_rollout_pick(None, 2, 2, 50, _P, 50, 0.0, 1, 0, 0, 0, 49, 51, state), "inv_temp")
    _refused(h, h.scnattn_rollout_pick(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 51, 0, 49, 51, state), "step beyond the records")
    _refused(h, h.scnattn_rollout_pick(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, None), "state is NULL")
    _refused(h, h.scnattn_rollout_advance(None, 2, 2, 0, 50, _P, _P, _P, _P, _P), "bad dims")
    _refused(h, h.scnattn_rollout_advance(None, 2, 2, 8, 50, _P, _P, None, _P, _P), "null operand")
    _refused(h, h.scnattn_caption_loss_weighted_fwd(None, 3, 4, 37, 0, _P, _P, 6, _P, 7, None, None, 0.0, _P, _P, None, None, _P),
             "row_weight is NULL")
    _refused(h, h.scnattn_caption_loss_weighted_fwd(None, 3, 4, 37, 0, _P, _P, 3, _P, 7, _P, None, 0.0, _P, _P, None, None, _P),
             "bad argument")
    _refused(h, h.scnattn_caption_loss_weighted_bwd(None, 3, 4, 37, 0, _P, _P, 6, _P, 7, None, _P, None, 0.0, _P, _P, None),
             "row_weight is NULL")
    _refused(h, h.scnattn_caption_loss_weighted_bwd(None, 3, 4, 37, 9, _P, _P, 6, _P, 7, _P, _P, None, 0.0, _P, _P, _P),
             "dalphas without sm1")


def test_header_declares_the_new_symbols_and_keeps_the_version():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "scnattn.h")).read()
    from scnattn import _lib as L
    for sym in ("scnattn_rollout_workspace", "scnattn_rollout_layout", "scnattn_rollout_init", "scnattn_rollout_steps",
                "scnattn_rollout_pick", "scnattn_rollout_advance", "scnattn_caption_loss_weighted_fwd",
                "scnattn_caption_loss_weighted_bwd"):
        assert "int %s(" % sym in header and sym in L.EXPORTS
    assert "#define SCNATTN_VERSION 109 " in header and "#define SCNATTN_ROLLOUT_NOFF %d" % L.ROLLOUT_NOFF in header
    assert math.isclose(RR.U, 2.0 ** -24)
