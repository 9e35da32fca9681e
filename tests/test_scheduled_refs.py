"""CPU tests of the references of scheduled sampling (tests/scheduled_refs.py): the coin against a plain-integer Philox and
against numpy's own fp32 evaluation of its definition, the two ends prob = 0 and prob = 1, the mixed run at prob = 1 against
rollout_refs.rollout, the share of rows the GPU module judges (on the reference alone, for exactly its cases), the bindings and
the layout, the refusals of the C entry points and of the Python layers, and scheduled_sampling_prob's staircase."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import beam_refs as BR
import rollout_refs as RR
import scheduled_refs as SS
from helpers import params_from, t

SYMBOLS = ("scnattn_rollout_workspace_ss", "scnattn_rollout_layout_ss", "scnattn_rollout_init_ss", "scnattn_rollout_steps_ss",
           "scnattn_rollout_pick_mixed")


# ---- the coin ----------------------------------------------------------------------------------------------------------------
def _philox_ints(c, k):
    """Philox4x32-10 on Python integers, from the paper: no numpy, no shared code with rollout_refs"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_coin_bits_are_word_0_of_the_reserved_counter():
    seed, draw = 0x5eed0123456789ab, 7
    for r, step in ((0, 0), (1, 0), (0, 1), (17, 50), (2 ** 20 - 1, 3)):
        want = _philox_ints((0xFFFFFFFF, r, step, draw), (seed & 0xFFFFFFFF, seed >> 32))[0]
        assert int(SS.coin_bits(seed, draw, r, step)) == want
    # a word's noise never uses that counter: its first word is v >> 2 < 2^30
    assert ((2 ** 31 - 1) >> 2) < 2 ** 30 < SS.COIN_WORD


def test_replaced_count_over_4096_pairs_equals_numpys_evaluation_of_the_definition():
    seed, draw = 5, 3
    rows, steps = np.meshgrid(np.arange(128), np.arange(32), indexing="ij")
    got = SS.coin(seed, draw, rows, steps, 0.25)
    assert got.shape == (128, 32)
    bits = RR.philox4x32_10((0xFFFFFFFF, rows, steps, draw), (seed, 0))[0]
    u32 = ((bits >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)      # fp32 throughout
    assert u32.dtype == np.float32 and bool((u32.astype(np.float64) == SS.coin_u(seed, draw, rows, steps)).all())
    want = u32 < np.float32(0.25)
    assert int(got.sum()) == int(want.sum()) and bool((got == want).all())
    # a fair coin: 4096 draws at 1/4 have mean 1024 and standard deviation 27.7; six of them
    assert abs(int(got.sum()) - 1024) <= 167, int(got.sum())
    assert not SS.coin(seed, draw, rows, steps, 0.0).any() and SS.coin(seed, draw, rows, steps, 1.0).all()


def test_coin_depends_on_seed_draw_row_and_step_alone():
    """not on V, not on the other rows (N, K), not on prob: one u per (seed, draw, row, step), compared with prob"""
    seed, draw, step = 9, 2, 4
    g = torch.Generator().manual_seed(1)
    nm = [9] * 6
    small = SS.mixed_step(torch.randn(6, 5, generator=g).double(), 2, 1.0, 0.5, seed, draw, step, False, [1] * 6, nm)
    large = SS.mixed_step(torch.randn(6, 37, generator=g).double(), 3, 1.0, 0.5, seed, draw, step, False, [2] * 6, nm)
    three = SS.mixed_step(torch.randn(3, 37, generator=g).double(), 1, 1.0, 0.5, seed, draw, step, True, [2] * 3, nm[:3])
    assert torch.equal(small["replaced"], large["replaced"]) and torch.equal(three["replaced"], large["replaced"][:3])
    u = SS.coin_u(seed, draw, np.arange(6), step)
    for prob in (0.1, 0.25, 0.5, 0.9):
        rep = SS.mixed_step(torch.randn(6, 5, generator=g).double(), 2, 1.0, prob, seed, draw, step, False, [1] * 6, nm)
        assert rep["replaced"].tolist() == (u < SS.fl32(prob)).tolist()
    other = [SS.coin_u(seed, draw + 1, np.arange(64), step), SS.coin_u(seed + 1, draw, np.arange(64), step),
             SS.coin_u(seed, draw, np.arange(64), step + 1)]
    base = SS.coin_u(seed, draw, np.arange(64), step)
    assert all(not (base == x).all() for x in other)


def test_mixed_step_records():
    V, R, K = 11, 6, 2
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(R, V, generator=g).double()
    gold, nmix = [3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 1, 9]
    s = SS.mixed_step(logits, K, 1.3, 0.5, 4, 0, 0, False, gold, nmix)
    p = RR.pick(logits, K, 1.3, 4, 0, 0, False)
    u = SS.coin_u(4, 0, np.arange(R), 0)
    for r in range(R):
        if nmix[r] == 0:
            assert (int(s["token"][r]), int(s["sample"][r]), float(s["logp"][r]), bool(s["replaced"][r])) == (0, -1, 0.0, False)
        elif u[r] < 0.5:
            assert int(s["token"][r]) == int(s["sample"][r]) == int(p["token"][r]) and float(s["logp"][r]) == float(p["logp"][r])
        else:
            assert (int(s["token"][r]), int(s["sample"][r]), float(s["logp"][r])) == (gold[r], -1, 0.0)
    assert s["closing"].tolist() == [False, True, False, False, True, False]
    greedy = SS.mixed_step(logits, K, 1.3, 1.0, 4, 0, 0, True, gold, [9] * R)
    assert greedy["token"].tolist() == logits.argmax(dim=1).tolist() and bool(greedy["replaced"].all())


# ---- whole runs ------------------------------------------------------------------------------------------------------------------
def _fixture(name, kind):
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    enc = t(d["enc"]).double()
    tags = t(d["tags"]).double() if kind != "pure_attention" else None
    return d, V, wm, enc, tags, params_from(d, dtype=torch.float64)


@pytest.mark.parametrize("name,kind", [BR.FIXTURES[1], BR.FIXTURES[2]])
def test_the_two_ends(name, kind):
    d, V, wm, enc, tags, P64 = _fixture(name, kind)
    gold, nmix = SS.gold_of(enc.shape[0], V)
    a = (kind, P64, 1, wm, enc, tags, gold.tolist(), nmix.tolist())
    none = SS.mix_rollout(*a, 0.0, SS.SEED, SS.DRAW, SS.INV_TEMP)
    every = SS.mix_rollout(*a, 1.0, SS.SEED, SS.DRAW, SS.INV_TEMP)
    for r, n in enumerate(nmix.tolist()):
        assert none["tokens"][r] == gold[r, :n].tolist() and not any(none["replaced"][r]) and none["sum_logp"][r] == 0.0
        assert none["sample"][r] == [-1] * n and none["logp"][r] == [0.0] * n and none["top2"][r] == []
        assert all(every["replaced"][r]) and len(every["replaced"][r]) == n and every["tokens"][r] == every["sample"][r]
        assert len(every["top2"][r]) == n
    assert none["steps"] == every["steps"] == 50


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_prob_one_is_the_rollout_until_it_ends(name, kind):
    """the same (seed, draw): the same noise, so the same words up to the rollout's first <end> or nmix"""
    d, V, wm, enc, tags, P64 = _fixture(name, kind)
    gold, nmix = SS.gold_of(enc.shape[0], V)
    mixed = SS.mix_rollout(kind, P64, 1, wm, enc, tags, gold.tolist(), nmix.tolist(), 1.0, SS.SEED, SS.DRAW, SS.INV_TEMP)
    roll = RR.rollout(kind, P64, 1, wm, enc, tags, SS.SEED, SS.DRAW, SS.INV_TEMP, False)
    compared = 0
    for r, n in enumerate(nmix.tolist()):
        m = min(n, roll["length"][r] or roll["steps"])
        assert mixed["tokens"][r][:m] == roll["tokens"][r][:m], r
        assert mixed["logp"][r][:m] == roll["logp"][r][:m], r
        compared += m
    assert compared >= 20


def test_share_of_rows_the_gpu_module_judges():
    """the caps of tests/test_gpu_rollout.py on the cases of tests/test_gpu_scheduled.py, from the CPU reference alone"""
    rows = left = 0
    for name, kind in BR.FIXTURES:
        here = out = 0
        for mix in SS.MIXES:
            case = SS.driver_case(name, kind, mix)
            here, out = here + len(case["ok"]), out + case["ok"].count(False)
            n_rep = sum(sum(x) for x in case["ref"]["replaced"])
            assert n_rep >= 20, (name, mix, n_rep)
            if mix[1] == 1.0:
                assert n_rep == int(case["nmix"].sum())
        assert 2 * out <= here, (name, out, here)
        rows, left = rows + here, left + out
    print("%d of %d rows left out" % (left, rows))
    assert rows == 90 and 4 * left <= rows


# ---- bindings, layout, refusals of the C entry points ----------------------------------------------------------------------------
def test_header_declares_the_new_symbols_and_keeps_the_version():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "scnattn.h")).read()
    from scnattn import _lib as L
    h = L.lib()
    for sym in SYMBOLS:
        assert "int %s(" % sym in header and sym in L.EXPORTS and getattr(h, sym) is not None
    assert "#define SCNATTN_VERSION 109 " in header and h.scnattn_version() == 109
    assert "#define SCNATTN_ROLLOUT_NOFF_SS %d" % L.ROLLOUT_NOFF_SS in header and L.ROLLOUT_NOFF_SS == L.ROLLOUT_NOFF + 3 == 11


def _dims(V=50, att=1):
    return (2, 4, 8, 8 if att else 0, 8, 8, 8, 3, V, 51, 51, att)


_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error().decode(), h.scnattn_last_error()


@pytest.mark.parametrize("att", (0, 1))
@pytest.mark.parametrize("want_alpha", (0, 1))
@pytest.mark.parametrize("K,T", ((1, 51), (3, 51), (8, 7)))
def test_layout_offsets_are_disjoint_and_inside_the_workspace(K, T, want_alpha, att):
    from scnattn import _lib as L
    h = L.lib()
    d = L.Dims(*_dims(att=att))
    N, P, R = 2, 4, 2 * K
    nbytes, small = C.c_size_t(), C.c_size_t()
    off, off0 = (C.c_long * L.ROLLOUT_NOFF_SS)(), (C.c_long * L.ROLLOUT_NOFF)()
    assert h.scnattn_rollout_workspace_ss(C.byref(d), K, T, want_alpha, C.byref(nbytes)) == 0
    assert h.scnattn_rollout_layout_ss(C.byref(d), K, T, want_alpha, off) == 0
    assert h.scnattn_rollout_workspace(C.byref(d), K, T, want_alpha, C.byref(small)) == 0
    assert h.scnattn_rollout_layout(C.byref(d), K, T, want_alpha, off0) == 0
    assert list(off)[:8] == list(off0)                      # the plain rollout's eight, unchanged
    sizes = [1, N, N, R, R, T * R, T * R, T * R * P, T * R, T * R, T * R]
    spans = sorted((o, o + n) for o, n in zip(off, sizes) if o >= 0)
    assert (off[7] >= 0) == bool(att and want_alpha) and len(spans) == (11 if att and want_alpha else 10)
    assert spans[0][0] >= 0 and 4 * spans[-1][1] <= nbytes.value
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    assert 4 * 3 * T * R <= nbytes.value - small.value < 4 * 3 * T * R + 3 * 256


def test_entry_points_refuse_before_launching():
    from scnattn import _lib as L
    h = L.lib()
    d, w = L.Dims(*_dims()), L.Params()
    nbytes, off = C.c_size_t(), (C.c_long * L.ROLLOUT_NOFF_SS)()
    state = (C.c_void_p * 7)(*([_P] * 7))
    for K in (0, 9):
        _refused(h, h.scnattn_rollout_workspace_ss(C.byref(d), K, 51, 0, C.byref(nbytes)), "beam_size")
        _refused(h, h.scnattn_rollout_layout_ss(C.byref(d), K, 51, 0, off), "beam_size")
        _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), K, 51, 0, C.byref(w), _P, _P, 48, _P, 51, _P, _P), "beam_size")
        _refused(h, h.scnattn_rollout_steps_ss(None, C.byref(d), K, 51, 0, C.byref(w), _P, 1.0, 0.5, 1, 0, 0, 0, 1, _P), "beam_size")
        _refused(h, h.scnattn_rollout_pick_mixed(None, 2, K, 50, _P, 50, 1.0, 0.5, 1, 0, 0, 0, 51, state, _P, _P, _P), "slot count")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _refused(h, h.scnattn_rollout_steps_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, bad, 0.5, 1, 0, 0, 0, 1, _P), "inv_temp")
        _refused(h, h.scnattn_rollout_pick_mixed(None, 2, 2, 50, _P, 50, bad, 0.5, 1, 0, 0, 0, 51, state, _P, _P, _P), "inv_temp")
    for bad in (-0.25, 1.5, float("inf"), float("nan")):
        _refused(h, h.scnattn_rollout_steps_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, 1.0, bad, 1, 0, 0, 0, 1, _P), "prob")
        _refused(h, h.scnattn_rollout_pick_mixed(None, 2, 2, 50, _P, 50, 1.0, bad, 1, 0, 0, 0, 51, state, _P, _P, _P), "prob")
    _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 50, _P, 51, _P, _P), "start token")
    _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, -1, _P, 51, _P, _P), "start token")
    _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P, 50, _P, _P), "ld_tok")
    _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, None, 51, _P, _P), "captions are NULL")
    _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P, 51, None, _P), "captions are NULL")
    _refused(h, h.scnattn_rollout_init_ss(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P, 51, _P, _P + 4), "16-byte aligned")
    _refused(h, h.scnattn_rollout_pick_mixed(None, 2, 2, 50, _P, 49, 1.0, 0.5, 1, 0, 0, 0, 51, state, _P, _P, _P), "bad argument")
    _refused(h, h.scnattn_rollout_pick_mixed(None, 2, 2, 50, _P, 50, 1.0, 0.5, 1, 0, 51, 0, 51, state, _P, _P, _P),
             "step beyond the records")
    _refused(h, h.scnattn_rollout_pick_mixed(None, 2, 2, 50, _P, 50, 1.0, 0.5, 1, 0, 0, 0, 51, None, _P, _P, _P), "state is NULL")
    for hole in range(3):
        rec = [_P, _P, _P]
        rec[hole] = None
        _refused(h, h.scnattn_rollout_pick_mixed(None, 2, 2, 50, _P, 50, 1.0, 0.5, 1, 0, 0, 0, 51, state, *rec), "record is NULL")


# ---- the refusals of the Python layers, on CPU tensors ---------------------------------------------------------------------------
def _decoders(V):
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    return [AttentionSCN(5, 4, 6, 7, 3, V, encoder_dim=8), PureSCN(4, 6, 7, 3, V, encoder_dim=8),
            PureAttention(5, 4, 6, V, encoder_dim=8)]


def _good(wm, N, per_image, L=6):
    caps = torch.zeros(N * per_image, L, dtype=torch.long)
    caps[:, 0] = wm["<start>"]
    caps[:, 1:4] = 3
    caps[:, 4] = wm["<end>"]
    return caps, torch.full((N * per_image, 1), 5, dtype=torch.long)


def test_python_refusals_come_before_the_device_check():
    V, N = 12, 2
    wm = BR.word_map(V)
    enc, tags = torch.rand(N, 2, 2, 8), torch.rand(N, 3)
    for dec in _decoders(V):
        caps, lens = _good(wm, N, 2)
        for prob in (-0.1, 1.0001, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="prob"):
                dec.mix_batch(wm, enc, tags, caps, lens, prob, per_image=2)
        for per_image in (0, 9, 2.5):
            with pytest.raises(ValueError, match="per_image"):
                dec.mix_batch(wm, enc, tags, caps, lens, 0.5, per_image=per_image)
        with pytest.raises(ValueError, match="images x"):
            dec.mix_batch(wm, enc, tags, caps, lens, 0.5)                   # per_image = 1: four rows for two images
        bad = caps.clone()
        bad[2, 0] = 3
        with pytest.raises(ValueError, match="<start>"):
            dec.mix_batch(wm, enc, tags, bad, lens, 0.5, per_image=2)
        bad = caps.clone()
        bad[1, 2] = V
        with pytest.raises(ValueError, match="outside the vocabulary"):
            dec.mix_batch(wm, enc, tags, bad, lens, 0.5, per_image=2)
        long_caps, long_lens = _good(wm, N, 2, L=60)
        long_lens[1] = 53
        with pytest.raises(ValueError, match="more than 51"):
            dec.mix_batch(wm, enc, tags, long_caps, long_lens, 0.5, per_image=2)
        for temperature in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature"):
                dec.mix_batch(wm, enc, tags, caps, lens, 0.5, per_image=2, temperature=temperature)
        for prob in (0.0, 0.5, 1.0):                                        # allowed, and goes on to the device check
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                dec.mix_batch(wm, enc, tags, caps, lens, prob, per_image=2)
    from models.decoders import _common
    per_image, nmix, prob = _common.check_mix_args(wm, N, caps, torch.tensor([[5], [2], [1], [0]]), 2, 0.1)
    assert nmix.tolist() == [3, 0, 0, 0] and per_image == 2 and prob == SS.fl32(0.1)
    from scnattn import functional as SF
    x, i = torch.zeros(1), torch.zeros(4, 51, dtype=torch.int32)
    for K in (0, 9):
        with pytest.raises(ValueError, match="K must be"):
            SF.mix_run(_dims(), K, (), x, x, 48, i, i[:, 0], 0.5, 1, 0)
    with pytest.raises(ValueError, match="inv_temp"):
        SF.mix_run(_dims(), 2, (), x, x, 48, i, i[:, 0], 0.5, 1, 0, inv_temp=0.0)
    with pytest.raises(ValueError, match="prob"):
        SF.mix_run(_dims(), 2, (), x, x, 48, i, i[:, 0], 1.5, 1, 0)
    with pytest.raises(ValueError, match="start token"):
        SF.mix_run(_dims(), 2, (), x, x, 50, i, i[:, 0], 0.5, 1, 0)
    with pytest.raises(ValueError, match="seed"):
        SF.mix_run(_dims(), 2, (), x, x, 48, i, i[:, 0], 0.5, 1, 2 ** 32)
    with pytest.raises(ValueError, match="int32"):
        SF.mix_run(_dims(), 2, (), x, x, 48, i.long(), i[:, 0], 0.5, 1, 0)
    with pytest.raises(ValueError, match="gold must be"):
        SF.mix_run(_dims(), 2, (), x, x, 48, i[:, :50], i[:, 0], 0.5, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.mix_run(_dims(), 2, (), x, x, 48, i, i[:, 0], 0.5, 1, 0)


def test_train_step_arguments():
    from trains.harness import SCSTTrainStep, TrainStep
    kw = dict(kind="pure_scn", device="cpu", encoder=False, emb_dim=4, decoder_dim=6, factored_dim=7, semantic_dim=3,
              vocab_size=12, encoder_dim=8)
    ts = TrainStep(**kw)
    assert ts.sampling_prob == 0.0 and ts.last_mix is None and ts.ss_seed == 1234 and len(ts.word_map) == 12
    ts = TrainStep(scheduled_sampling=0.25, ss_seed=9, ss_temperature=0.7, ss_greedy=True, **kw)
    assert ts.sampling_prob == 0.25 and ts.ss_seed == 9 and ts.ss_temperature == 0.7 and ts.ss_greedy
    ts.set_sampling_prob(0.1)
    assert ts.sampling_prob == SS.fl32(0.1)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="prob"):
            ts.set_sampling_prob(bad)
        with pytest.raises(ValueError, match="prob"):
            TrainStep(scheduled_sampling=bad, **kw)
    with pytest.raises(ValueError, match="temperature"):
        TrainStep(scheduled_sampling=0.25, ss_temperature=0.0, **kw)
    with pytest.raises(ValueError, match="scheduled_sampling"):
        SCSTTrainStep(scorer=type("Scorer", (), {"score_rows": None})(), scheduled_sampling=0.1, **kw)
    caps, lens = _good(BR.word_map(12), 2, 1)
    with pytest.raises(ValueError, match="prepool"):                        # a pre-pool map alone: refused before any work
        ts.step(None, torch.rand(2, 3), caps, lens, prepool=torch.rand(2, 2, 2, 8))


# ---- the staircase -----------------------------------------------------------------------------------------------------------------
def test_scheduled_sampling_prob_staircase():
    from trains.harness import scheduled_sampling_prob as ssp
    assert [ssp(e) for e in (0, 4, 5, 9, 10, 19, 20, 24, 25, 100)] == pytest.approx(
        [0.05, 0.05, 0.10, 0.10, 0.15, 0.20, 0.25, 0.25, 0.25, 0.25])
    assert [ssp(e, start=3) for e in (0, 2, 3, 7, 8)] == pytest.approx([0.0, 0.0, 0.05, 0.05, 0.10])
    assert ssp(-1) == 0.0 and ssp(2, start=3) == 0.0
    assert ssp(7, start=1, every=2, increase=0.1, max_prob=0.35) == pytest.approx(0.35)       # 0.1 * 4, capped
    assert ssp(5, start=1, every=2, increase=0.1, max_prob=0.35) == pytest.approx(0.3)
    assert all(0.0 <= ssp(e, increase=0.3, max_prob=1.0) <= 1.0 for e in range(60))
    for e in range(40):
        assert ssp(e, 2, 3, 0.04, 0.3) == (0 if e < 2 else min(0.3, 0.04 * ((e - 2) // 3 + 1)))
    with pytest.raises(ValueError):
        ssp(3, every=0)
