"""CPU tests of the references of scoring given captions (tests/scoring_refs.py), of a numpy restatement of the kernel's fp32 /
fp64 contract on every kernel case, of the bindings and the layout, of the Python refusals, of rerank's order, of the ensemble's
combination, and of the share of positions the GPU module judges, on the reference alone and for exactly its captions."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import beam_refs as BR
import ensemble_refs as ER
import scoring_cases as SC
import scoring_refs as SR
from kernel_harness import SENT, SENTI

F64 = torch.float64


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_is_log_softmax_gathered():
    g = torch.Generator().manual_seed(1)
    for V, it in ((1, 1.0), (7, 1.0 / 0.7), (300, 1.0), (1003, 0.5)):
        x = (torch.rand(9, V, generator=g, dtype=F64) * 2 - 1) * 6
        tgt = torch.randint(0, V, (9,), generator=g)
        y, logp, rank, best = SR.score_step(x, tgt, it)
        want = torch.log_softmax(x * it, dim=1).gather(1, tgt.unsqueeze(1)).squeeze(1)
        assert float((logp - want).abs().max()) <= 1e-12
        assert torch.equal(best, (x * it).argmax(dim=1))
        assert torch.equal(y, x * torch.tensor(it, dtype=F64))


def test_rank_is_the_position_in_a_stable_sort():
    g = torch.Generator().manual_seed(2)
    x = torch.floor(torch.rand(12, 40, generator=g, dtype=F64) * 5)        # ties everywhere
    x[3] = 2.0                                                              # all equal: rank is the index
    x[4, :20] = -0.0
    x[4, 20:] = 0.0
    tgt = torch.randint(0, 40, (12,), generator=g)
    _, _, rank, best = SR.score_step(x, tgt, 1.0)
    for r in range(12):
        order = torch.sort(-x[r], stable=True)[1].tolist()
        assert order.index(int(tgt[r])) == int(rank[r])
        assert order[0] == int(best[r])
        assert (int(rank[r]) == 0) == (int(best[r]) == int(tgt[r]))
    assert int(rank[3]) == int(tgt[3]) and int(rank[4]) == int(tgt[4])
    lo, hi = SR.rank_interval(x, tgt)
    assert bool((lo <= rank).all()) and bool((rank <= hi).all())


def test_infinite_logits():
    ninf = float("-inf")
    x = torch.tensor([[ninf, 0.75, ninf, ninf], [1.0, ninf, 2.0, ninf]], dtype=F64)
    _, logp, rank, best = SR.score_step(x, [1, 3], 1.0)
    assert float(logp[0]) == 0.0 and not bool(torch.signbit(logp[0])) and int(rank[0]) == 0 and int(best[0]) == 1
    assert float(logp[1]) == ninf and int(rank[1]) == 3 and int(best[1]) == 2


# ---- a numpy restatement of the kernel's arithmetic, judged like the device ----------------------------------------------
def restate(V, case):
    """What the header says the kernel does, in numpy: fp32 y and terms, the fp64 sum in the kernel's order (thread i of 256
    owns the groups of four q = i, i + 256, ...; lanes as a butterfly, then the waves 0..3), one rounding; the book-keeping."""
    N, K = case["N"], case["K"]
    R = N * K
    ntok, nsrc = case["ntok"].tolist(), case["nsrc"].tolist()
    nopen = torch.where(case["nsrc"] > 0, (case["ntok"].view(N, K) > 0).sum(dim=1).to(torch.int32), torch.zeros_like(case["nsrc"]))
    got = dict(token=torch.full((SC.STEPS, R), SENTI, dtype=torch.int32), rank=torch.full((SC.STEPS, R), SENTI, dtype=torch.int32),
               best=torch.full((SC.STEPS, R), SENTI, dtype=torch.int32),
               logp=torch.full((SC.STEPS, R), SENT, dtype=torch.int32).view(torch.float32).clone(),
               sum_logp=torch.zeros(R), nopen=nopen.clone(), nopen0=nopen, nsrc=case["nsrc"], ntok=case["ntok"],
               target=case["target"])
    open_rows = int(nopen.sum())
    it = np.float32(case["inv_temp"])
    for t in range(SC.STEPS):
        x = case["logits"][t].numpy()
        for r in range(R):
            if nsrc[r // K] == 0:
                continue
            if t >= ntok[r]:
                for k in ("token", "rank", "best"):
                    got[k][t, r] = 0
                got["logp"][t, r] = 0.0
                continue
            tgt = int(case["target"][t, r])
            y = (x[r] * it).astype(np.float32) + np.float32(0)      # -0 is taken as +0 (-0 + +0 = +0)
            m = y.max()
            with np.errstate(invalid="ignore", under="ignore"):
                e = np.where(np.isneginf(y), np.float32(0), np.exp((y - m).astype(np.float32)).astype(np.float32))
            pad = np.zeros(-V % 1024 + V, dtype=np.float64)
            pad[:V] = e
            lanes = pad.reshape(-1, 256, 4)                 # [sweep][thread][word of the group]
            acc = np.zeros(256)
            for sweep in lanes:
                for c in range(4):
                    acc = acc + sweep[:, c]
            waves = acc.reshape(4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                waves = waves + waves[:, np.arange(64) ^ o]
            S = ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]
            with np.errstate(divide="ignore"):
                lp = np.float32(np.float64(y[tgt]) - (np.float64(m) + np.log(S)))
            got["token"][t, r] = tgt
            got["logp"][t, r] = float(lp)
            got["rank"][t, r] = int(((y > y[tgt]) | ((y == y[tgt]) & (np.arange(V) < tgt))).sum())
            got["best"][t, r] = int(np.argmax(y))
            got["sum_logp"][r] = got["sum_logp"][r] + got["logp"][t, r]
            if t + 1 == ntok[r]:
                got["nopen"][r // K] -= 1
                open_rows -= 1
    got["open_rows"] = torch.tensor([open_rows])
    return got


@pytest.mark.parametrize("cfg", sorted(SC.CONFIGS))
@pytest.mark.parametrize("V", SC.VS)
def test_restatement_stays_inside_the_bound_on_every_kernel_case(V, cfg):
    total = {}
    for run in range(0, len(SC.RUNS), 1 if V < 10000 else 3):      # the load path does not enter on the host
        case = SC.gen_case(V, cfg, run)
        for k, v in SC.judge(V, case, restate(V, case), "numpy").items():
            total[k] = total.get(k, 0) + v
    N, K, closed = SC.CONFIGS[cfg]
    assert total["open"] > 0 and total["zero"] > 0 and total["closing"] > 0
    assert (total["closed_image"] > 0) == (closed is not None)
    if V < 10000:                   # the coverage the GPU module asserts, which runs every run
        assert V == 1 or total["ties"] > 0
        assert V == 1 or N * K == 1 or (total["inf"] > 0 and total["pzero"] > 0 and total["allequal"] > 0), total


def test_the_bound_is_not_slack_by_orders_of_magnitude():
    """a bound that the restatement never comes near would hide an error: somewhere it uses more than a tenth of it"""
    worst = 0.0
    for V in (257, 1025):
        for run in range(len(SC.RUNS)):
            case = SC.gen_case(V, "N3K8", run)
            got = restate(V, case)
            for t in range(SC.STEPS):
                y = SC.y32(case["logits"][t], case["inv_temp"])
                ref = SR.of_y(y.double(), case["target"][t].long())
                b = SR.logp_bound(ref)
                for r in range(24):
                    if case["nsrc"][r // 8] > 0 and t < case["ntok"][r] and torch.isfinite(ref["logp"][r]):
                        worst = max(worst, abs(float(got["logp"][t, r]) - float(ref["logp"][r])) / float(b[r]))
    assert 0.1 <= worst <= 1.0, worst


# ---- the bindings, the header, the layout ----------------------------------------------------------------------------------
SYMBOLS = ("scnattn_rollout_workspace_sc", "scnattn_rollout_layout_sc", "scnattn_rollout_init_sc", "scnattn_rollout_steps_sc",
           "scnattn_rollout_score")


def test_header_declares_the_new_symbols_and_keeps_the_version():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "scnattn.h")).read()
    from scnattn import _lib as L
    h = L.lib()
    for sym in SYMBOLS:
        assert "int %s(" % sym in header and sym in L.EXPORTS and getattr(h, sym) is not None
    assert "#define SCNATTN_VERSION 109 " in header and h.scnattn_version() == 109
    assert "#define SCNATTN_ROLLOUT_NOFF_SC %d" % L.ROLLOUT_NOFF_SC in header and L.ROLLOUT_NOFF_SC == L.ROLLOUT_NOFF + 3


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
    off, off0 = (C.c_long * L.ROLLOUT_NOFF_SC)(), (C.c_long * L.ROLLOUT_NOFF)()
    assert h.scnattn_rollout_workspace_sc(C.byref(d), K, T, want_alpha, C.byref(nbytes)) == 0
    assert h.scnattn_rollout_layout_sc(C.byref(d), K, T, want_alpha, off) == 0
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
    nbytes, off = C.c_size_t(), (C.c_long * L.ROLLOUT_NOFF_SC)()
    state = (C.c_void_p * 7)(*([_P] * 7))
    for K in (0, 9):
        _refused(h, h.scnattn_rollout_workspace_sc(C.byref(d), K, 51, 0, C.byref(nbytes)), "beam_size")
        _refused(h, h.scnattn_rollout_layout_sc(C.byref(d), K, 51, 0, off), "beam_size")
        _refused(h, h.scnattn_rollout_init_sc(None, C.byref(d), K, 51, 0, C.byref(w), _P, _P, 48, _P, 51, _P, _P), "beam_size")
        _refused(h, h.scnattn_rollout_steps_sc(None, C.byref(d), K, 51, 0, C.byref(w), _P, 1.0, 0, 1, _P), "beam_size")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _refused(h, h.scnattn_rollout_steps_sc(None, C.byref(d), 2, 51, 0, C.byref(w), _P, bad, 0, 1, _P), "inv_temp")
        _refused(h, h.scnattn_rollout_score(None, 2, 2, 50, _P, 50, bad, 0, 51, state, _P, _P, _P), "inv_temp")
    _refused(h, h.scnattn_rollout_init_sc(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 50, _P, 51, _P, _P), "start token")
    _refused(h, h.scnattn_rollout_init_sc(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P, 50, _P, _P), "ld_tok")
    _refused(h, h.scnattn_rollout_init_sc(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, None, 51, _P, _P), "captions are NULL")
    _refused(h, h.scnattn_rollout_init_sc(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P, 51, None, _P), "captions are NULL")
    _refused(h, h.scnattn_rollout_init_sc(None, C.byref(d), 2, 51, 0, C.byref(w), _P, _P, 48, _P, 51, _P, _P + 4), "16-byte aligned")
    _refused(h, h.scnattn_rollout_score(None, 2, 9, 50, _P, 50, 1.0, 0, 51, state, _P, _P, _P), "slot count")
    _refused(h, h.scnattn_rollout_score(None, 2, 2, 50, _P, 49, 1.0, 0, 51, state, _P, _P, _P), "bad argument")
    _refused(h, h.scnattn_rollout_score(None, 2, 2, 50, _P, 50, 1.0, 51, 51, state, _P, _P, _P), "step beyond the records")
    _refused(h, h.scnattn_rollout_score(None, 2, 2, 50, _P, 50, 1.0, 0, 51, None, _P, _P, _P), "state is NULL")
    _refused(h, h.scnattn_rollout_score(None, 2, 2, 50, _P, 50, 1.0, 0, 51, state, None, _P, _P), "record is NULL")


# ---- the refusals of the Python layers, on CPU tensors ---------------------------------------------------------------------
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
    from models.decoders import DecoderEnsemble
    V, N = 12, 2
    wm = BR.word_map(V)
    enc, tags = torch.zeros(N, 2, 2, 8), torch.zeros(N, 3)
    decs = _decoders(V)
    for dec in decs + [DecoderEnsemble(decs), DecoderEnsemble(decs[:1])]:
        caps, lens = _good(wm, N, 2)
        for per_image in (0, 9, -1, 2.5):
            with pytest.raises(ValueError, match="per_image"):
                dec.score_batch(wm, enc, tags, caps, lens, per_image)
        with pytest.raises(ValueError, match="images x"):              # a row count that is not N x per_image
            dec.score_batch(wm, enc, tags, caps, lens, 3)
        with pytest.raises(ValueError, match="images x"):
            dec.score_batch(wm, enc, tags, caps, lens[:3], 2)
        long_caps, long_lens = _good(wm, N, 2, L=60)
        long_lens[1] = 53                                               # caplens - 1 = 52 > 51
        with pytest.raises(ValueError, match="more than 51"):
            dec.score_batch(wm, enc, tags, long_caps, long_lens, 2)
        long_lens[1] = 52                                               # 51 tokens: allowed, and goes on to the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.score_batch(wm, enc, tags, long_caps, long_lens, 2)
        bad = caps.clone()
        bad[2, 0] = 3
        with pytest.raises(ValueError, match="<start>"):
            dec.score_batch(wm, enc, tags, bad, lens, 2)
        empty = lens.clone()
        empty[2] = 1                                                    # an empty slot need not begin with <start>
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.score_batch(wm, enc, tags, bad, empty, 2)
        for tok in (V, -1):
            bad = caps.clone()
            bad[1, 2] = tok
            with pytest.raises(ValueError, match="outside the vocabulary"):
                dec.score_batch(wm, enc, tags, bad, lens, 2)
        bad = caps.clone()
        bad[1, 5] = V                                                   # behind the caption: not scored, not checked
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.score_batch(wm, enc, tags, bad, lens, 2)
        for temperature in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="temperature"):
                dec.score_batch(wm, enc, tags, caps, lens, 2, temperature=temperature)
    from scnattn import functional as SF
    x, i = torch.zeros(1), torch.zeros(4, 51, dtype=torch.int32)
    for K in (0, 9):
        with pytest.raises(ValueError, match="K must be"):
            SF.score_run(_dims(), K, (), x, x, 48, i, i[:, 0])
    with pytest.raises(ValueError, match="inv_temp"):
        SF.score_run(_dims(), 2, (), x, x, 48, i, i[:, 0], inv_temp=0.0)
    with pytest.raises(ValueError, match="start token"):
        SF.score_run(_dims(), 2, (), x, x, 50, i, i[:, 0])
    with pytest.raises(ValueError, match="int32"):
        SF.score_run(_dims(), 2, (), x, x, 48, i.long(), i[:, 0])
    with pytest.raises(ValueError, match="targets must be"):
        SF.score_run(_dims(), 2, (), x, x, 48, i[:, :50], i[:, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.score_run(_dims(), 2, (), x, x, 48, i, i[:, 0])


# ---- rerank ----------------------------------------------------------------------------------------------------------------
def test_rerank_order_and_tie_rule():
    from scnattn.inference import rerank_order
    recs = [{"id": i, "score": s, "tokens": [0] * (n + 1)} for i, (s, n) in
            enumerate(((-6.0, 3), (-4.0, 2), (-6.0, 6), (-4.0, 2), (-9.0, 9), (-4.0, 4)))]
    ids = lambda out: [r["id"] for r in out]      # noqa: E731
    assert ids(rerank_order(recs, 0.0)) == [1, 3, 5, 0, 2, 4]          # by score; ties keep the input order
    assert ids(rerank_order(recs, 1.0)) == [2, 4, 5, 0, 1, 3]          # per token: -1, -1, -1, -2, -2, -2
    assert ids(rerank_order(recs, 0.5)) == [5, 2, 1, 3, 4, 0]          # -2, -2.45, -2.83, -2.83, -3, -3.46
    assert rerank_order([], 1.0) == [] and recs[0]["id"] == 0           # a new list; the input keeps its order
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            rerank_order(recs, bad)


# ---- the ensemble's combination --------------------------------------------------------------------------------------------
def test_ensemble_combination_is_the_reference_taken_at_one_word():
    from models.decoders.ensemble import combine_logp
    g = torch.Generator().manual_seed(3)
    logits = [(torch.rand(5, 33, generator=g, dtype=F64) * 2 - 1) * 4 for _ in range(3)]
    tgt = torch.randint(0, 33, (5, 1), generator=g)
    w = ER.member_weights([2.0, 1.0, 1.0], 3)
    ls = [l.gather(1, tgt).squeeze(1) for l in ER.log_probs(logits)]
    for mode in (0, 1):
        want = ER.combine(logits, w, mode).gather(1, tgt).squeeze(1)
        assert torch.equal(combine_logp(ls, w, mode), want)
        assert torch.equal(SR.combine_at(ls, w, mode), want)
        assert torch.equal(combine_logp(ls[:1], [1.0], mode), ls[0])
    ninf = torch.full((2,), float("-inf"), dtype=F64)
    for mode in (0, 1):
        assert bool((combine_logp([ninf, ninf], [0.5, 0.5], mode) == ninf).all())
    assert float(combine_logp([ninf[:1], torch.zeros(1, dtype=F64)], [0.5, 0.5], 1)) == pytest.approx(np.log(0.5))


# ---- the share of positions the GPU module judges, on the reference alone ------------------------------------------------
def _share(ref):
    ok = SC.rank_checked(ref)
    return sum(map(sum, ok)), sum(map(len, ok))


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_driver_captions_keep_their_share_of_judged_ranks(name, kind):
    case = SC.driver_case(name, kind)
    good, total = _share(case["ref"])
    print("%s: %d of %d positions judged; ntok %s" % (name, good, total, case["ntok"]))
    assert 4 * good >= 3 * total
    ntok, end = case["ntok"], case["wm"]["<end>"]
    assert 1 in ntok and 51 in ntok
    assert any(end not in tg for tg in case["targets"]) and any(end in tg[:-1] for tg in case["targets"])
    assert max(ntok) == case["ref"]["steps"] and all(len(x) == n for x, n in zip(case["ref"]["logp"], ntok))
    ranks = [r for row in case["ref"]["rank"] for r in row]
    assert 0 in ranks and max(ranks) > 5            # the model's own word and a foreign one both occur
