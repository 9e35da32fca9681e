"""Scoring given captions on the GPU, from the driver up (csrc/beam_search.cpp: scnattn_rollout_*_sc,
scnattn.functional.score_run, the decoders' score_batch / score_matrix, DecoderEnsemble.score_batch, Captioner.score / rerank,
trains.harness.evaluate_likelihood) against the CPU reference of tests/scoring_refs.py in fp64, against the training forward,
against the rollout's and the searches' own scores, and for what it writes.

Teacher forcing has no discrete choice, so EVERY row and position counts for logp, sum_logp and alpha; the bars are those of
the rollout and beam tests: 1e-4 * max(1, |.|), alphas within 1e-4 of the row's largest.  rank (and best) are integers that a
near-tie can move, so they are judged where the fp64 reference's gap between the target (the maximum) and its nearest
neighbour exceeds rollout_refs.band without noise; the share judged is printed and must be at least 3/4 (the captions and how
they were chosen: tests/scoring_cases.py; the same share on the CPU alone: tests/test_scoring_refs.py)."""
import pytest
import torch

import beam_refs as BR
import ensemble_refs as ER
import rollout_refs as RR
import scoring_cases as SC
import scoring_refs as SR
from helpers import params_from, t

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4
K = SC.DRIVER_K
INV_TEMP = SC.DRIVER_INV_TEMP
GUARD = 0x7FC5A5A5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def near(got, want):
    return abs(got - want) <= TOL_OUT * max(1.0, abs(want))


def as_caps(wm, targets, L=None):
    """the form `forward` takes: caps (R, L) int64 = <start>, the tokens, <pad> ...; caplens (R, 1) = tokens + 1"""
    L = L or 1 + max(len(x) for x in targets)
    caps = torch.full((len(targets), L), wm["<pad>"], dtype=torch.int64)
    caps[:, 0] = wm["<start>"]
    for r, x in enumerate(targets):
        caps[r, 1:1 + len(x)] = torch.tensor(x, dtype=torch.int64)
    return caps, torch.tensor([[len(x) + 1] for x in targets], dtype=torch.int64)


def _device(m, kind, wm, enc, tags, targets, inv_temp, dev, per_image=K, **kw):
    """SF.score_run on the captions `targets` [R][...] -> (results, steps)"""
    from models.decoders import _common
    from scnattn import functional as SF
    R = len(targets)
    tg = torch.zeros(R, SF.BEAM_MAX_STEPS, dtype=torch.int32)
    for r, x in enumerate(targets):
        tg[r, :len(x)] = torch.tensor(x, dtype=torch.int32)
    ntok = torch.tensor([len(x) for x in targets], dtype=torch.int32)
    with torch.no_grad():
        dims, weights, e, tgs = _common._search_operands(m, len(wm), enc.to(dev), None if tags is None else tags.to(dev),
                                                         kind != "pure_scn", kind != "pure_attention")
        return SF.score_run(dims, per_image, weights, e, tgs, wm["<start>"], tg.to(dev), ntok.to(dev), inv_temp=inv_temp, **kw)


def _compare(res, steps, case, use_att):
    """every row, every position -> (positions whose rank was judged, positions)"""
    ref, targets, ntok = case["ref"], case["targets"], case["ntok"]
    R = len(targets)
    lp, rank, best, tok = (res[k].cpu() for k in ("logp", "rank", "best", "tokens"))
    slp = res["sum_logp"].cpu().tolist()
    alpha = res["alpha"].cpu() if res["alpha"] is not None else None
    assert use_att == (alpha is not None)
    assert steps == max(ntok) == ref["steps"] and tuple(lp.shape) == (R, steps)
    assert res["ntok"].cpu().tolist() == ntok
    assert int(res["open_rows"]) == 0 and not bool(res["nopen"].any()) and not bool(res["nsrc"].any())
    checked = SC.rank_checked(ref)
    judged = total = 0
    for r in range(R):
        n = ntok[r]
        assert tok[r, :n].tolist() == targets[r]
        for rec in (lp, rank, best, tok):           # zero records behind the caption
            assert bool((rec[r, n:].view(torch.int32) == 0).all()), r
        assert near(slp[r], ref["sum_logp"][r]), (r, slp[r], ref["sum_logp"][r])
        for s in range(n):
            assert near(float(lp[r, s]), ref["logp"][r][s]), (r, s, float(lp[r, s]), ref["logp"][r][s])
            total += 1
            if checked[r][s]:
                judged += 1
                assert int(rank[r, s]) == ref["rank"][r][s], (r, s, int(rank[r, s]), ref["rank"][r][s])
            if ref["bgap"][r][s] > ref["band"][r][s]:
                assert int(best[r, s]) == ref["best"][r][s], (r, s)
            assert (int(rank[r, s]) == 0) == (int(best[r, s]) == targets[r][s]), (r, s)
            if use_att:
                a, b = alpha[s, r].double(), ref["alpha"][s][r].double()
                assert float((a - b).abs().max()) <= TOL_OUT * float(b.abs().max()), (r, s)
    return judged, total


# ---- (1) against the fp64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_fixture_scores_vs_reference(dev, name, kind):
    """three captions per image at temperature 0.7: random words, the model's own sample, and by image a caption of one token,
    one of 51 without <end>, one with <end> in the middle, a short one without <end>"""
    from test_gpu_parity import _build_decoder
    case = SC.driver_case(name, kind)
    m = _build_decoder(kind, case["d"], dev).eval()
    res, steps = _device(m, kind, case["wm"], case["enc"], case["tags"], case["targets"], INV_TEMP, dev, want_alpha=True)
    judged, total = _compare(res, steps, case, kind != "pure_scn")
    print("%s: rank judged at %d of %d positions (%.3f); ntok %s" % (name, judged, total, judged / total, case["ntok"]))
    assert 4 * judged >= 3 * total


@pytest.mark.parametrize("kind", ("attention_scn", "pure_scn"))
def test_vector_width_scores_vs_reference(dev, kind):
    """E=256, A=128, D=F=128, M=64, S=40, 7x7, V=1003, N=3: the 16-byte paths of the attention kernels; ld = V = 1003 is the
    scoring kernel's scalar path (its vector path: tests/test_gpu_scoring_kernels.py)"""
    from test_gpu_parity import _build_decoder
    case = SC.vector_case(kind)
    m = _build_decoder(kind, case["d"], dev).eval()
    res, steps = _device(m, kind, case["wm"], case["enc"], case["tags"], case["targets"], 1.0, dev, want_alpha=True)
    judged, total = _compare(res, steps, case, kind != "pure_scn")
    print("%s: rank judged at %d of %d positions (%.3f); ntok %s" % (kind, judged, total, judged / total, case["ntok"]))
    assert 4 * judged >= 3 * total


# ---- (2) against the training forward: scoring is what training optimises -------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_score_batch_vs_the_training_forward(dev, name, kind):
    from test_gpu_parity import _build_decoder
    case = SC.driver_case(name, kind)
    wm, enc, tags = case["wm"], case["enc"], case["tags"]
    m = _build_decoder(kind, case["d"], dev).eval()
    caps, caplens = as_caps(wm, case["targets"])
    with torch.no_grad():
        out = m.score_batch(wm, enc.to(dev), None if tags is None else tags.to(dev), caps.to(dev), caplens.to(dev),
                            per_image=K, temperature=1.0 / INV_TEMP)
    assert tuple(out["logp"].shape) == (len(caps), caps.shape[1] - 1) and out["logp"].is_cuda
    assert out["rank"].dtype == torch.int32 and out["best"].dtype == torch.int32 and out["n_tokens"].dtype == torch.int32
    assert out["n_tokens"].cpu().tolist() == case["ntok"] and out["alpha"] is None
    P64 = params_from(case["d"], dtype=torch.float64)
    slp = out["sum_logp"].cpu().tolist()
    for r, x in enumerate(case["targets"]):
        n = r // K
        want = RR.teacher_forced_logp(kind, P64, [wm["<start>"]] + x, enc[n:n + 1].double(),
                                      None if tags is None else tags[n:n + 1].double(), INV_TEMP)
        assert near(slp[r], want), (r, slp[r], want)
        assert near(slp[r], float(out["logp"][r].double().sum())), r


# ---- (3) round trip: the rollout's sum_logp is the score of its own captions ----------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_round_trip_with_the_rollout(dev, name, kind):
    import test_gpu_rollout as TR
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    enc = t(d["enc"])
    tags = t(d["tags"]) if kind != "pure_attention" else None
    m = _build_decoder(kind, d, dev).eval()
    seed, draw = 11, 3
    e, tg = enc.to(dev), None if tags is None else tags.to(dev)
    with torch.no_grad():
        caps, caplens, sum_logp = m.rollout_batch(wm, e, tg, samples=2, seed=seed, draw=draw, temperature=0.7,
                                                  greedy_first=True)
        out = m.score_batch(wm, e, tg, caps, caplens, per_image=3, temperature=0.7)
    roll, _ = TR._device(m, kind, wm, enc, tags, 3, seed, draw, TR.INV_TEMP, True, dev, want_alpha=False)
    n_tok = (caplens.view(-1) - 1).cpu().tolist()
    targets = [caps[r, 1:1 + n].cpu().tolist() for r, n in enumerate(n_tok)]
    assert out["n_tokens"].cpu().tolist() == n_tok
    # the magnitudes both kernels' bounds need, from the fp64 reference on the same tokens
    ref = SR.score(kind, params_from(d, dtype=torch.float64), 3, wm, enc.double(), None if tags is None else tags.double(),
                   targets, n_tok, TR.INV_TEMP)
    got, want, rank, best = out["logp"].cpu(), roll["logp"].cpu(), out["rank"].cpu(), out["best"].cpu()
    worst = 0.0
    for r, n in enumerate(n_tok):
        assert roll["tokens"][r, :n].cpu().tolist() == targets[r]
        for s in range(n):
            bound = ref["bound_score"][r][s] + ref["bound_pick"][r][s]
            err = abs(float(got[r, s]) - float(want[r, s]))
            worst = max(worst, err / bound)
            assert err <= bound, (r, s, float(got[r, s]), float(want[r, s]), bound)
        if r % 3 == 0:                  # the arg-max slot: every token was the model's own first word
            assert best[r, :n].tolist() == targets[r] and not bool(rank[r, :n].any()), r
        assert near(float(out["sum_logp"][r]), float(sum_logp[r])), r
    print("%s: worst |score - rollout| / (sum of the two bounds) %.3f over %d tokens" % (name, worst, sum(n_tok)))


# ---- (4) the beam search's score of its best caption ----------------------------------------------------------------------
_BEAMS = {}


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_score_of_the_best_beam(dev, name, kind):
    from models.decoders import _common
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    with torch.no_grad():
        beams = _common.beam_search_batched(m, 3, wm, enc, tags, use_att, use_tags, return_all=True)
    compared = 0
    for n, (res, done) in enumerate(beams):
        seq = res[0] if use_att else res
        scores = [s for q, s in done if list(q) == list(seq)]
        if not scores:                  # nothing completed: the search fell back to an open beam and reports no score
            continue
        caps, caplens = as_caps(wm, [list(seq)[1:]])
        with torch.no_grad():
            out = m.score_batch(wm, enc[n:n + 1], None if tags is None else tags[n:n + 1], caps.to(dev), caplens.to(dev),
                                per_image=1)
        assert near(float(out["sum_logp"][0]), max(scores)), (n, float(out["sum_logp"][0]), scores)
        compared += 1
    print("%s: %d of %d images compared" % (name, compared, len(beams)))
    _BEAMS[name] = compared
    if len(_BEAMS) == len(BR.FIXTURES):
        assert sum(_BEAMS.values()) >= 8, _BEAMS


# ---- (5) ragged input -------------------------------------------------------------------------------------------------------
def _bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("name,kind", [BR.FIXTURES[0], BR.FIXTURES[2]])
def test_ragged_input(dev, name, kind):
    from test_gpu_parity import _build_decoder
    case = SC.driver_case(name, kind)
    wm, targets = case["wm"], case["targets"]
    m = _build_decoder(kind, case["d"], dev).eval()
    enc = case["enc"].to(dev)
    tags = None if case["tags"] is None else case["tags"].to(dev)
    caps, caplens = as_caps(wm, targets)
    keys = ("logp", "rank", "best", "sum_logp", "n_tokens")

    def run(lens):
        with torch.no_grad():
            return m.score_batch(wm, enc, tags, caps.to(dev), lens.to(dev), per_image=K)

    full = run(caplens)
    longest = max(range(len(targets)), key=lambda r: len(targets[r]))
    for emptied in ([2 * K + 1], [longest], [K, K + 1, K + 2], list(range(len(targets)))):      # a slot; ...; image 1; all
        lens = caplens.clone()
        lens[torch.tensor(emptied)] = 1
        lens[emptied[0]] = 0                    # 0 and 1 both mark an empty slot
        got = run(lens)
        for r in range(len(targets)):
            for k in keys:
                if r in emptied:
                    assert not bool(_bits(got[k][r]).any()), (emptied, r, k)
                else:
                    assert torch.equal(_bits(got[k][r]), _bits(full[k][r])), (emptied, r, k)
    # steps is the longest caption that is left
    most = len(targets[longest])
    rest = [x if len(x) < most else [] for x in targets]
    _, steps = _device(m, kind, wm, case["enc"], case["tags"], rest, 1.0, dev)
    assert steps == max(len(x) for x in rest) and 0 < steps < most
    res, steps = _device(m, kind, wm, case["enc"], case["tags"], [[] for _ in targets], 1.0, dev)
    assert steps == 0 and tuple(res["logp"].shape) == (len(targets), 0) and not bool(res["sum_logp"].any())


# ---- (6) driver mechanics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [BR.FIXTURES[0], BR.FIXTURES[2]])
def test_chunks_guard_band_and_repeats(dev, name, kind):
    from test_gpu_parity import _build_decoder
    case = SC.driver_case(name, kind)
    m = _build_decoder(kind, case["d"], dev).eval()
    args = (m, kind, case["wm"], case["enc"], case["tags"], case["targets"], INV_TEMP, dev)
    keys = ("logp", "rank", "best", "tokens", "sum_logp", "ntok", "alpha")
    for want_alpha in (False, True):
        a, steps = _device(*args, want_alpha=want_alpha, guard=4096, chunk=8)
        a = {k: None if a[k] is None else a[k].clone() for k in keys + ("guard",)}
        assert bool((a["guard"] == GUARD).all()), "words behind the workspace were overwritten"
        assert (a["alpha"] is not None) == (want_alpha and kind != "pure_scn")
        for chunk in (1, 8):                    # another chunking, and the same call again: equal bits
            b, steps_b = _device(*args, want_alpha=want_alpha, guard=4096, chunk=chunk)
            assert steps_b == steps and bool((b["guard"] == GUARD).all())
            for k in keys:
                assert (a[k] is None and b[k] is None) or torch.equal(_bits(a[k]), _bits(b[k])), (want_alpha, chunk, k)


# ---- (7) the ensemble -----------------------------------------------------------------------------------------------------------
def test_one_member_ensemble_is_the_decoder_bit_for_bit(dev):
    from models.decoders import DecoderEnsemble
    from test_gpu_parity import _build_decoder
    name, kind = BR.FIXTURES[0]
    case = SC.driver_case(name, kind)
    m = _build_decoder(kind, case["d"], dev).eval()
    ens = DecoderEnsemble([m]).to(dev).eval()
    caps, caplens = as_caps(case["wm"], case["targets"])
    a = (case["wm"], case["enc"].to(dev), case["tags"].to(dev), caps.to(dev), caplens.to(dev), K)
    with torch.no_grad():
        one, two = m.score_batch(*a, want_alpha=True), ens.score_batch(*a, want_alpha=True)
    assert sorted(one) == sorted(two) == ["alpha", "best", "logp", "n_tokens", "rank", "sum_logp"]
    for k in one:
        assert torch.equal(_bits(one[k]), _bits(two[k])), k


ENS_SEED, ENS_KINDS, ENS_WEIGHTS = 3, ("attention_scn", "pure_scn"), (2.0, 1.0)


def _ensemble_case():
    g = torch.Generator().manual_seed(ENS_SEED)
    dicts = []
    for kind in ENS_KINDS:
        d, V, E, S = ER.uniform_params(kind, g)
        dicts.append(d)
    enc, tags = torch.rand(3, 7, 7, E, generator=g), torch.rand(3, S, generator=g)
    for d in dicts:
        d["p.fc.bias"][V - 1] += ER.END_BIAS
    return dicts, V, enc, tags


@pytest.mark.parametrize("mode", ("logprob", "prob"))
def test_two_member_ensemble_vs_fp64(dev, mode):
    """the fp64 combination of the members' fp64 logp, and the ensemble search's score of its own best caption"""
    from models.decoders import DecoderEnsemble
    from test_gpu_parity import _build_decoder
    dicts, V, enc, tags = _ensemble_case()
    wm = BR.word_map(V)
    ens = DecoderEnsemble([_build_decoder(k, d, dev) for k, d in zip(ENS_KINDS, dicts)], weights=ENS_WEIGHTS,
                          combine=mode).to(dev).eval()
    w = ER.member_weights(ENS_WEIGHTS, 2)
    g = torch.Generator().manual_seed(77)
    targets = [torch.randint(1, V - 3, (int(torch.randint(1, 9, (1,), generator=g)),), generator=g).tolist() + [V - 1]
               for _ in range(6)]
    caps, caplens = as_caps(wm, targets)
    e, tg = enc.to(dev), tags.to(dev)
    with torch.no_grad():
        out = ens.score_batch(wm, e, tg, caps.to(dev), caplens.to(dev), per_image=2, want_alpha=True)
    assert out["rank"] is None and out["best"] is None and out["alpha"] is not None
    refs = [SR.score(k, params_from(d, dtype=torch.float64), 2, wm, enc.double(), tags.double(), targets,
                     [len(x) for x in targets]) for k, d in zip(ENS_KINDS, dicts)]
    lp = out["logp"].cpu()
    for r, x in enumerate(targets):
        want = SR.combine_at([torch.tensor(ref["logp"][r], dtype=torch.float64) for ref in refs], w, ER.MODES[mode])
        for s in range(len(x)):
            assert near(float(lp[r, s]), float(want[s])), (r, s, float(lp[r, s]), float(want[s]))
        assert not bool(lp[r, len(x):].any())
        assert near(float(out["sum_logp"][r]), float(want.sum())), r
    # the search's own best caption
    with torch.no_grad():
        found = ens.sample_batch(3, wm, e, tg, return_all=True)
    compared = 0
    for n, (res, done) in enumerate(found):
        seq = list(res[0])
        scores = [s for q, s in done if list(q) == seq]
        if not scores:
            continue
        caps, caplens = as_caps(wm, [seq[1:]])
        with torch.no_grad():
            one = ens.score_batch(wm, e[n:n + 1], tg[n:n + 1], caps.to(dev), caplens.to(dev), per_image=1)
        assert near(float(one["sum_logp"][0]), max(scores)), (n, float(one["sum_logp"][0]), scores)
        compared += 1
    print("%s: %d of %d images compared with the ensemble search" % (mode, compared, len(found)))
    assert compared >= 2


# ---- (8) the application layer ----------------------------------------------------------------------------------------------------
def test_score_matrix_equals_the_single_calls(dev):
    from test_gpu_parity import _build_decoder
    name, kind = BR.FIXTURES[1]
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    enc, tags = t(d["enc"])[:3].to(dev), t(d["tags"])[:3].to(dev)
    g = torch.Generator().manual_seed(5)
    targets = [torch.randint(1, V - 3, (int(torch.randint(1, 7, (1,), generator=g)),), generator=g).tolist() + [V - 1]
               for _ in range(10)]
    caps, caplens = as_caps(wm, targets)
    with torch.no_grad():
        got = m.score_matrix(wm, enc, tags, caps.to(dev), caplens.to(dev))
        assert tuple(got.shape) == (3, 10) and got.is_cuda
        for q in range(10):
            one = m.score_batch(wm, enc, tags, caps[q:q + 1].repeat(3, 1).to(dev), caplens[q:q + 1].repeat(3, 1).to(dev), 1)
            for n in range(3):
                assert near(float(got[n, q]), float(one["sum_logp"][n])), (n, q)
    assert len({round(float(x), 4) for x in got[:, 0]}) == 3        # the images differ


def test_captioner_score_and_rerank(dev):
    import test_gpu_captioner as TC
    from scnattn.inference import Captioner
    wm = BR.word_map(TC.V)
    enc, tag, dec = TC._modules("attention_scn", dev)
    cap = Captioner(enc, dec, wm, tagger=tag)
    images = TC._images()[:2]
    g = torch.Generator().manual_seed(8)
    nine = [torch.randint(1, TC.V - 3, (int(torch.randint(1, 6, (1,), generator=g)),), generator=g).tolist() + [wm["<end>"]]
            for _ in range(9)]
    nine[3] = [wm["<start>"]] + nine[3]                                 # a leading <start> is not doubled
    words = [["w1", "w2", "no-such-word"], ["w3", "<end>"]]             # <unk>; <end> appended, or kept
    calls, passes = [], []
    orig = dec.score_batch
    dec.score_batch = lambda *a, **kw: (calls.append(kw.get("per_image")), orig(*a, **kw))[1]
    hook = enc.register_forward_hook(lambda mod, i, o: passes.append(1))
    try:
        recs = cap.score(images, [nine, words])
        ranked = cap.rerank(images, [nine, words], length_penalty=1.0)
    finally:
        hook.remove()
        del dec.score_batch
    assert calls == [8, 1, 8, 1] and len(passes) == 2                   # two calls over ONE encoder pass, each time
    assert [len(r) for r in recs] == [9, 2]
    assert recs[1][0]["tokens"] == [wm["<start>"], 1, 2, wm["<unk>"], wm["<end>"]] and recs[1][0]["words"] == ["w1", "w2", "<unk>"]
    assert recs[1][1]["tokens"] == [wm["<start>"], 3, wm["<end>"]] and recs[0][3]["tokens"] == nine[3]
    for n, per_image in enumerate(recs):
        for j, rec in enumerate(per_image):
            nt = len(rec["tokens"]) - 1
            assert set(rec) == {"tokens", "words", "logp", "score", "per_token", "rank"}
            assert len(rec["logp"]) == len(rec["rank"]) == nt and near(rec["score"], sum(rec["logp"]))
            assert rec["per_token"] == rec["score"] / nt and all(0 <= x < TC.V for x in rec["rank"])
            alone = cap.score(images[n:n + 1], [[rec["tokens"]]])[0][0]
            assert near(alone["score"], rec["score"]) and alone["tokens"] == rec["tokens"], (n, j)
    for n, per_image in enumerate(ranked):
        keys = [r["per_token"] for r in per_image]
        assert keys == sorted(keys, reverse=True) and sorted(r["score"] for r in per_image) == sorted(r["score"] for r in recs[n])
    with pytest.raises(ValueError):
        cap.score(images, [nine])
    with pytest.raises(ValueError):
        cap.score(images, [[[]], []])
    with pytest.raises(ValueError):
        cap.score(images, [[[TC.V]], []])


def test_evaluate_likelihood_equals_the_perplexity_by_hand(dev):
    import math
    import test_gpu_caption_metrics_step as S
    from models.decoders.attention_scn import AttentionSCN
    from trains.harness import evaluate_likelihood
    V, B, Q, L = 30, 4, 5, 9
    wm = BR.word_map(V)
    torch.manual_seed(9)
    dec = AttentionSCN(24, 20, 28, 36, 14, V, encoder_dim=40, dropout=0.5).to(dev)
    g = torch.Generator().manual_seed(10)
    batches = []
    for _ in range(2):
        allcaps = torch.zeros(B, Q, L, dtype=torch.long)
        for b in range(B):
            for q in range(Q):
                n = int(torch.randint(3, L + 1, (1,), generator=g))
                allcaps[b, q, 0] = wm["<start>"]
                allcaps[b, q, 1:n - 1] = torch.randint(1, V - 3, (n - 2,), generator=g)
                allcaps[b, q, n - 1] = wm["<end>"]
        allcaps[1, 4] = 0                                               # image 1 has four references only
        imgs = (torch.rand(B, 2, 2, 40, generator=g).to(dev), torch.rand(B, 14, generator=g).to(dev))
        batches.append((imgs, allcaps.to(dev)))
    got = evaluate_likelihood(S._Encoder(), dec, batches, wm, tagger=lambda im: im[1])
    assert not dec.training
    total, n_tok, hits1, hits5, ranks, n_cap = 0.0, 0, 0, 0, 0, 0
    for imgs, allcaps in batches:
        lens = (allcaps != 0).sum(dim=2)
        with torch.no_grad():
            out = dec.score_batch(wm, imgs[0], imgs[1], allcaps.reshape(B * Q, L), lens.reshape(B * Q, 1), per_image=Q)
        nt = out["n_tokens"].cpu().long()
        given = torch.arange(L - 1).unsqueeze(0) < nt.unsqueeze(1)
        total += float(out["logp"].cpu().double()[given].sum())
        n_tok += int(nt.sum())
        n_cap += int((nt > 0).sum())
        rank = out["rank"].cpu()[given]
        hits1, hits5, ranks = hits1 + int((rank == 0).sum()), hits5 + int((rank < 5).sum()), ranks + int(rank.sum())
    assert got["n_tokens"] == n_tok and got["n_captions"] == n_cap == 2 * (B * Q - 1)
    assert got["perplexity"] == pytest.approx(math.exp(-total / n_tok), rel=1e-12)
    assert got["top1"] == pytest.approx(100.0 * hits1 / n_tok) and got["top5"] == pytest.approx(100.0 * hits5 / n_tok)
    assert got["mean_rank"] == pytest.approx(ranks / n_tok) and 1.0 < got["perplexity"] < 10 * V
