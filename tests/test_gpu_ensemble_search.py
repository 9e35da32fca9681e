"""DecoderEnsemble.sample_batch -- M decoders under one beam search on the GPU (csrc/beam_search.cpp: scnattn_ensemble_*) --
against the single-decoder search bit for bit, against the fp64 reference of tests/ensemble_refs.py, and for the shape of
what it returns.

Against fp64 a case (table, mode, image, beam size) is compared under the decidability rule of
tests/test_gpu_beam_search.py: beam_refs.decidable on the fp64 and fp32 traces of ensemble_refs.search, both from the CPU
alone.  Bars: sequences equal, completed lists equal in order, scores within 1e-4 * max(1, |s|), alphas within 1e-4 (that
file's bars).  Caps, asserted: at most 1/4 of all cases and at most 1/2 of any table left out."""
import pytest
import torch

import beam_refs as BR
import ensemble_refs as ER
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


def _ensemble(dev, members, **kw):
    from models.decoders import DecoderEnsemble
    return DecoderEnsemble(members, **kw).to(dev).eval()


# ---- (a) one member, and the same member twice, are the single search bit for bit -------------------------------------
@pytest.mark.parametrize("name,kind", [f for f in BR.FIXTURES if f[0].endswith("_distinct")])
def test_one_member_is_sample_batch_bit_for_bit(dev, name, kind):
    """sequences, completed lists, scores and alphas EQUAL (no tolerance): [d] and [d, d] with weights (.5, .5)"""
    from models.decoders import _common
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    one, two = _ensemble(dev, [m]), _ensemble(dev, [m, m], weights=[.5, .5])
    for k in BR.BEAMS:
        with torch.no_grad():
            want = _common.beam_search_batched(m, k, wm, enc, tags, use_attention=use_att, use_tags=use_tags, return_all=True)
            pub = m.sample_batch(k, wm, enc, tags) if use_tags else m.sample_batch(k, wm, enc)
            for ens in (one, two):
                got = ens.sample_batch(k, wm, enc, tags, return_all=True)
                assert got == want, (k, len(ens.decoders))
                assert ens.sample_batch(k, wm, enc, tags) == pub, (k, len(ens.decoders))
        assert all(len(done) >= 1 for _, done in want)


# ---- (b) against the fp64 reference -----------------------------------------------------------------------------------
# Seeds picked on the CPU reference alone (ensemble_refs.table; weights (0.625, 0.375) for A+S, (0.5, 0.25, 0.25) for A+S+P):
#   3, A+S    logprob: chosen lengths 3-11, searches of 2 .. 15 steps and one that uses all 51 with completed beams behind it;
#             prob: chosen lengths 3-18, up to 28 steps and all 51
#   3, A+S+P  logprob: one image (k = 1) with nothing completed in 51 steps -- the fallback path; prob: lengths 2-5
#   6, A+S    chosen lengths 2-8 (logprob) and 2-13 (prob), 1 .. 17 steps
# none leaves a case out: 0 of 54.
TABLES = [(3, "A+S"), (3, "A+S+P"), (6, "A+S")]
_LEFT = {}


def _check(got, ref, has_alpha, where):
    one, done = got
    seq = one[0] if has_alpha else one
    assert seq == ref.seq, (where, seq, ref.seq)
    if not ref.completed:           # nothing completed: the best open beam, as the reference's fallback
        assert len(seq) == BR.MAX_STEPS + 1 and seq[0] == ref.seq[0]
    assert [s for s, _ in done] == [s for s, _ in ref.done], where
    for (_, sg), (_, sr) in zip(done, ref.done):
        assert abs(sg - sr) <= 1e-4 * max(1.0, abs(sr)), (where, sg, sr)
    if has_alpha:
        a, r = torch.tensor(one[1]).double(), torch.tensor(ref.alphas).double()
        assert a.shape == r.shape and float((a - r).abs().max()) <= TOL_OUT * float(r.abs().max()), where


@pytest.mark.parametrize("seed,name", TABLES)
@pytest.mark.parametrize("mode", ["logprob", "prob"])
def test_ensemble_vs_fp64(dev, seed, name, mode):
    """E=256, A=128, D=F=128, M=64, S=40, 7x7, V=1003, N=3, k in {1, 3, 5}: the batch of three images, and image by image
    -- the results must be IDENTICAL, a finished image's kernels being no-ops"""
    from test_gpu_parity import _build_decoder
    T = ER.table(seed, name)
    wm = BR.word_map(T["V"])
    members = [_build_decoder(kind, d, dev) for kind, d in zip(T["kinds"], T["dicts"])]
    ens = _ensemble(dev, members, weights=T["weights"], combine=mode)
    assert ens.member_weights == T["w"] and ens.alpha_member == 0
    enc, tags = T["enc"].to(dev), T["tags"].to(dev)
    N, left, total = enc.shape[0], 0, 0
    for k in BR.BEAMS:
        with torch.no_grad():
            got = ens.sample_batch(k, wm, enc, tags, return_all=True)
            alone = [ens.sample_batch(k, wm, enc[b:b + 1], tags[b:b + 1], return_all=True)[0] for b in range(N)]
        assert len(got) == N and got == alone, k
        for b in range(N):
            ref, ok = T["cases"][(ER.MODES[mode], b, k)]
            total += 1
            if not ok:
                left += 1
                continue
            _check(got[b], ref, True, (seed, name, mode, b, k))
    print("%d %s %s: %d of %d cases left out" % (seed, name, mode, left, total))
    assert total == 9 and 2 * left <= total
    _LEFT[(seed, name, mode)] = left
    if len(_LEFT) == 2 * len(TABLES):
        assert 4 * sum(_LEFT.values()) <= 9 * len(_LEFT), _LEFT


def test_decidable_counts_on_the_cpu():
    """the caps, where the rule is computed (no device needed for this part)"""
    left = {(seed, name, mode): sum(1 for (md, _, _), (_, ok) in ER.table(seed, name)["cases"].items() if md == mode and not ok)
            for seed, name in TABLES for mode in (0, 1)}
    assert all(2 * v <= 9 for v in left.values()) and 4 * sum(left.values()) <= 54, left


# ---- (c) the shape of the result ----------------------------------------------------------------------------------------
def test_members_without_attention_return_plain_sequences(dev):
    from test_gpu_parity import _build_decoder
    g = torch.Generator().manual_seed(5)
    dicts = []
    for _ in range(2):
        d, V, E, S = ER.uniform_params("pure_scn", g)
        d["p.fc.bias"][V - 1] += ER.END_BIAS
        dicts.append(d)
    enc, tags = torch.rand(2, 7, 7, E, generator=g).to(dev), torch.rand(2, S, generator=g).to(dev)
    ens = _ensemble(dev, [_build_decoder("pure_scn", d, dev) for d in dicts])
    assert ens.alpha_member is None and not ens.has_alphas
    wm = BR.word_map(V)
    with torch.no_grad():
        got = ens.sample_batch(3, wm, enc, tags)
        both = ens.sample_batch(3, wm, enc, tags, return_all=True)
    assert len(got) == 2 and all(isinstance(s, list) and s[0] == wm["<start>"] and all(isinstance(x, int) for x in s) for s in got)
    assert [one for one, _ in both] == got and all(isinstance(done, list) and done for _, done in both)


def test_alpha_member_selects_the_second_attention_member(dev):
    """A+S+P at seed 3 with alpha_member = 2: the maps are PureAttention's, checked against the reference's"""
    from helpers import params_from
    from test_gpu_parity import _build_decoder
    T = ER.table(3, "A+S+P")
    wm = BR.word_map(T["V"])
    members = [_build_decoder(kind, d, dev) for kind, d in zip(T["kinds"], T["dicts"])]
    ens = _ensemble(dev, members, weights=T["weights"], combine="prob", alpha_member=2)
    P64 = [params_from(d, dtype=torch.float64) for d in T["dicts"]]
    k, b = 3, 1
    assert T["cases"][(1, b, k)][1], "picked as a decidable case"
    enc, tags = T["enc"][b:b + 1], T["tags"][b:b + 1]
    ref = ER.search(T["kinds"], P64, T["w"], 1, k, wm, enc.double(), tags.double(), alpha_member=2)
    first = T["cases"][(1, b, k)][0]
    assert ref.seq == first.seq and ref.alphas != first.alphas
    with torch.no_grad():
        got, = ens.sample_batch(k, wm, enc.to(dev), tags.to(dev), return_all=True)
    _check(got, ref, True, "alpha_member = 2")
    a0 = torch.tensor(first.alphas).double()
    assert float((torch.tensor(got[0][1]).double() - a0).abs().max()) > 10 * TOL_OUT      # not the first member's maps


def test_workspace_guard_band_and_refusals_of_the_driver(dev):
    """nothing is written behind the ensemble's workspace (three members, the maps of the third); members that disagree in
    V, and an alpha_member that is no member, are refused before anything is launched"""
    from models.decoders import _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    T = ER.table(3, "A+S+P")
    V = T["V"]
    members = [_build_decoder(kind, d, dev).eval() for kind, d in zip(T["kinds"], T["dicts"])]
    enc4, tags = T["enc"].to(dev), T["tags"].to(dev)
    ops = [_common._search_operands(m, V, enc4, tags if kind != "pure_attention" else None, kind != "pure_scn",
                                    kind != "pure_attention") for m, kind in zip(members, T["kinds"])]
    dims, weights, tg = [o[0] for o in ops], [o[1] for o in ops], [o[3] for o in ops]
    res, steps = SF.ensemble_search_run(dims, 5, weights, ops[0][2], tg, T["weights"], "prob", V - 2, V - 1, 2, guard=4096)
    assert steps >= 1 and bool((res["guard"] == 0x7FC5A5A5).all()), "words behind the workspace were overwritten"
    assert bool((res["nsrc"] == res["kk"]).all()) and int(res["open_images"]) == int((res["kk"] > 0).sum())
    assert bool((res["ncomp"] + res["kk"] == 5).all()) and res["alpha"].shape == (steps, 15, 49)
    for a in (res["scores"], res["comp_score"], res["best_score"], res["alpha"]):
        assert bool(torch.isfinite(a).all())
    none, _ = SF.ensemble_search_run(dims, 5, weights, ops[0][2], tg, T["weights"], "prob", V - 2, V - 1, -1)
    assert none["alpha"] is None and torch.equal(none["token"], res["token"])
    bad = [tuple(dims[0]), tuple(dims[1][:8]) + (V - 1,) + tuple(dims[1][9:])]
    with pytest.raises(ValueError):
        SF.ensemble_search_run(bad, 5, weights[:2], ops[0][2], tg[:2], None, 0, V - 2, V - 2, None)
    with pytest.raises(ValueError):
        SF.ensemble_search_run(dims, 5, weights, ops[0][2], tg, None, 0, V - 2, V - 1, 3)
    from scnattn._lib import Dims
    import ctypes as C
    d = (Dims * 2)(Dims(*bad[0]), Dims(*bad[1]))
    nbytes = C.c_size_t()
    with pytest.raises(RuntimeError, match="agree"):
        SF.call("scnattn_ensemble_workspace", 2, d, 5, 51, -1, C.byref(nbytes))


# ---- (d) wherever a decoder is taken ------------------------------------------------------------------------------------
def test_captioner_and_evaluate_captions_take_an_ensemble(dev):
    import test_gpu_caption_metrics_step as S
    import test_gpu_captioner as TC
    from scnattn.inference import Captioner
    from trains.harness import evaluate_captions
    wm = BR.word_map(TC.V)
    torch.manual_seed(4)
    enc, tag = TC.TinyEncoder().to(dev), TC.TinyTagger().to(dev)
    ens = _ensemble(dev, [TC._decoder(kind).to(dev) for kind in TC.KINDS])
    with pytest.raises(ValueError):
        Captioner(enc, ens, wm)                         # a member uses tags: a tagger is needed
    records = Captioner(enc, ens, wm, tagger=tag, beam_size=3)(TC._images(), tag_count=2)
    assert len(records) == 4
    for rec in records:
        assert set(rec) >= {"tokens", "words", "alphas", "tags"} and rec["tokens"][0] == wm["<start>"]
        assert len(rec["alphas"]) == len(rec["tokens"]) and len(rec["tags"][0]) == 2
        assert all(w not in ("<start>", "<end>", "<pad>") for w in rec["words"])
    # evaluate_captions: the ensemble of the three kinds at that test's small dimensions
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    V, B, R, L = 30, 4, 3, 9
    wm = BR.word_map(V)
    torch.manual_seed(9)
    ens = _ensemble(dev, [AttentionSCN(24, 20, 28, 36, 14, V, encoder_dim=40, dropout=0.5),
                          PureSCN(20, 28, 36, 14, V, encoder_dim=40, dropout=0.5),
                          PureAttention(24, 20, 28, V, encoder_dim=40, dropout=0.5)], combine="prob")
    g = torch.Generator().manual_seed(10)
    allcaps = torch.zeros(B, R, L, dtype=torch.long)
    for b in range(B):
        for r in range(R):
            n = int(torch.randint(3, L + 1, (1,), generator=g))
            allcaps[b, r, 0] = wm["<start>"]
            allcaps[b, r, 1:n - 1] = torch.randint(1, 8, (n - 2,), generator=g)
            allcaps[b, r, n - 1] = wm["<end>"]
    imgs = (torch.rand(B, 2, 2, 40, generator=g).to(dev), torch.rand(B, 14, generator=g).to(dev))
    got = evaluate_captions([(imgs, allcaps.to(dev))], S._Encoder(), lambda im: im[1], ens, wm, beam_size=3)
    assert {"Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr"} <= set(got) and all(0.0 <= float(got[k]) for k in ("Bleu_1", "ROUGE_L", "CIDEr"))
