"""sample_batch(..., options=SearchOptions(...)) -- n-gram blocking, a minimum length and banned tokens inside the GPU search,
a length penalty when the results are read -- against the fp64 restatement of tests/beam_options_refs.py.

The reference project has no such options; the restatement is the yardstick.  A case is compared under the decidability
rule of tests/test_gpu_beam_search.py (beam_refs.decidable on the restatement's fp64 and fp32 traces, the candidates taken
AFTER exclusion), with that file's bars: sequences equal, scores within 1e-4 * max(1, |s|), alphas within 1e-4.  Caps,
asserted here and, from the restatement alone, in tests/test_beam_options_refs.py: at most 1/4 of a table's cases left out,
and in every table at least 3 compared cases whose caption the n-gram rule changes -- a kernel that ignored the history
would fail them."""
import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
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


def _so(o):
    from models.decoders import SearchOptions
    return SearchOptions(min_length=o.min_length, no_repeat_ngram=o.no_repeat_ngram, banned_tokens=o.banned_tokens,
                         length_penalty=o.length_penalty)


def _batched(m, k, wm, enc, tags, kind, options, return_all=True):
    from models.decoders import _common
    with torch.no_grad():
        return _common.beam_search_batched(m, k, wm, enc, tags, use_attention=kind != "pure_scn",
                                           use_tags=kind != "pure_attention", return_all=return_all, options=options)


def _check(got, ref, use_att, where):
    """the bars of test_gpu_beam_search._compare"""
    (one, done), (r_one, r_all) = got, ref
    seq, r_seq = (one[0], r_one[0]) if use_att else (one, r_one)
    assert seq == r_seq, (where, seq, r_seq)
    assert [s for s, _ in done] == [s for s, _ in r_all], where
    for (_, sg), (_, sr) in zip(done, r_all):
        assert abs(sg - sr) <= 1e-4 * max(1.0, abs(sr)), (where, sg, sr)
    if use_att:
        a, r = torch.tensor(one[1]).double(), torch.tensor(r_one[1]).double()
        assert a.shape == r.shape and float((a - r).abs().max()) <= TOL_OUT * float(r.abs().max()), where


def _run_opt(m, kind, V, enc, tags, k, options, **kw):
    """SF.beam_search_run on the decoder's operands -> (results, steps)"""
    from models.decoders import _common
    from scnattn import functional as SF
    dims, weights, e3, tg = _common._search_operands(m, V, enc, tags, kind != "pure_scn", kind != "pure_attention")
    return SF.beam_search_run(dims, k, weights, e3, tg, V - 2, V - 1, options=options, **kw)


# ---- (a) default options are no options ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_default_options_are_no_options_bit_for_bit(dev, name, kind):
    """through sample_batch (an all-default object takes the plain path) and through the _opt calls themselves (the
    selection with an empty bitmap, the advance with the history): sequences, scores and alpha maps EQUAL"""
    from models.decoders import SearchOptions
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    use_tags = kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    for k in BR.BEAMS:
        want = _batched(m, k, wm, enc, tags, kind, None)
        assert _batched(m, k, wm, enc, tags, kind, SearchOptions()) == want
        with torch.no_grad():
            pub = m.sample_batch(k, wm, enc, tags, options=SearchOptions()) if use_tags else \
                m.sample_batch(k, wm, enc, options=SearchOptions())
        assert pub == [one for one, _ in want]
        plain, steps = _run_opt(m, kind, V, enc, tags, k, None)
        opt, steps2 = _run_opt(m, kind, V, enc, tags, k, SearchOptions())
        assert steps == steps2 and plain["history"] is None and opt["history"].shape == (enc.shape[0] * k, steps)
        for key in ("token", "parent", "scores", "comp_score", "comp_step", "comp_parent", "ncomp", "best_idx", "best_score",
                    "nsrc", "kk", "alpha"):
            if plain[key] is None:
                assert opt[key] is None
            else:
                assert torch.equal(plain[key], opt[key]), (k, key)


# ---- (b) the tables against the restatement -----------------------------------------------------------------------------
_COUNTS = {}


@pytest.mark.parametrize("table,idx", [(name, i) for name in sorted(OR.TABLES) for i in range(3)])
def test_tables_vs_restatement(dev, table, idx):
    """E=256, A=D=F=128, M=64, S=40, 7x7, V=1003, N=3, beams 1/3/5; the batch in REVERSED image order gives every image
    the same result"""
    from test_gpu_parity import _build_decoder
    kind, seed, o = OR.TABLES[table][idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    cases = OR.cases(kind, seed, o)
    m = _build_decoder(kind, d, dev).eval()
    use_att = kind != "pure_scn"
    N = enc.shape[0]
    perm = list(reversed(range(N)))
    encd, tagd = enc.to(dev), tags.to(dev)
    left = changed = 0
    for k in BR.BEAMS:
        got = _batched(m, k, wm, encd, tagd, kind, _so(o))
        rev = _batched(m, k, wm, encd[perm], tagd[perm], kind, _so(o))
        assert len(got) == N
        for b in range(N):
            assert rev[perm.index(b)] == got[b], (b, k)
            ref, ok, differs = cases[(b, k)]
            if not ok:
                left += 1
                continue
            _check(got[b], ref, use_att, (table, kind, seed, b, k))
            changed += differs
    print("%s %s %d: %d of 9 cases left out, the n-gram rule changes %d compared captions" % (table, kind, seed, left, changed))
    _COUNTS[(table, idx)] = (left, changed)
    mine = [v for (tb, _), v in _COUNTS.items() if tb == table]
    if len(mine) == 3:
        assert 4 * sum(x for x, _ in mine) <= 27 and sum(c for _, c in mine) >= 3, (table, mine)


# ---- (c) what the search writes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", OR.SEEDS)
def test_history_is_the_parent_chain_and_the_guard_is_intact(dev, kind, seed):
    """a search cut off after 7 steps with min_length = 7: every beam is still open; the downloaded history of every open
    slot is the sequence read off the parent chain; the words behind the workspace are intact; and the full search too"""
    from models.decoders import SearchOptions
    from test_gpu_parity import _build_decoder
    d, V, enc, tags = OR.inputs(kind, seed)
    m = _build_decoder(kind, d, dev).eval()
    N, k = enc.shape[0], 5
    for max_steps, o in ((8, SearchOptions(min_length=7, no_repeat_ngram=2)),
                         (51, SearchOptions(min_length=8, no_repeat_ngram=2, banned_tokens=(OR.UNK,)))):
        res, steps = _run_opt(m, kind, V, enc.to(dev), tags.to(dev), k, o, max_steps=max_steps, guard=4096)
        assert bool((res["guard"] == 0x7FC5A5A5).all()), "words behind the workspace were overwritten"
        assert bool((res["nsrc"] == res["kk"]).all()) and bool((res["ncomp"] + res["kk"] == k).all())
        token, parent, hist = res["token"].tolist(), res["parent"].tolist(), res["history"]
        assert hist.shape == (N * k, steps)
        if max_steps == 8:
            assert steps == 8 and int(res["nsrc"].sum()) >= 1, "picked so that beams are still open at the cut"
        for n in range(N):
            for s in range(int(res["nsrc"][n])):
                words, slot = [], s
                for t_ in range(steps - 1, -1, -1):
                    words.append(token[t_][n * k + slot])
                    slot = parent[t_][n * k + slot]
                assert hist[n * k + s].tolist() == words[::-1], (n, s)
                grams = [tuple(words[i:i + 2]) for i in range(len(words) - 1)]
                assert len(grams) == len(set(grams)) and V - 1 not in words


def test_chunking_does_not_change_a_search_with_options(dev):
    """no_repeat_ngram = 2, min_length = 3 with chunk = 1 and with chunk = max_steps, for the single decoder and for a
    two-member ensemble: every entry of the two result dicts EQUAL, the history included.  Which of the two history buffers
    a step reads depends on t alone, so a step loop that counted from its chunk's start would differ here.
    The fixtures are the smallest of BR.FIXTURES (4 images, 3x3 pixels, E = 32, V = 23; the attention and the tags-only
    decoder share these shapes, so they also make the ensemble).  V = 23 bounds max_steps by the candidate rule
    (23 - 1 - 16 >= 3), and <end> is biased away so that every beam is open at every step: both runs then execute the same
    16 steps -- a chunk of 1 would otherwise stop at the first look after the last image closed, which the other run never
    takes -- and every row's history is a live one."""
    from models.decoders import SearchOptions, _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    k, T, o = 3, 16, SearchOptions(no_repeat_ngram=2, min_length=3)
    ops, V = [], None
    for name, kind in (BR.FIXTURES[1], BR.FIXTURES[2]):
        d, V = BR.sharpened(name)
        d["p.fc.bias"] = d["p.fc.bias"].copy()
        d["p.fc.bias"][V - 1] -= 30.0
        m = _build_decoder(kind, d, dev).eval()
        ops.append(_common._search_operands(m, V, t(d["enc"]).to(dev), t(d["tags"]).to(dev), kind != "pure_scn", True))
    (dims, weights, enc, tags), _ = ops

    def single(chunk):
        return SF.beam_search_run(dims, k, weights, enc, tags, V - 2, V - 1, max_steps=T, chunk=chunk, options=o)

    def pair(chunk):
        return SF.ensemble_search_run([x[0] for x in ops], k, [x[1] for x in ops], enc, [x[3] for x in ops], (0.6, 0.4),
                                      "prob", V - 2, V - 1, 0, max_steps=T, chunk=chunk, options=o)

    for run in (single, pair):
        (one, steps1), (whole, steps) = run(1), run(T)
        assert steps1 == steps == T and int(whole["open_images"]) == enc.shape[0]
        assert sorted(one) == sorted(whole) and whole["history"].shape == (enc.shape[0] * k, T)
        for key in whole:
            assert torch.equal(one[key], whole[key]), (run.__name__, key)


# ---- (d) the ensemble -----------------------------------------------------------------------------------------------------
def _ensemble(dev, members, **kw):
    from models.decoders import DecoderEnsemble
    return DecoderEnsemble(members, **kw).to(dev).eval()


@pytest.mark.parametrize("kind,seed", OR.SEEDS[1:])
def test_one_member_ensemble_is_sample_batch_bit_for_bit(dev, kind, seed):
    from test_gpu_parity import _build_decoder
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    ens = _ensemble(dev, [m])
    o = OR.TABLES["min8_ngram"][OR.SEEDS.index((kind, seed))][2]._replace(length_penalty=0.7)
    for k in BR.BEAMS:
        want = _batched(m, k, wm, enc.to(dev), tags.to(dev), kind, _so(o))
        with torch.no_grad():
            got = ens.sample_batch(k, wm, enc.to(dev), tags.to(dev), return_all=True, options=_so(o))
        assert got == want, k


@pytest.mark.parametrize("mode", ["logprob", "prob"])
def test_two_member_ensemble_vs_restatement(dev, mode):
    from test_gpu_parity import _build_decoder
    import ensemble_refs as ER
    I, o = OR.ensemble_inputs(), OR.ENSEMBLE[2]
    cases = OR.ensemble_cases(ER.MODES[mode])
    wm = BR.word_map(I["V"])
    members = [_build_decoder(kind, d, dev) for kind, d in zip(I["kinds"], I["dicts"])]
    ens = _ensemble(dev, members, weights=I["weights"], combine=mode)
    assert ens.member_weights == I["w"]
    enc, tags = I["enc"].to(dev), I["tags"].to(dev)
    left = changed = 0
    for k in BR.BEAMS:
        with torch.no_grad():
            got = ens.sample_batch(k, wm, enc, tags, return_all=True, options=_so(o))
        for b in range(enc.shape[0]):
            ref, ok, differs = cases[(b, k)]
            if not ok:
                left += 1
                continue
            _check(got[b], ref, True, (mode, b, k))
            changed += differs
    print("two-member ensemble %s: %d of 9 left out, the n-gram rule changes %d" % (mode, left, changed))
    assert 4 * left <= 9 and changed >= 3


# ---- (e) the length penalty on a real search ----------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(3))
def test_length_penalty_returns_the_restatements_caption(dev, idx):
    """the device search does not depend on alpha; the returned caption is the restatement's pick among the restatement's
    completed beams.  A case is compared when it is decidable AND the fp64 margin of the pick (best minus second
    normalised score) exceeds twice the score bar 1e-4 * max(1, |s|) divided by L**alpha -- what fp32 scores may move"""
    from test_gpu_parity import _build_decoder
    kind, seed, o = OR.TABLES["min3_trigram"][idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    cases = OR.cases(kind, seed, o)
    m = _build_decoder(kind, d, dev).eval()
    use_att = kind != "pure_scn"
    compared = moved = 0
    for alpha in (0.7, 1.0):
        for k in BR.BEAMS:
            got = _batched(m, k, wm, enc.to(dev), tags.to(dev), kind, _so(o._replace(length_penalty=alpha)))
            for b in range(enc.shape[0]):
                (r_one, done), ok, _ = cases[(b, k)]
                norm = sorted((s / float(len(q) - 1) ** alpha for q, s in done), reverse=True)
                slack = max(1e-4 * max(1.0, abs(s)) / float(len(q) - 1) ** alpha for q, s in done)
                if not ok or (len(norm) > 1 and norm[0] - norm[1] <= 2 * slack):
                    continue
                i = OR.pick(done, alpha)
                one, gdone = got[b]
                assert (one[0] if use_att else one) == done[i][0], (alpha, b, k)
                assert [q for q, _ in gdone] == [q for q, _ in done]            # raw scores, completion order
                compared += 1
                moved += i != OR.pick(done, 0.0)
    print("%s %d: %d cases compared, alpha moves the pick in %d" % (kind, seed, compared, moved))
    assert compared >= 12 and moved >= 1


# ---- (f) wherever a decoder is taken ------------------------------------------------------------------------------------
def test_captioner_and_evaluate_captions_pass_the_options_through(dev):
    import test_gpu_caption_metrics_step as S
    import test_gpu_captioner as TC
    from models.decoders import SearchOptions
    from models.decoders.attention_scn import AttentionSCN
    from scnattn.inference import Captioner
    from trains.harness import evaluate_captions
    wm = BR.word_map(TC.V)
    o = SearchOptions.from_words(wm, min_length=3)
    assert o.banned_tokens == (wm["<unk>"],)
    enc, tag, dec = TC._modules("attention_scn", dev)
    seen = []
    real = dec.sample_batch

    def spy(*a, **kw):
        seen.append((a, kw, real(*a, **kw)))
        return seen[-1][2]

    dec.sample_batch = spy
    records = Captioner(enc, dec, wm, tagger=tag, beam_size=3, search_options=o)(TC._images())
    dec.sample_batch = real
    (a, kw, results), = seen
    assert kw == {"options": o}
    with torch.no_grad():
        direct = dec.sample_batch(*a, options=o)
        plain = dec.sample_batch(*a)
    assert direct == results and [r["tokens"] for r in records] == [seq for seq, _ in direct]
    assert [r["tokens"] for r in Captioner(enc, dec, wm, tagger=tag, beam_size=3)(TC._images())] == [seq for seq, _ in plain]
    for seq, _ in direct:
        assert wm["<unk>"] not in seq and (seq[-1] != wm["<end>"] or len(seq) - 2 >= 3)
    # evaluate_captions: the same metrics as with a decoder that always searches with these options
    V, B, R, L = 30, 4, 3, 9
    wm = BR.word_map(V)
    o = SearchOptions.from_words(wm, min_length=4)
    torch.manual_seed(9)
    dec = AttentionSCN(24, 20, 28, 36, 14, V, encoder_dim=40, dropout=0.5).to(dev)
    g = torch.Generator().manual_seed(10)
    allcaps = torch.zeros(B, R, L, dtype=torch.long)
    for b in range(B):
        for r in range(R):
            n = int(torch.randint(3, L + 1, (1,), generator=g))
            allcaps[b, r, 0] = wm["<start>"]
            allcaps[b, r, 1:n - 1] = torch.randint(1, 8, (n - 2,), generator=g)
            allcaps[b, r, n - 1] = wm["<end>"]
    imgs = (torch.rand(B, 2, 2, 40, generator=g).to(dev), torch.rand(B, 14, generator=g).to(dev))
    batches = [(imgs, allcaps.to(dev))]
    calls = []
    real = dec.sample_batch

    def spy2(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    dec.sample_batch = spy2
    with_opt = evaluate_captions(batches, S._Encoder(), lambda im: im[1], dec, wm, beam_size=3, search_options=o)
    assert calls == [{"options": o}]
    dec.sample_batch = lambda *a, **kw: real(*a, options=o)
    fixed = evaluate_captions(batches, S._Encoder(), lambda im: im[1], dec, wm, beam_size=3)
    dec.sample_batch = real
    assert {"Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr"} <= set(with_opt)
    assert all(float(with_opt[key]) == float(fixed[key]) for key in ("Bleu_1", "Bleu_4", "ROUGE_L", "CIDEr"))
