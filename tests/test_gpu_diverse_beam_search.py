"""decoder.sample_groups(beam_size, groups, diversity, ...) -- diverse beam search on the GPU, G groups of Kg beams and a
Hamming penalty inside the merge kernel -- against the fp64 restatement of tests/diverse_beam_refs.py.

The reference project has no such search; the restatement is the yardstick.  A case is compared under the decidability rule
of tests/test_gpu_beam_search.py (beam_refs.decidable on the restatement's fp64 and fp32 traces, one entry per (step,
group), the candidates taken AFTER exclusion and penalty) with that file's bars: sequences equal, scores within
1e-4 * max(1, |s|), alphas within 1e-4.  Caps, asserted here and, from the restatement alone, in
tests/test_diverse_beam_refs.py: at most 1/4 of a table's cases left out, at least 3 compared cases per table in which the
penalty changes some group's caption -- a merge that ignored the penalty would fail them.
Fixture sizes are those of the option tables: E=256, A=D=F=128, M=64, S=40, 7x7, V=1003, N=3."""
import ctypes as C

import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
import diverse_beam_refs as DR
from helpers import t
from test_gpu_beam_options_search import _check, _so

pytestmark = pytest.mark.gpu

KEYS = ("token", "parent", "scores", "comp_score", "comp_step", "comp_parent", "ncomp", "best_idx", "best_score", "nsrc", "kk",
        "alpha", "open_images")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _grouped(m, kg, G, lam, wm, enc, tags, kind, options=None, **kw):
    from models.decoders import _common
    with torch.no_grad():
        return _common.beam_search_grouped(m, kg, G, lam, wm, enc, tags, use_attention=kind != "pure_scn",
                                           use_tags=kind != "pure_attention", options=options, **kw)


def _batched(m, k, wm, enc, tags, kind, options=None, return_all=True):
    from models.decoders import _common
    with torch.no_grad():
        return _common.beam_search_batched(m, k, wm, enc, tags, use_attention=kind != "pure_scn",
                                           use_tags=kind != "pure_attention", return_all=return_all, options=options)


def _div_run(operands, K, V, options, G, lam, ensemble=None):
    """the four _div calls THEMSELVES (SF.*_search_run takes today's entry points when groups == 1) -> the result dict of
    SF.beam_search_run.  operands: one (dims, weights, enc, tags) per member; ensemble: (member weights, mode) or None"""
    from scnattn import _lib
    from scnattn import functional as SF
    M = len(operands)
    end = V - 1
    d = (SF.Dims * M)(*[SF.Dims(*x[0]) for x in operands])
    enc = _lib.f32c(operands[0][2])
    tags = [_lib.f32c(x[3]) for x in operands]
    wl = [tuple(None if w is None else _lib.f32c(w.detach()) for w in x[1]) for x in operands]
    w = (SF.Params * M)(*[SF._params_struct(x) for x in wl])
    opt = None if options is None else SF.search_options_struct(options, V, K, SF.BEAM_MAX_STEPS, end)
    div = _lib.Diversity(groups=G, penalty=lam)
    tail = (C.byref(opt) if opt is not None else None, C.byref(div))
    st, T = SF.stream_of(enc), SF.BEAM_MAX_STEPS
    if ensemble is None:
        ws, off, nwords, steps = SF._run_on_device("scnattn_beam_%s_div", (C.byref(d[0]), K, T, *tail), _lib.BEAM_NOFF_OPT,
                                                   (C.byref(w[0]), SF.ptr(enc), SF.ptr(tags[0]), V - 2),
                                                   (C.byref(w[0]), SF.ptr(enc), end), st, enc.device, T, SF.BEAM_CHUNK, 0)
    else:
        mw, mode = ensemble
        tg = (C.c_void_p * M)(*[x.data_ptr() for x in tags])
        cw = (C.c_float * M)(*mw)
        ws, off, nwords, steps = SF._run_on_device("scnattn_ensemble_%s_div", (M, d, K, T, 0, *tail), _lib.BEAM_NOFF_OPT,
                                                   (w, SF.ptr(enc), tg, V - 2), (w, SF.ptr(enc), cw, mode, end), st,
                                                   enc.device, T, SF.BEAM_CHUNK, 0)
    return SF._beam_results(ws, off, d[0].B, K, d[0].P, steps, nwords, 0, T, groups=G), steps


def _equal_results(a, b, where):
    for key in KEYS:
        if a[key] is None:
            assert b[key] is None, (where, key)
        else:
            assert torch.equal(a[key], b[key]), (where, key)
    assert (a["history"] is None) == (b["history"] is None)
    if a["history"] is not None:
        assert torch.equal(a["history"], b["history"]), where


# ---- (a) one group is the existing search, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("with_options", [False, True])
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_one_group_is_sample_batch_bit_for_bit(dev, name, kind, with_options):
    """sample_groups(k, 1, lambda): sequences, scores and alpha maps EQUAL those of sample_batch(k); and the _div calls
    themselves with groups = 1 (the grouped merge, the selection with Kg = K) leave every result tensor EQUAL to the plain
    search's, for lambda = 0, 0.5 and 1e4"""
    from models.decoders import SearchOptions, _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    use_tags = kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    # V = 23 here: no n-gram rule (the candidate rule would need 23 - 1 - 51 >= k)
    o = SearchOptions(min_length=3, banned_tokens=(V - 3,), length_penalty=0.7) if with_options else None
    ops = _common._search_operands(m, V, enc, tags, kind != "pure_scn", use_tags)
    for k in BR.BEAMS:
        want = _batched(m, k, wm, enc, tags, kind, o)
        with torch.no_grad():
            one = m.sample_batch(k, wm, enc, tags, options=o) if use_tags else m.sample_batch(k, wm, enc, options=o)
        plain, steps = SF.beam_search_run(*ops[:1], k, *ops[1:], V - 2, V - 1, options=_common.device_options(o)[0])
        for lam in (0.0, 0.5, 1e4):
            got = _grouped(m, k, 1, lam, wm, enc, tags, kind, o, return_all=True)
            assert [g for g, in got] == want, (k, lam)
            with torch.no_grad():
                pub = m.sample_groups(k, 1, lam, wm, enc, tags, options=o)
            assert [g for g, in pub] == one
            res, steps2 = _div_run([ops], k, V, _common.device_options(o)[0], 1, lam)
            assert steps2 == steps
            _equal_results(res, plain, (name, k, lam))


@pytest.mark.parametrize("with_options", [False, True])
@pytest.mark.parametrize("mode", ["logprob", "prob"])
def test_one_group_two_member_ensemble_bit_for_bit(dev, mode, with_options):
    from models.decoders import DecoderEnsemble, _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    import ensemble_refs as ER
    I = OR.ensemble_inputs()
    V = I["V"]
    wm = BR.word_map(V)
    members = [_build_decoder(kind, d, dev) for kind, d in zip(I["kinds"], I["dicts"])]
    ens = DecoderEnsemble(members, weights=I["weights"], combine=mode).to(dev).eval()
    enc, tags = I["enc"].to(dev), I["tags"].to(dev)
    o = _so(OR.ENSEMBLE[2]) if with_options else None
    ops = [_common._search_operands(dec, V, enc, tags, att, True) for dec, (att, _) in zip(ens.decoders, ens.kinds)]
    for k in (3, 5):
        with torch.no_grad():
            want = ens.sample_batch(k, wm, enc, tags, return_all=True, options=o)
        plain, steps = SF.ensemble_search_run([x[0] for x in ops], k, [x[1] for x in ops], enc, [x[3] for x in ops],
                                              I["weights"], mode, V - 2, V - 1, 0, options=o)
        for lam in (0.0, 0.5):
            with torch.no_grad():
                got = ens.sample_groups(k, 1, lam, wm, enc, tags, options=o, return_all=True)
            assert [g for g, in got] == want
            res, steps2 = _div_run(ops, k, V, o, 1, lam, ensemble=(ens.member_weights, ER.MODES[mode]))
            assert steps2 == steps
            _equal_results(res, plain, (mode, k, lam))


# ---- (b) a penalty of zero: every group is the Kg-beam search -----------------------------------------------------------
@pytest.mark.parametrize("G,kg", [(2, 3), (8, 1), (3, 1)])
@pytest.mark.parametrize("kind,seed", OR.SEEDS)
def test_zero_penalty_groups_equal_each_other_and_sample_batch(dev, kind, seed, G, kg):
    """lambda = 0: a == r, so every group takes group 0's picks.  Sequences EQUAL group 0's and sample_batch(kg)'s wherever
    the kg-beam case is decidable (beam_options_refs.cases without options); scores within 1e-4 * max(1, |s|) -- not bit
    equality: the GEMMs run over G*kg rows per image instead of kg"""
    from test_gpu_parity import _build_decoder
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    cases = OR.cases(kind, seed, OR.Opts())
    m = _build_decoder(kind, d, dev).eval()
    encd, tagd = enc.to(dev), tags.to(dev)
    want = _batched(m, kg, wm, encd, tagd, kind)
    got = _grouped(m, kg, G, 0.0, wm, encd, tagd, kind, return_all=True)
    compared = 0
    for b in range(enc.shape[0]):
        if not cases[(b, kg)][1]:
            continue
        compared += 1
        (w_one, w_done) = want[b]
        for g in range(G):
            one, done = got[b][g]
            assert DR.seq_of(one, kind) == DR.seq_of(w_one, kind) == DR.seq_of(got[b][0][0], kind), (b, g)
            assert [s for s, _ in done] == [s for s, _ in w_done], (b, g)
            for (_, sg), (_, sr) in zip(done, w_done):
                assert abs(sg - sr) <= 1e-4 * max(1.0, abs(sr)), (b, g, sg, sr)
    assert compared >= 2


# ---- (c) the tables against the restatement -----------------------------------------------------------------------------
_COUNTS = {}


@pytest.mark.parametrize("table,idx", [(name, i) for name in sorted(DR.TABLES) for i in range(3)])
def test_tables_vs_restatement(dev, table, idx):
    """(G, Kg) = (2, 2), (3, 2), (4, 2), and (3, 2) with no_repeat_ngram = 2 and a banned token; the batch in REVERSED
    image order gives every image the same result"""
    from test_gpu_parity import _build_decoder
    G, kg, o, rows = DR.TABLES[table]
    kind, seed, lam = rows[idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    cases = DR.cases(table, idx)
    m = _build_decoder(kind, d, dev).eval()
    use_att = kind != "pure_scn"
    N = enc.shape[0]
    perm = list(reversed(range(N)))
    encd, tagd = enc.to(dev), tags.to(dev)
    so = _so(o) if o != OR.Opts() else None
    got = _grouped(m, kg, G, lam, wm, encd, tagd, kind, so, return_all=True)
    rev = _grouped(m, kg, G, lam, wm, encd[perm], tagd[perm], kind, so, return_all=True)
    assert len(got) == N and all(len(x) == G for x in got)
    left = changed = 0
    for b in range(N):
        assert rev[perm.index(b)] == got[b], b
        ref, ok, differs = cases[b]
        if not ok:
            left += 1
            continue
        for g in range(G):
            _check(got[b][g], ref[g], use_att, (table, kind, seed, b, g))
        changed += differs
    print("%s %s %d: %d of 3 cases left out, the penalty changes %d compared cases" % (table, kind, seed, left, changed))
    _COUNTS[(table, idx)] = (left, changed)
    mine = [v for (tb, _), v in _COUNTS.items() if tb == table]
    if len(mine) == 3:
        assert 4 * sum(x for x, _ in mine) <= 9 and sum(c for _, c in mine) >= 3, (table, mine)


# ---- (d) an invariant that needs no oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed,G,kg", [("attention_scn", 2, 4, 2), ("pure_scn", 78, 3, 2), ("attention_scn", 6, 2, 4)])
def test_huge_penalty_no_group_repeats_an_earlier_groups_word_at_a_step(dev, kind, seed, G, kg):
    """lambda = 1e4.  A group is penalised on at most g*kg <= K - kg distinct words, so each of its rows offers at least kg
    unpenalised candidates among its K, and a penalised one lies 1e4 below them: at no step does a group pick a word that an
    earlier group picked at that step, <end> included.  Read from the records alone: after step t group g holds
    kg - (its completions up to t) open beams in its first slots (token[t]), and picked <end> once per completion at t."""
    from models.decoders import SearchOptions, _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    d, V, enc, tags = OR.inputs(kind, seed)
    m = _build_decoder(kind, d, dev).eval()
    K, N, end = G * kg, enc.shape[0], V - 1
    ops = _common._search_operands(m, V, enc.to(dev), tags.to(dev), kind != "pure_scn", True)
    res, steps = SF.beam_search_run(*ops[:1], K, *ops[1:], V - 2, end, options=SearchOptions(min_length=4), groups=G,
                                    diversity=1e4)
    assert res["nsrc"].shape == (N * G,) and bool((res["nsrc"] == res["kk"]).all())
    assert bool((res["ncomp"] + res["kk"] == kg).all())
    token, comp_step = res["token"].tolist(), res["comp_step"].tolist()
    busy = 0
    for n in range(N):
        for step in range(steps):
            seen = set()
            for g in range(G):
                r0 = n * K + g * kg
                ends = [s for s in comp_step[r0:r0 + int(res["ncomp"][n * G + g])]]
                before, now = sum(1 for s in ends if s < step), sum(1 for s in ends if s == step)
                if kg - before == 0:
                    continue                        # finished before this step: picks nothing, penalises nobody
                nopen = kg - before - now
                words = token[step][r0:r0 + nopen] + [end] * now
                assert end not in words[:nopen]
                assert not (set(words) & seen), (n, step, g, words, sorted(seen))
                seen |= set(words)
                busy += len(words) > 0 and g > 0
    assert busy >= steps, "later groups were searching"


# ---- (e) refusals, and the Captioner ------------------------------------------------------------------------------------
def test_refusals_come_before_the_gpu(dev):
    """every refusal is a ValueError raised while the operands are still CPU tensors (the device check that follows would
    raise a RuntimeError); the C calls refuse the same things"""
    from models.decoders import DecoderEnsemble, SearchOptions
    from scnattn import _lib
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened("attention_scn_distinct")
    wm = BR.word_map(V)
    m = _build_decoder("attention_scn", d, torch.device("cpu")).eval()
    enc, tags = t(d["enc"]), t(d["tags"])
    for target in (m, DecoderEnsemble([m])):
        for kg, G, lam in ((0, 2, 0.5), (2, 0, 0.5), (3, 3, 0.5), (2, 5, 0.5), (1.5, 2, 0.5), (2, 2, -0.1), (2, 2, float("nan")),
                           (2, 2, float("inf"))):
            with pytest.raises(ValueError):
                target.sample_groups(kg, G, lam, wm, enc, tags)
        with pytest.raises(ValueError):             # the candidate rule takes the total K: 23 - 15 - 1 = 7 >= 2, but < 8
            target.sample_groups(2, 4, 0.5, wm, enc, tags, options=SearchOptions(banned_tokens=tuple(range(1, 16))))
        with pytest.raises(RuntimeError):           # accepted arguments reach the device check
            target.sample_groups(2, 2, 0.5, wm, enc, tags)
    dims = _lib.Dims(3, 9, 32, 16, 16, 16, 8, 4, V, 51, 51, 1)
    nbytes = C.c_size_t()
    for K, G, lam in ((6, 0, 0.5), (6, 4, 0.5), (9, 3, 0.5), (0, 1, 0.5), (6, 3, -1.0), (6, 3, float("nan")), (6, 3, float("inf"))):
        with pytest.raises(RuntimeError):
            _lib.call("scnattn_beam_workspace_div", C.byref(dims), K, 51, None, C.byref(_lib.Diversity(G, lam)), C.byref(nbytes))
    with pytest.raises(RuntimeError):
        _lib.call("scnattn_beam_workspace_div", C.byref(dims), 6, 51, None, None, C.byref(nbytes))
    _lib.call("scnattn_beam_workspace_div", C.byref(dims), 6, 51, None, C.byref(_lib.Diversity(3, 0.5)), C.byref(nbytes))
    assert nbytes.value > 0


def test_captioner_diverse(dev):
    """G records per image from one search; at groups = 1 the first (only) group is __call__'s caption; search_options are
    honoured; the scores are raw sums of log-probabilities (those of the same beams under sample_groups)"""
    import test_gpu_captioner as TC
    from models.decoders import SearchOptions
    from scnattn.inference import Captioner
    wm = BR.word_map(TC.V)
    enc, tag, dec = TC._modules("attention_scn", dev)
    images = TC._images()
    o = SearchOptions.from_words(wm, min_length=3)
    for opts in (None, o):
        cap = Captioner(enc, dec, wm, tagger=tag, beam_size=3, search_options=opts)
        calls = []
        real = dec.sample_groups

        def spy(*a, **kw):
            calls.append((a, kw))
            return real(*a, **kw)

        dec.sample_groups = spy
        recs = cap.diverse(images, groups=3, beam_size=2, diversity=0.5)
        dec.sample_groups = real
        assert len(calls) == 1 and calls[0][1]["options"] is opts
        assert len(recs) == len(images) and all(len(r) == 3 for r in recs)
        a, kw = calls[0]
        with torch.no_grad():
            direct = dec.sample_groups(*a, options=opts, return_all=True)
        for per_image, want in zip(recs, direct):
            for g, (rec, (one, done)) in enumerate(zip(per_image, want)):
                assert set(rec) == {"group", "tokens", "words", "score"} and rec["group"] == g
                assert rec["tokens"] == one[0] and rec["score"] in [s for _, s in done]
                assert rec["words"] == [cap.rev_word_map[w] for w in one[0] if w not in cap.skip]
                if opts is not None:
                    assert wm["<unk>"] not in rec["tokens"]
        single = cap.diverse(images, groups=1, beam_size=3, diversity=0.5)
        assert [r[0]["tokens"] for r in single] == [r["tokens"] for r in cap(images)]
    with pytest.raises(ValueError):
        cap.diverse(images, groups=3, beam_size=3)
