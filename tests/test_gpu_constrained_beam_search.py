"""decoder.sample_constrained(beam_size, required, ...) -- constrained beam search on the GPU: required words, beam banks,
the selection kernel's constrained flavour and scnattn_beam_merge_banks -- against the fp64 restatement of
tests/constrained_beam_refs.py.

The reference project has no such search; the restatement is the yardstick.  A case is compared under the decidability rule
of tests/test_gpu_beam_search.py (beam_refs.decidable on the restatement's fp64 and fp32 traces, one entry per (step, bank)
after exclusion and one per step for the picked set) with that file's bars: sequences equal, scores within
1e-4 * max(1, |s|), alphas within 1e-4.  Caps, asserted here and, from the restatement alone, in
tests/test_constrained_beam_refs.py: at most 1/4 of a table's cases left out, at least 3 compared cases per table in which
the requirement changes the caption and is satisfied -- a search that ignored the requirement would fail them.
Fixture sizes are those of the option tables: E=256, A=D=F=128, M=64, S=40, 7x7, V=1003, N=3; BR.FIXTURES (V=23) for the
bit-for-bit tests."""
import ctypes as C

import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
import constrained_beam_refs as CR
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


def _constrained(m, k, req, wm, enc, tags, kind, options=None, **kw):
    from models.decoders import _common
    with torch.no_grad():
        return _common.beam_search_constrained(m, k, req, wm, enc, tags, use_attention=kind != "pure_scn",
                                               use_tags=kind != "pure_attention", options=options, **kw)


def _batched(m, k, wm, enc, tags, kind, options=None, return_all=True):
    from models.decoders import _common
    with torch.no_grad():
        return _common.beam_search_batched(m, k, wm, enc, tags, use_attention=kind != "pure_scn",
                                           use_tags=kind != "pure_attention", return_all=return_all, options=options)


def _equal_results(a, b, where):
    for key in KEYS:
        if a[key] is None:
            assert b[key] is None, (where, key)
        else:
            assert torch.equal(a[key], b[key]), (where, key)
    assert (a["history"] is None) == (b["history"] is None)
    if a["history"] is not None:
        assert torch.equal(a["history"], b["history"]), where


# ---- (a) empty lists: the existing search, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("with_options", [False, True])
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_empty_lists_are_sample_batch_bit_for_bit(dev, name, kind, with_options):
    """required = [[], ..]: SF.beam_search_run then takes the _con calls THEMSELVES (the constrained selection, the bank
    merge), which leave every result tensor EQUAL to the plain search's; sample_constrained returns sample_batch's result"""
    from models.decoders import SearchOptions, _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    use_tags = kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    N = enc.shape[0]
    none = [[] for _ in range(N)]
    # V = 23 here: no n-gram rule (the candidate rule would need 23 - 1 - 51 - 4 >= k)
    o = SearchOptions(min_length=3, banned_tokens=(V - 3,), length_penalty=0.7) if with_options else None
    ops = _common._search_operands(m, V, enc, tags, kind != "pure_scn", use_tags)
    for k in BR.BEAMS:
        want = _batched(m, k, wm, enc, tags, kind, o)
        assert _constrained(m, k, none, wm, enc, tags, kind, o, return_all=True) == want, k
        with torch.no_grad():
            one = m.sample_batch(k, wm, enc, tags, options=o) if use_tags else m.sample_batch(k, wm, enc, options=o)
            pub = m.sample_constrained(k, none, wm, enc, tags, options=o)
        assert pub == one
        plain, steps = SF.beam_search_run(*ops[:1], k, *ops[1:], V - 2, V - 1, options=_common.device_options(o)[0])
        res, steps2 = SF.beam_search_run(*ops[:1], k, *ops[1:], V - 2, V - 1, options=_common.device_options(o)[0],
                                         required=none, pad_token=0)
        assert steps2 == steps and res["met"] is not None and not bool(res["met"].any())
        assert res["required"].shape == (N, 4) and bool((res["required"] == -1).all())
        _equal_results(res, plain, (name, k))


# ---- (b) the tables against the restatement ------------------------------------------------------------------------------
_COUNTS = {}


@pytest.mark.parametrize("table,idx", [(name, i) for name in sorted(CR.TABLES) for i in range(3)])
def test_tables_vs_restatement(dev, table, idx):
    """2 words, 4 words with min_length = 6, 1 word with no_repeat_ngram = 2 and a banned token; beams 1 / 3 / 5; the batch in
    REVERSED image order gives every image the same result; every completed caption returned contains its words"""
    from test_gpu_parity import _build_decoder
    o, ranks, rows = CR.TABLES[table]
    kind, seed = rows[idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    cases = CR.cases(table, idx)
    req = CR.required_words(kind, seed, ranks)
    m = _build_decoder(kind, d, dev).eval()
    use_att = kind != "pure_scn"
    N, end = enc.shape[0], V - 1
    perm = list(reversed(range(N)))
    encd, tagd = enc.to(dev), tags.to(dev)
    so = _so(o) if o != OR.Opts() else None
    left = changed = 0
    for k in BR.BEAMS:
        got = _constrained(m, k, req, wm, encd, tagd, kind, so, return_all=True, with_met=True)
        rev = _constrained(m, k, [req[b] for b in perm], wm, encd[perm], tagd[perm], kind, so, return_all=True, with_met=True)
        for b in range(N):
            assert rev[perm.index(b)] == got[b], (k, b)
            (one, done), score, mask = got[b]
            seq = CR.seq_of(one, kind)
            assert mask == sum(1 << c for c, w in enumerate(req[b]) if w in seq), "met is not what the caption implies"
            for words, _ in done:
                if words[-1] == end:
                    assert all(w in words for w in req[b]), (table, k, b, words)
            ref, ok, rmask, differs, _ = cases[(b, k)]
            if not ok:
                left += 1
                continue
            _check(got[b][0], ref, use_att, (table, kind, seed, b, k))
            assert mask == rmask
            changed += differs
    print("%s %s %d: %d of 9 cases left out, the requirement changes %d compared cases" % (table, kind, seed, left, changed))
    _COUNTS[(table, idx)] = (left, changed)
    mine = [v for (tb, _), v in _COUNTS.items() if tb == table]
    if len(mine) == 3:
        assert 4 * sum(x for x, _ in mine) <= 27 and sum(c for _, c in mine) >= 3, (table, mine)


# ---- (c) invariants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", OR.SEEDS)
def test_mixed_batch_empty_list_is_the_plain_result_and_the_guard_is_intact(dev, kind, seed):
    """image 1 requires nothing: its result EQUALS its plain result (sequences, scores, alpha maps), whatever its neighbours
    require; nothing is written behind the workspace; the masks of the open slots are what their parent chains imply"""
    from models.decoders import _common
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    encd, tagd = enc.to(dev), tags.to(dev)
    req = CR.required_words(kind, seed, (3, 6, 10, 15))
    req[1] = []
    N = enc.shape[0]
    for k in (3, 5):
        got = _constrained(m, k, req, wm, encd, tagd, kind, None, return_all=True)
        plain = _batched(m, k, wm, encd, tagd, kind)
        assert got[1] == plain[1], k
        assert CR.seq_of(got[0][0], kind) != CR.seq_of(plain[0][0], kind)
    ops = _common._search_operands(m, V, encd, tagd, kind != "pure_scn", True)
    for max_steps in (6, 51):
        k = 5
        res, steps = SF.beam_search_run(*ops[:1], k, *ops[1:], V - 2, V - 1, max_steps=max_steps, guard=4096, required=req,
                                        pad_token=0)
        assert bool((res["guard"] == 0x7FC5A5A5).all()), "words behind the workspace were overwritten"
        assert bool((res["nsrc"] == res["kk"]).all()) and bool((res["ncomp"] + res["kk"] == k).all())
        assert res["required"].tolist() == [r + [-1] * (4 - len(r)) for r in req]
        token, parent = res["token"].tolist(), res["parent"].tolist()
        for n in range(N):
            for s in range(int(res["nsrc"][n])):
                words, slot = [], s
                for t_ in range(steps - 1, -1, -1):
                    words.append(token[t_][n * k + slot])
                    slot = parent[t_][n * k + slot]
                assert int(res["met"][n * k + s]) == sum(1 << c for c, w in enumerate(req[n]) if w in words), (n, s)
                assert V - 1 not in words
        if max_steps == 6:      # four words cannot be met and ended in 6 steps by every beam: the cut finds open beams
            assert steps == 6 and int(res["nsrc"][0]) >= 1 and int(res["nsrc"][2]) >= 1


# ---- (d) the ensemble -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", OR.SEEDS)
def test_one_member_ensemble_is_the_single_decoder_bit_for_bit(dev, kind, seed):
    from models.decoders import DecoderEnsemble
    from test_gpu_parity import _build_decoder
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    ens = DecoderEnsemble([m]).to(dev).eval()
    req = CR.required_words(kind, seed, (4, 11))
    o = _so(OR.Opts(min_length=4, no_repeat_ngram=2, length_penalty=0.7))
    for k in BR.BEAMS:
        want = _constrained(m, k, req, wm, enc.to(dev), tags.to(dev), kind, o, return_all=True, with_met=True)
        with torch.no_grad():
            got = ens.sample_constrained(k, req, wm, enc.to(dev), tags.to(dev), options=o, return_all=True, with_met=True)
        assert got == want, k


@pytest.mark.parametrize("mode", ["logprob", "prob"])
def test_two_member_ensemble_vs_restatement(dev, mode):
    from models.decoders import DecoderEnsemble
    from test_gpu_parity import _build_decoder
    import ensemble_refs as ER
    I, o = OR.ensemble_inputs(), OR.ENSEMBLE[2]
    cases = CR.ensemble_cases(ER.MODES[mode])
    req = cases["required"]
    wm = BR.word_map(I["V"])
    members = [_build_decoder(kind, d, dev) for kind, d in zip(I["kinds"], I["dicts"])]
    ens = DecoderEnsemble(members, weights=I["weights"], combine=mode).to(dev).eval()
    enc, tags = I["enc"].to(dev), I["tags"].to(dev)
    left = changed = 0
    for k in BR.BEAMS:
        with torch.no_grad():
            got = ens.sample_constrained(k, req, wm, enc, tags, return_all=True, options=_so(o), with_met=True)
        for b in range(enc.shape[0]):
            ref, ok, rmask, differs, _ = cases[(b, k)]
            if not ok:
                left += 1
                continue
            _check(got[b][0], ref, True, (mode, b, k))
            assert got[b][2] == rmask
            changed += differs
    print("ensemble %s: %d of 9 cases left out, the requirement changes %d compared cases" % (mode, left, changed))
    assert 4 * left <= 9 and changed >= 3


# ---- (e) with options: the length penalty (the n-gram rule and min_length are in the tables) --------------------------------
@pytest.mark.parametrize("idx", range(3))
def test_length_penalty_chooses_among_finished_beams(dev, idx):
    """the device search does not depend on alpha; the returned caption is the restatement's pick among the restatement's
    completed beams, all of which satisfy the requirement.  Compared when the case is decidable, some beam completed AND the
    fp64 margin of the pick exceeds twice the score bar 1e-4 * max(1, |s|) / L**alpha -- what fp32 scores may move"""
    from test_gpu_parity import _build_decoder
    table = "one_word_ngram_unk"
    o, ranks, rows = CR.TABLES[table]
    kind, seed = rows[idx]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    cases = CR.cases(table, idx)
    req = CR.required_words(kind, seed, ranks)
    m = _build_decoder(kind, d, dev).eval()
    compared = 0
    for alpha in (0.7, 1.0):
        for k in BR.BEAMS:
            got = _constrained(m, k, req, wm, enc.to(dev), tags.to(dev), kind, _so(o._replace(length_penalty=alpha)),
                               return_all=True)
            for b in range(enc.shape[0]):
                (r_one, done), ok, _, _, _ = cases[(b, k)]
                if not ok or any(q[-1] != V - 1 for q, _ in done):
                    continue
                norm = sorted((s / float(len(q) - 1) ** alpha for q, s in done), reverse=True)
                slack = max(1e-4 * max(1.0, abs(s)) / float(len(q) - 1) ** alpha for q, s in done)
                if len(norm) > 1 and norm[0] - norm[1] <= 2 * slack:
                    continue
                one, gdone = got[b]
                pick = done[OR.pick(done, alpha)][0]
                assert CR.seq_of(one, kind) == pick and all(w in pick for w in req[b]), (alpha, b, k)
                assert [q for q, _ in gdone] == [q for q, _ in done]
                compared += 1
    print("%s %d: %d cases compared" % (kind, seed, compared))
    assert compared >= 9


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_gpu(dev):
    """every refusal of the Python layer is a ValueError raised while the operands are still CPU tensors (the device check that
    follows would raise a RuntimeError); the C calls refuse the same things without launching: <start> in _init_con, <end>
    in _steps_con, and the rest in every call"""
    from models.decoders import SearchOptions
    from scnattn import _lib
    from scnattn import functional as SF
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened("attention_scn_distinct")
    wm = BR.word_map(V)
    m = _build_decoder("attention_scn", d, torch.device("cpu")).eval()
    enc, tags = t(d["enc"]), t(d["tags"])
    N = enc.shape[0]
    rest = [[] for _ in range(N - 1)]
    for req in ([[1, 2, 3, 4, 5]] + rest, [[V]] + rest, [[3, 3]] + rest, [[V - 1]] + rest, [[V - 2]] + rest, [[0]] + rest,
                [[1]] * (N + 1)):
        with pytest.raises(ValueError):
            m.sample_constrained(3, req, wm, enc, tags)
    with pytest.raises(ValueError):
        m.sample_constrained(3, [[2]] + rest, wm, enc, tags, options=SearchOptions(banned_tokens=(2,)))
    with pytest.raises(ValueError):
        m.sample_constrained(9, [[2]] + rest, wm, enc, tags)
    with pytest.raises(RuntimeError):
        m.sample_constrained(3, [[2]] + rest, wm, enc, tags)
    # the C calls: a workspace that is never touched (the refusals come before any launch or copy)
    dims = _lib.Dims(N, 9, 32, 16, 16, 16, 8, 4, V, 51, 51, 1)
    K, T, start, end = 3, 51, V - 2, V - 1

    def con(rows):
        flat = [w for r in rows for w in list(r) + [-1] * (4 - len(r))]
        tab = (C.c_int32 * len(flat))(*flat)
        c = _lib.Constraints(n_images=len(rows), pad_token=0, required=C.addressof(tab))
        c._keep = tab
        return c

    ws = torch.full((1024,), float("nan"), device=dev)
    st = SF.stream_of(ws)
    h = _lib.lib()
    w = SF.Params()
    for rows, call in (([[start]] + rest, "init"), ([[end]] + rest, "steps"), ([[3, 3]] + rest, "init"),
                       ([[3, 3]] + rest, "steps"), ([[V]] + rest, "init"), ([[0]] + rest, "steps")):
        c = con(rows)
        if call == "init":
            rc = h.scnattn_beam_init_con(st, C.byref(dims), K, T, None, C.byref(c), C.byref(w), SF.ptr(ws), SF.ptr(ws), start,
                                         SF.ptr(ws))
        else:
            rc = h.scnattn_beam_steps_con(st, C.byref(dims), K, T, None, C.byref(c), C.byref(w), SF.ptr(ws), end, 0, 1,
                                          SF.ptr(ws))
        assert rc == -1, (rows, call)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all()), "a refused call wrote to the workspace"
    with pytest.raises(ValueError, match="do not compose"):
        SF.beam_search_run((N, 9, 32, 16, 16, 16, 8, 4, V, 51, 51, 1), 4, (), ws, ws, start, end, groups=2, diversity=0.5,
                           required=[[2]] + rest)


# ---- (h) the Captioner ------------------------------------------------------------------------------------------------------
def test_captioner_constrained(dev):
    """one record per image with the stated keys; satisfied / missing follow the caption; one list for all images or one per
    image; search_options are honoured; a word outside the word map raises"""
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
        real = dec.sample_constrained

        def spy(*a, **kw):
            calls.append((a, kw))
            return real(*a, **kw)

        dec.sample_constrained = spy
        recs = cap.constrained(images, ["w3", "w5"])
        dec.sample_constrained = real
        assert len(calls) == 1 and calls[0][1]["options"] is opts and calls[0][0][1] == [[wm["w3"], wm["w5"]]] * len(images)
        assert len(recs) == len(images)
        a, kw = calls[0]
        with torch.no_grad():
            direct = dec.sample_constrained(*a, options=opts, with_scores=True)
        for rec, (one, score) in zip(recs, direct):
            assert set(rec) == {"tokens", "words", "alphas", "score", "satisfied", "missing"}
            assert rec["tokens"] == one[0] and rec["alphas"] == one[1] and rec["score"] == score
            assert rec["words"] == [cap.rev_word_map[x] for x in one[0] if x not in cap.skip]
            assert rec["missing"] == [x for x in ("w3", "w5") if wm[x] not in rec["tokens"]]
            assert rec["satisfied"] == (not rec["missing"])
            if rec["tokens"][-1] == wm["<end>"]:
                assert rec["satisfied"] and "w3" in rec["words"] and "w5" in rec["words"]
            if opts is not None:
                assert wm["<unk>"] not in rec["tokens"]
        per_image = [["w3", "w5"]] + [[] for _ in images[1:]]
        mixed = cap.constrained(images, per_image)
        assert mixed[0]["tokens"] == recs[0]["tokens"]
        assert [r["tokens"] for r in mixed[1:]] == [r["tokens"] for r in cap(images)[1:]]
        assert all(r["satisfied"] and r["missing"] == [] for r in mixed[1:])
    assert any(r["satisfied"] for r in recs)
    for bad in (["w3", "no-such-word"], [["w3"]] * (len(images) + 1), ["w1", "w2", "w3", "w4", "w5"], ["<end>"], ["w3", "w3"]):
        with pytest.raises(ValueError):
            cap.constrained(images, bad)
