"""sample_batch() -- the batched beam search resident on the GPU (csrc/beam_search.cpp, csrc/beam.hip) -- against
oracle/beam_ref.py in fp64, against this build's per-image sample(), and for what it writes.

A search is a chain of discrete choices: a case can only be compared when fp32 arithmetic cannot change a choice.  A case
(fixture or shape, image, beam size) is DECIDABLE when (1) the CPU oracle run in fp32 picks the same indices as in fp64 at
every step and (2) every fp64 gap between consecutive entries of each step's top k+1 is at least max(8 x the worst
fp32-vs-fp64 running-score difference of that case, 1e-5); both come from the CPU oracle alone (beam_refs.trace_oracle /
decidable).  Undecidable cases are left out, under asserted caps: at most 1/4 of all cases of a table and at most 1/2 of
any fixture's.  Bars: sequences equal, scores within 1e-4 * max(1, |s|), alphas within 1e-4 (those of
test_sample_beam_search_vs_oracle).  Where the oracle raises (nothing completed) the result must be the sequence this
build's sample() returns on the GPU."""
import pytest
import torch

import beam_refs as BR
from helpers import params_from, t

pytestmark = pytest.mark.gpu

TOL_OUT = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _seq(one, use_att):
    return one[0] if use_att else one


def _sample(m, k, wm, enc, tags):
    with torch.no_grad():
        return m.sample(k, wm, enc, tags) if tags is not None else m.sample(k, wm, enc)


def _batched(m, k, wm, enc, tags, kind, return_all=True):
    from models.decoders import _common
    with torch.no_grad():
        return _common.beam_search_batched(m, k, wm, enc, tags, use_attention=kind != "pure_scn",
                                           use_tags=kind != "pure_attention", return_all=return_all)


def _compare(m, kind, wm, enc, tags, cases, dev):
    """all images as one batch per beam size; -> number of cases left out"""
    use_att = kind != "pure_scn"
    V = len(wm)
    left = 0
    for k in BR.BEAMS:
        got = _batched(m, k, wm, enc.to(dev), None if tags is None else tags.to(dev), kind)
        assert len(got) == enc.shape[0]
        for b, (one, done) in enumerate(got):
            ref, ok = cases[(b, k)]
            if not ok:
                left += 1
                continue
            seq = _seq(one, use_att)
            if ref is None:         # the reference would raise: this build's sample() is the yardstick
                alone = _sample(m, k, wm, enc[b:b + 1].to(dev), None if tags is None else tags[b:b + 1].to(dev))
                assert seq == _seq(alone, use_att) and seq[0] == V - 2 and len(seq) >= 52, (b, k)
                continue
            r_one, r_all = ref
            assert seq == _seq(r_one, use_att), (b, k, seq, _seq(r_one, use_att))
            assert [s for s, _ in done] == [s for s, _ in r_all], (b, k)
            for (_, sg), (_, sr) in zip(done, r_all):
                assert abs(sg - sr) <= 1e-4 * max(1.0, abs(sr)), (b, k, sg, sr)
            if use_att:
                a, r = torch.tensor(one[1]).double(), torch.tensor(r_one[1]).double()
                assert a.shape == r.shape and float((a - r).abs().max()) <= TOL_OUT * float(r.abs().max()), (b, k)
    return left


# ---- (a) the four fixtures --------------------------------------------------------------------------------------------
_LEFT = {}


@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_fixture_batch_vs_oracle(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    m = _build_decoder(kind, d, dev).eval()
    cases = BR.oracle_cases(name, kind)
    enc = t(d["enc"])
    tags = t(d["tags"]) if kind != "pure_attention" else None
    left = _compare(m, kind, BR.word_map(V), enc, tags, cases, dev)
    print("%s: %d of %d cases left out" % (name, left, len(cases)))
    assert 2 * left <= len(cases)
    _LEFT[name] = (left, len(cases))
    if len(_LEFT) == len(BR.FIXTURES):
        assert sum(n for _, n in _LEFT.values()) == 54 and 4 * sum(o for o, _ in _LEFT.values()) <= 54, _LEFT


# ---- (b) vector-width shapes ------------------------------------------------------------------------------------------
def _uniform_params(kind, g):
    E, A, D, Fd, M, S, V = 256, 128, 128, 128, 64, 40, 1003

    def u(*shape, r):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * r).numpy()

    d = {"p.embedding.weight": u(V, M, r=1.0), "p.fc.weight": u(V, D, r=1.0), "p.fc.bias": u(V, r=0.1),
         "p.init_h.weight": u(D, E, r=E ** -0.5), "p.init_h.bias": u(D, r=0.1),
         "p.init_c.weight": u(D, E, r=E ** -0.5), "p.init_c.bias": u(D, r=0.1)}
    I = M + E if kind == "attention_scn" else M
    d.update({"p.decode_step.weight_ia": u(I, 4 * Fd, r=I ** -0.5), "p.decode_step.weight_ib": u(S, 4 * Fd, r=1.0),
              "p.decode_step.weight_ic": u(D, 4 * Fd, r=Fd ** -0.5), "p.decode_step.weight_ha": u(D, 4 * Fd, r=D ** -0.5),
              "p.decode_step.weight_hb": u(S, 4 * Fd, r=1.0), "p.decode_step.weight_hc": u(D, 4 * Fd, r=Fd ** -0.5),
              "p.decode_step.bias_ih": u(4 * D, r=0.1), "p.decode_step.bias_hh": u(4 * D, r=0.1)})
    if kind == "attention_scn":
        d.update({"p.attention.encoder_att.weight": u(A, E, r=E ** -0.5), "p.attention.encoder_att.bias": u(A, r=0.1),
                  "p.attention.decoder_att.weight": u(A, D, r=D ** -0.5), "p.attention.decoder_att.bias": u(A, r=0.1),
                  "p.attention.full_att.weight": u(1, A, r=1.0), "p.attention.full_att.bias": u(1, r=0.1),
                  "p.f_beta.weight": u(E, D, r=D ** -0.5), "p.f_beta.bias": u(E, r=0.1)})
    d["p.fc.bias"][V - 1] += 2.0 if kind == "attention_scn" else 1.0
    return d, V, E, S


# seeds picked on the CPU oracle alone: 6 -> chosen lengths 2-7 over up to 10 steps, 2 -> searches that use all 51 steps with
# completed beams behind them, 78 (pure_scn) -> chosen lengths up to 33, i.e. long back-traces; none leaves a case out
@pytest.mark.parametrize("kind,seed", [("attention_scn", 6), ("attention_scn", 2), ("pure_scn", 78)])
def test_vector_width_shapes_vs_oracle(dev, kind, seed):
    """E=256, A=128, D=F=128, M=64, S=40, 7x7, V=1003, N=3: every 16-byte path of the two attention kernels and the
    staged row selection"""
    from test_gpu_parity import _build_decoder
    g = torch.Generator().manual_seed(seed)
    d, V, E, S = _uniform_params(kind, g)
    N = 3
    enc, tags = torch.rand(N, 7, 7, E, generator=g), torch.rand(N, S, generator=g)
    wm = BR.word_map(V)
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    cases = {}
    for b in range(N):
        for k in BR.BEAMS:
            r64, t64 = BR.trace_oracle(kind, P64, k, wm, enc[b:b + 1].double(), tags[b:b + 1].double())
            _, t32 = BR.trace_oracle(kind, P32, k, wm, enc[b:b + 1], tags[b:b + 1])
            cases[(b, k)] = (r64, BR.decidable(t64, t32))
    lens = sorted({len(_seq(r[0], kind != "pure_scn")) for r, _ in cases.values() if r is not None})
    m = _build_decoder(kind, d, dev).eval()
    left = _compare(m, kind, wm, enc, tags, cases, dev)
    print("%s: %d of %d cases left out; chosen lengths %s" % (kind, left, len(cases), lens))
    assert 4 * left <= len(cases)


# ---- (c) sample_batch == sample per image, in any image order ---------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_sample_batch_equals_sample(dev, name, kind):
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    cases = BR.oracle_cases(name, kind)
    use_att, use_tags = kind != "pure_scn", kind != "pure_attention"
    enc = t(d["enc"]).to(dev)
    tags = t(d["tags"]).to(dev) if use_tags else None
    N = enc.shape[0]
    perm = list(reversed(range(N)))
    compared = 0
    for k in BR.BEAMS:
        with torch.no_grad():
            pub = m.sample_batch(k, wm, enc, tags) if use_tags else m.sample_batch(k, wm, enc)
        got = _batched(m, k, wm, enc, tags, kind)
        rev = _batched(m, k, wm, enc[perm], None if tags is None else tags[perm], kind)
        for b in range(N):
            assert _seq(pub[b], use_att) == _seq(got[b][0], use_att)
            # the same image at another place of the batch: nothing of its result may change
            assert rev[perm.index(b)][0] == got[b][0] and rev[perm.index(b)][1] == got[b][1], (b, k)
            if not cases[(b, k)][1]:
                continue
            from models.decoders import _common
            with torch.no_grad():
                one, done = _common.beam_search(m, k, wm, enc[b:b + 1], None if tags is None else tags[b:b + 1],
                                                use_attention=use_att, use_tags=use_tags, return_all=True)
            assert _seq(got[b][0], use_att) == _seq(one, use_att), (b, k)
            assert [s for s, _ in got[b][1]] == [s for s, _ in done], (b, k)
            for (_, sg), (_, sr) in zip(got[b][1], done):
                assert abs(sg - sr) <= 1e-4 * max(1.0, abs(sr)), (b, k, sg, sr)
            compared += 1
    assert compared >= 4


# ---- (d) nothing is written behind the workspace ----------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [BR.FIXTURES[0], BR.FIXTURES[2]])
def test_workspace_guard_band(dev, name, kind):
    from test_gpu_parity import _build_decoder
    from models.decoders.attention_scn import _collect_weights
    from scnattn import functional as SF
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    m = _build_decoder(kind, d, dev).eval()
    enc = t(d["enc"]).to(dev)
    N, hh, ww, E = enc.shape
    att = kind != "pure_scn"
    dims = (N, hh * ww, E, m.attention_dim if att else 0, m.decoder_dim, m.factored_dim, m.embed_dim, m.semantic_dim, V,
            51, 51, int(att))
    res, steps = SF.beam_search_run(dims, 5, _collect_weights(m), enc.reshape(N, hh * ww, E), t(d["tags"]).to(dev), V - 2,
                                    V - 1, guard=4096)
    assert steps >= 1 and bool((res["guard"] == 0x7FC5A5A5).all()), "words behind the workspace were overwritten"
    assert bool((res["nsrc"] == res["kk"]).all()) and int(res["open_images"]) == int((res["kk"] > 0).sum())
    assert bool((res["ncomp"] + res["kk"] == 5).all())
    for a in (res["scores"], res["comp_score"], res["best_score"]):
        assert bool(torch.isfinite(a).all())
