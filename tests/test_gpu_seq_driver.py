"""The sequence drivers scnattn_seq_fwd / scnattn_seq_bwd (csrc/sequence.cpp) through the C ABI: the driver tier of
DESIGN.md 3.  References, cases, the row judge and the call pair: tests/seq_driver_refs.py (its CPU half:
tests/test_seq_driver_refs.py).

  a. every row of every output against the fp64 oracle, the bar taken against the ROW's maximum (row_ok), in fp32 mode;
     cells past a caption's length and embedding rows of absent tokens exactly 0; one case per nn.Module for the glue;
  b. extents and content of the workspaces: exactly the reported bytes inside sentinel margins, every output a guarded
     window; NaN-filled workspaces where include/scnattn.h says no fill is needed;
  c. the bookkeeping, bit for bit (torch.equal) in every mode: row isolation, causality, padding, dead cells, zero upstream,
     dalphas == NULL, gating by null pointers, re-use of the workspaces.
The invariants rest on each output row's summation order being fixed by the dims, the options and bt_host alone."""
import pytest
import torch

import seq_driver_refs as S
from kernel_harness import GBig, _write_report  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
REPORT_TITLE = "sequence drivers vs fp64 per row: worst |got - ref| / bound per driver + case and result"
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()  # must load: there is no fallback
    return torch.device("cuda:0")


class _Workspaces:
    """saved and the two scratches, allocated once per module and refilled on the device (a scratch carries 96 MiB of GEMM
    partials); each call gets a window of exactly the reported size"""

    def __init__(self, dev):
        self.dev, self.flat = dev, {}

    def get(self, name, n, fill):
        t = self.flat.get(name)
        if t is None or t.numel() < n:
            t = self.flat[name] = torch.empty(n, device=self.dev, dtype=torch.float32)
        v = t[:n]
        if fill is not None:
            v.fill_(fill)
        return S.PBuf(v)


@pytest.fixture(scope="module")
def ws(dev):
    w = _Workspaces(dev)
    yield w
    w.flat.clear()


def _run(dev, ws, c, mode=0, fills=(0.0, 0.0, 0.0), guarded=False, **kw):
    """one call pair under the case's options; fills: saved, forward scratch, backward scratch (None: left as it is)"""
    from scnattn.functional import set_option
    nsaved, nscratch, _ = S.workspace_floats(dev, c)
    if guarded:
        bufs = [GBig(dev, n, f) for n, f in zip((nsaved, nscratch, nscratch), fills)]
    else:
        bufs = [ws.get(name, n, f) for name, n, f in zip(("saved", "fscratch", "bscratch"), (nsaved, nscratch, nscratch), fills)]
    set_option("ksplit", c.ksplit)
    set_option("decoder_bf16", mode)
    try:
        return S.run_driver(dev, c, *bufs, **kw)
    finally:
        set_option("ksplit", 0)
        set_option("decoder_bf16", 0)


_BASE = {}


def _base(dev, ws, c, mode):
    """the plain run of a case: zero-filled workspaces, every output asked for"""
    key = (c.id, mode)
    if key not in _BASE:
        _BASE[key] = _run(dev, ws, c, mode)
    return _BASE[key]


# ==== a. per row against fp64 ================================================================================================
def _exact_zeros(c, got):
    dead = ~c.live
    assert not bool(got["preds"][dead].ne(0).any()), "preds past the decode length"
    if c.has_att:
        assert not bool(got["alphas"][dead].ne(0).any()), "alphas past the decode length"
    if "g.embedding.weight" in got:
        assert not bool(got["g.embedding.weight"][~S.tokens_present(c)].ne(0).any()), "embedding rows of absent tokens"


@pytest.mark.parametrize("cid", S.CASE_IDS)
def test_rows_vs_fp64(dev, ws, cid):
    c = S.case(cid)
    got = _base(dev, ws, c, 0)
    assert set(got) - {"saved"} == set(c.ref64)
    bad = []
    for name in c.ref64:
        try:
            S.row_ok(("seq_fwd " if name in ("preds", "alphas") else "seq_bwd ") + cid, name, got[name], c.ref64[name],
                     c.ref32[name], S.tol_of(name))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
    _exact_zeros(c, got)


@pytest.mark.parametrize("kind", S.MODULE_KINDS)
def test_module_rows_vs_fp64(dev, kind):
    """AttentionSCN / PureSCN / PureAttention .forward on an unsorted batch: sort, permutation and bt_host are Python's"""
    import copy
    m, (enc, tags, caps, caplens, si), (wp, wa), ref64, ref32 = S.module_case(kind)
    m = copy.deepcopy(m).to(dev).train()
    e2, t2 = enc.to(dev).requires_grad_(True), tags.to(dev).requires_grad_(True)
    args = (e2, caps.to(dev), caplens.to(dev)) if kind == "pure_attention" else (e2, t2, caps.to(dev), caplens.to(dev))
    out = m(*args)                                    # the module's own stable sort
    preds, alphas = out[0], (None if kind == "pure_scn" else out[3])
    assert torch.equal(out[-1].cpu(), si) and list(out[2]) == (caplens.squeeze(1)[si] - 1).tolist()
    loss = (preds * wp.to(dev)).sum() + (0 if alphas is None else (alphas * wa.to(dev)).sum())
    loss.backward()
    got = {"preds": preds.detach(), "denc": e2.grad}
    if alphas is not None:
        got["alphas"] = alphas.detach()
    if kind != "pure_attention":
        got["dtags"] = t2.grad
    got.update({"g." + k: p.grad for k, p in m.named_parameters()})
    assert set(got) == set(ref64)
    bad = []
    for name in ref64:
        try:
            S.row_ok("module " + kind, name, got[name].cpu(), ref64[name], ref32[name], S.tol_of(name))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


# ==== b. extents and content of the workspaces ===============================================================================
@pytest.mark.parametrize("cid", ["att-m4-B6-ragged", "att-m4-pool-B6-ragged-k3", "scn-m4-B6-ragged-k3", "scn-m4-pool-B6-full",
                                 "att-odd-B33-ragged-k3"])
def test_workspace_guard_band(dev, ws, cid):
    """saved and both scratches of exactly the reported bytes between sentinel margins, every output a guarded window
    (run_driver): no margin word changes, and the results are those of the roomy workspaces"""
    c = S.case(cid)
    got = _run(dev, ws, c, 0, fills=(0.0, NAN, 0.0), guarded=True)
    S.same_bits(got, _base(dev, ws, c, 0), cid, names=[n for n in got])


@pytest.mark.parametrize("cid,mode", [("att-m4-B6-full-k3", 0), ("att-m4-B6-full-k3", 2), ("scn-m4-pool-B6-full", 0),
                                      ("att-m4-B33-full", 0), ("att-m4-B33-full", 1), ("att-odd-B6-T1-k3", 0)])
def test_full_length_batch_needs_no_fill(dev, ws, cid, mode):
    """bt_host[T-1] == B: saved, both scratches and alphas NaN-filled give the bits of the zero-filled run"""
    c = S.case(cid)
    assert c.bt_host[-1] == c.B
    got = _run(dev, ws, c, mode, fills=(NAN, NAN, NAN), alphas_fill=NAN)
    names = [n for n in got if n != "saved"]
    assert all(bool(torch.isfinite(got[n]).all()) for n in names)
    S.same_bits(got, _base(dev, ws, c, mode), cid, names=names)


_RAGGED = [(row[0], mode) for row in S.CASES if row[6] in ("ragged", "ties") and row[5] > 1 for mode in (0,) + tuple(row[10])]


@pytest.mark.parametrize("cid,mode", _RAGGED)
def test_ragged_batch_forward_scratch_needs_no_fill(dev, ws, cid, mode):
    """include/scnattn.h: saved, alphas and the backward's scratch zero-filled, the FORWARD's scratch not -- NaN-filled it
    gives the bits of the zero-filled run, the saved state included"""
    c = S.case(cid)
    assert c.bt_host[-1] < c.B
    got = _run(dev, ws, c, mode, fills=(0.0, NAN, 0.0))
    S.same_bits(got, _base(dev, ws, c, mode), cid, names=[n for n in got])


def test_module_forward_scratch_is_poisoned(dev, monkeypatch):
    """scnattn/functional.py hands the forward a scratch from _workspace(..., True): _POISON reaches it (the forward of a
    ragged batch asks for saved and alphas zero-filled and for ONE workspace that is not), and a ragged batch through the
    module gives the same bits with it"""
    import copy
    from scnattn import functional as SF
    m, (enc, tags, caps, caplens, _), (wp, wa), _, _ = S.module_case("attention_scn")
    m = copy.deepcopy(m).to(dev).train()
    asked, inner = [], SF._workspace

    def recording(nfloats, d, fully_written):
        asked.append((nfloats, fully_written))
        return inner(nfloats, d, fully_written)
    monkeypatch.setattr(SF, "_workspace", recording)
    m(enc.to(dev), tags.to(dev), caps.to(dev), caplens.to(dev))
    assert sorted(w for _, w in asked) == [False, False, True], asked
    assert max(asked)[1] is True and max(asked)[0] >= 24 << 20          # the scratch: it carries the 96 MiB of GEMM partials
    runs = []
    for poison in (False, True):
        SF._POISON = poison
        try:
            m.zero_grad(set_to_none=True)
            e = enc.to(dev).requires_grad_(True)
            out = m(e, tags.to(dev), caps.to(dev), caplens.to(dev))
            ((out[0] * wp.to(dev)).sum() + (out[3] * wa.to(dev)).sum()).backward()
            runs.append([out[0].detach(), out[3].detach(), e.grad] + [p.grad.clone() for p in m.parameters()])
        finally:
            SF._POISON = False
    for a, b in zip(*runs):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


# ==== c. exact invariants ====================================================================================================
_INV = [(cid, mode) for cid in ("att-m4-B6-ragged", "att-m4-pool-B6-ragged-k3", "scn-m4-B6-ragged-k3", "att-odd-B33-ragged-k3")
        for mode in (0,) + S.CASES[S.CASE_IDS.index(cid)][10]]
_FWD = ("preds", "alphas")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _other_image(c, b, g):
    """the case with image b's enc, tags and tokens replaced (lengths kept)"""
    enc, tags, caps = c.enc.clone(), c.tags.clone(), c.caps.clone()
    enc[b], tags[b] = torch.rand(enc[b].shape, generator=g), torch.rand(tags[b].shape, generator=g)
    caps[b] = torch.randint(1, c.V - 3, caps[b].shape, generator=g)
    return c.variant(enc=enc, tags=tags, caps=caps)


@pytest.mark.parametrize("cid,mode", _INV)
def test_row_isolation_forward(dev, ws, cid, mode):
    c = S.case(cid)
    base = _base(dev, ws, c, mode)
    for b in (0, c.B // 2, c.B - 1):
        got = _run(dev, ws, _other_image(c, b, _gen(b)), mode, bwd=False)
        keep = torch.tensor([i for i in range(c.B) if i != b])
        for n in _FWD:
            if n in base:
                assert torch.equal(got[n][keep], base[n][keep]), "%s of the other images" % n
                assert not torch.equal(got[n][b], base[n][b])
        a, w = S.saved_rows(c, got["saved"], keep), S.saved_rows(c, base["saved"], keep)
        bad = [n for n in a if not torch.equal(a[n], w[n])]
        assert not bad, "saved state of the other images: %s" % ", ".join(bad)


@pytest.mark.parametrize("cid,mode", _INV)
def test_causality(dev, ws, cid, mode):
    c = S.case(cid)
    base = _base(dev, ws, c, mode)
    for b, t in ((0, 3), (1, c.dl[1] - 1), (0, 0)):
        caps = c.caps.clone()
        caps[b, t] = caps[b, t] % (c.V - 4) + 1
        assert caps[b, t] != c.caps[b, t] and t < c.dl[b]
        got = _run(dev, ws, c.variant(caps=caps), mode, bwd=False)
        keep = torch.tensor([i for i in range(c.B) if i != b])
        for n in _FWD:
            if n in base:
                assert torch.equal(got[n][b, :t], base[n][b, :t]), "%s[%d, :%d]" % (n, b, t)
                assert torch.equal(got[n][keep], base[n][keep])
        assert not torch.equal(got["preds"][b, t], base["preds"][b, t])


@pytest.mark.parametrize("cid,mode", _INV)
def test_padding_and_dead_cells(dev, ws, cid, mode):
    """tokens at or past a caption's length and the columns T..L-1; finite garbage in dpreds / dalphas at t >= dl[b]"""
    c = S.case(cid)
    base = _base(dev, ws, c, mode)
    g = _gen(5)
    pad = torch.ones(c.B, c.L, dtype=torch.bool)
    pad[:, :c.T] = ~c.live
    assert c.L > c.T and bool(pad[:, :c.T].any())
    caps = c.caps.clone()
    caps[pad] = torch.randint(0, c.V, (int(pad.sum()),), generator=g)
    S.same_bits(_run(dev, ws, c.variant(caps=caps), mode), base, "padding tokens")
    dpreds = c.dpreds.clone()
    dpreds[~c.live] = torch.randn(int((~c.live).sum()), c.V, generator=g) * 1e3
    kw = {}
    if c.has_att:
        kw["dalphas"] = c.dalphas.clone()
        kw["dalphas"][~c.live] = -1e3
    S.same_bits(_run(dev, ws, c.variant(dpreds=dpreds, **kw), mode), base, "dead upstream cells")


@pytest.mark.parametrize("cid,mode", _INV)
def test_zero_upstream(dev, ws, cid, mode):
    c = S.case(cid)
    for b in (0, c.B - 1):                       # the longest and the shortest caption
        dpreds = c.dpreds.clone()
        dpreds[b] = 0
        kw = {}
        if c.has_att:
            kw["dalphas"] = c.dalphas.clone()
            kw["dalphas"][b] = 0
        one = c.variant(dpreds=dpreds, **kw)
        r1 = _run(dev, ws, one, mode)
        assert not bool(r1["denc"][b].ne(0).any()) and not bool(r1["dtags"][b].ne(0).any())
        r2 = _run(dev, ws, _other_image(one, b, _gen(40 + b)), mode)
        S.same_bits(r1, r2, "zero upstream for image %d" % b, names=[n for n in r1 if n not in _FWD + ("saved",)])


@pytest.mark.parametrize("cid,mode", [x for x in _INV if not x[0].startswith("scn")])
def test_dalphas_null_is_dalphas_of_zeros(dev, ws, cid, mode):
    c = S.case(cid)
    S.same_bits(_run(dev, ws, c, mode, dalphas=None), _run(dev, ws, c, mode, dalphas="zeros"), "dalphas NULL")


@pytest.mark.parametrize("cid,mode", _INV)
def test_gating_by_null_pointers(dev, ws, cid, mode):
    """any one gradient pointer, denc or dtags NULL: the remaining outputs keep the bits of the full call (pooled:
    pool_transpose feeds d encoder_att.weight and d x, each with the other one omitted, and with both)"""
    c = S.case(cid)
    base = _base(dev, ws, c, mode)
    skips = [(f,) for f, k in c.fields if k is not None] + [("denc",), ("dtags",), ("denc", "dtags")]
    if c.has_att:
        skips.append(("attention_encoder_att_weight", "denc"))
    for skip in skips:
        got = _run(dev, ws, c, mode, skip=skip)
        gone = {"g." + dict(c.fields)[s] if s in dict(c.fields) else s for s in skip}
        assert set(base) - set(got) == gone
        S.same_bits(got, base, "without %s" % "+".join(skip))


@pytest.mark.parametrize("cid,mode", _INV)
def test_workspace_reuse(dev, ws, cid, mode):
    """a second call pair in the same saved / scratch after ANOTHER problem of the same dims ran there, re-zeroed as the
    header says (the forward's scratch not at all); then scnattn_seq_bwd again on the same saved"""
    c = S.case(cid)
    base = _base(dev, ws, c, mode)
    other = _run(dev, ws, S.other_problem(cid), mode)
    assert not torch.equal(other["preds"], base["preds"])
    again = _run(dev, ws, c, mode, fills=(0.0, None, 0.0))
    S.same_bits(again, base, "second run in used workspaces", names=[n for n in again])
    twice = _run(dev, ws, c, mode, fills=(None, None, 0.0), fwd=False)       # fresh output windows: embedding gradient zeroed
    assert set(twice) == set(base) - set(_FWD)
    S.same_bits(twice, base, "seq_bwd twice on one saved", names=[n for n in twice])
