"""The kernels of a batched beam-search step (csrc/beam.hip) through the C ABI, one launch per call, against the fp64
references of tests/beam_refs.py; buffers are guarded windows (tests/kernel_harness.py: sentinel around outputs, NaN around
inputs).

How a case is judged:
  * beam_attn_scores: per element |got - ref| <= (n + 8) * 2^-24 * sum|terms| (att1 / att2 on the 1/256 grid, half a step
    apart, so every ReLU mask is unambiguous); rows of dead slots (j >= nsrc[n]) must still hold the sentinel.
  * beam_attn_context: alpha / awe / z per element within the forward bound of the formula in fp32 (_context_bounds: the
    (n + 8) * 2^-24 * sum|terms| form with the roundings of the softmax counted in); dead rows untouched.
  * beam_row_topk: inputs are drawn from a fixed seed list until the fp64 gap among the top kk+1 MERGED candidates is at
    least 64 x the value bound 2^-24 * ((V + 8) + 2 (|score| + |logit| + |lse|)) -- V positive terms in the sum of
    exponentials, 2-ulp expf, three roundings -- asserted on the CPU before the kernel is called; then the selected words
    must be EQUAL and the values within the bound.
  * beam_merge: picks, compaction, counters and the running best exactly as beam_refs.merge / ImageState.
  * beam_advance: exact (a gather)."""
import ctypes as C

import pytest
import torch

import beam_refs as BR
from kernel_harness import GBuf, NAN, SENT, U, _bound_ok, _call, _note, _slab_buf, _sum_ok, _write_report  # noqa: F401
from test_gpu_decoder_kernels import _f64, _gen, _grid, _ptr

pytestmark = pytest.mark.gpu
REPORT_TITLE = "batched beam-search kernels vs fp64: worst |got - ref| / bound over all cases"
TOL_OUT = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ints(dev, vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _live(nsrc, K):
    return torch.tensor([j < n for n in nsrc for j in range(K)])


def _untouched(buf, live, what):
    """rows of dead slots still hold the sentinel"""
    got = buf.read(what)
    dead = got[~live].view(torch.int32)
    assert bool((dead == SENT).all()), "%s: %d words of dead slots were written" % (what, int((dead != SENT).sum()))
    return got[live]


# P, A, E, K, nsrc per image, mis
SHAPES = [(5, 20, 36, 1, (1,), 0),                  # one slot; scalar-free vector paths at tiny widths
          (17, 516, 260, 3, (1, 3, 2), 0),          # A > 512: three column trips; E: 4 columns in a second workgroup
          (49, 128, 256, 8, (8, 5, 1), 0),          # all 8 slots, 64 candidates; exactly one 256-column workgroup
          (17, 516, 260, 3, (1, 3, 2), 1),          # base off by one float: the non-vector paths although A, E % 4 == 0
          (17, 21, 38, 3, (2, 0, 3), 0)]            # A % 4, E % 4: non-vector; a finished image (nsrc = 0) in the middle


@pytest.mark.parametrize("P,A,E,K,nsrc,mis", SHAPES)
def test_beam_attn_scores(dev, P, A, E, K, nsrc, mis):
    g = _gen(3000 + A + P + K)
    N, nslab = len(nsrc), 2
    R = N * K
    att1 = _grid(g, N, P, A)
    slabs = _grid(g, nslab, R, A)
    bd = _grid(g, A, half=True)
    w, b0 = torch.randn(A, generator=g), torch.randn(1, generator=g)
    live = _live(nsrc, K)
    ref = BR.attn_scores(_f64(att1), _f64(slabs), _f64(bd), _f64(w), _f64(b0), K)
    assert float(ref["pre"].abs().min()) >= 1e-3
    slabs_dev = slabs.clone()
    slabs_dev[:, ~live] = NAN                       # att2 of a dead slot must not be read into a live result
    b_att1 = GBuf(dev, att1.shape, None, att1, mis=mis)
    b_att2, stride, ld = _slab_buf(dev, slabs_dev)
    b_bd, b_w, b_b0 = GBuf(dev, (A,), None, bd), GBuf(dev, (A,), None, w), GBuf(dev, (1,), None, b0)
    b_e = GBuf(dev, (R, P), None, out=True)
    _call("scnattn_beam_attn_scores", dev, N, K, P, A, b_att1.ptr, b_att2.ptr, nslab, stride, ld, b_bd.ptr, b_w.ptr, b_b0.ptr,
          C.c_void_p(_ints(dev, nsrc).data_ptr()), b_e.ptr)
    got = _untouched(b_e, live, "e")
    sub = {"e": ref["e"][live], "e_abs": ref["e_abs"][live], "e_n": ref["e_n"]}
    if got.numel():
        _sum_ok("beam_attn_scores", "e", got, sub)


@pytest.mark.parametrize("P,A,E,K,nsrc,mis", SHAPES)
@pytest.mark.parametrize("gated", [1, 0])
def test_beam_attn_context(dev, P, A, E, K, nsrc, mis, gated):
    g = _gen(4000 + E + P + K)
    N, nslab = len(nsrc), 2
    R = N * K
    enc = torch.randn(N, P, E, generator=g)
    e = torch.randn(R, P, generator=g) * 2
    e[0, 0], e[0, P - 1] = 45.0, -35.0              # a row whose softmax needs the max subtraction
    gp = torch.randn(nslab, R, E, generator=g) * 2 if gated else None
    bb = torch.randn(E, generator=g) if gated else None
    live = _live(nsrc, K)
    ref = BR.attn_context(_f64(enc), _f64(e), _f64(gp), _f64(bb), K)
    e_dev = e.clone()
    e_dev[~live] = NAN
    b_enc, b_e = GBuf(dev, enc.shape, None, enc, mis=mis), GBuf(dev, e.shape, None, e_dev)
    b_gp, stride, ld = _slab_buf(dev, gp) if gated else (None, 0, 0)
    b_bb = GBuf(dev, (E,), None, bb) if gated else None
    b_al, b_awe, b_z = (GBuf(dev, s, None, out=True) for s in ((R, P), (R, E), (R, E)))
    _call("scnattn_beam_attn_context", dev, N, K, P, E, b_enc.ptr, b_e.ptr, _ptr(b_gp), nslab, stride, ld, _ptr(b_bb),
          C.c_void_p(_ints(dev, nsrc).data_ptr()), b_al.ptr, b_awe.ptr, b_z.ptr)
    bounds = _context_bounds(_f64(enc), _f64(e), _f64(gp), _f64(bb), K, ref)
    for name, buf in (("alpha", b_al), ("awe", b_awe), ("z", b_z)):
        got = _untouched(buf, live, name)
        if got.numel():
            _bound_ok("beam_attn_context", name, got, ref[name][live], bounds[name][live])
            if name == "alpha":
                assert bool((got >= 0).all()) and float((got.double().sum(1) - 1).abs().max()) <= P * 2.0 ** -23


def _context_bounds(enc, e, gp, bb, K, ref):
    """Forward bounds of the softmax-weighted sum in fp32, in units of U = 2^-24, from the formula alone.
    ex_p = expf(e_p - m): the subtraction's rounding and the one of expf's own argument scaling are each an absolute
    D_p U on the argument (D_p = |e_p - m|), i.e. relative on the result, and expf is good to 2 ulp beyond that: relative
    (2 D_p + 3) U; the sum s of P such terms adds P roundings and the alpha-weighted mean 2 Dbar + 3 of its terms' errors;
    one division.  Hence |d alpha_p| <= (P + 8 + 2 D_p + 2 Dbar) U alpha_p.
    awe_c = sum_p alpha_p enc_pc adds P roundings: |d awe_c| <= U sum_p (2P + 8 + 2 D_p + 2 Dbar) |alpha_p enc_pc|.
    gate = sigmoid(gpre): gpre is a sum of n terms ((n + 1) U sum|terms| absolute, which moves the sigmoid by at most that
    times gate), expf, an add and a division: relative (n + 1) sum|terms| U + 5 U; z = gate * awe one more rounding."""
    P = e.shape[1]
    alpha = ref["alpha"]
    D = (e - e.max(dim=1, keepdim=True)[0]).abs()
    rel = P + 8 + 2 * D + 2 * (alpha * D).sum(1, keepdim=True)
    encr = enc.repeat_interleave(K, 0).abs()
    awe_abs = (alpha.unsqueeze(2) * encr).sum(1)
    out = {"alpha": U * rel * alpha, "awe": U * ((rel + P) * alpha).unsqueeze(2).mul(encr).sum(1)}
    if gp is None:
        out["z"] = out["awe"]
    else:
        terms = gp.abs().sum(0) + (bb.abs() if bb is not None else 0.0)
        grel = (gp.shape[0] + 2) * terms + 6
        out["z"] = ref["gate"] * (out["awe"] + U * grel * awe_abs)
    return out


# ---- beam_row_topk + beam_merge -----------------------------------------------------------------------------------------
def _value_bound(V, score, logit, lse):
    return U * ((V + 8) + 2 * (abs(score) + abs(logit) + abs(lse)))


def _draw(V, K, nsrc, kk, seed0):
    """logits / scores of ONE image whose merged top kk+1 are separated by >= 64 x the bound in fp64"""
    for seed in range(seed0, seed0 + 50):
        g = _gen(seed)
        logits = (torch.randn(K, V, generator=g) * 3).float()
        for j in range(K):          # a head of min(2K, V) words above the bulk: the top of 10 000 normals alone is too dense
            head = torch.randperm(V, generator=g)[:2 * K]
            logits[j, head] = 12.0 + 0.5 * torch.arange(head.numel()) + 0.2 * torch.rand(head.numel(), generator=g)
        scores = (torch.randn(K, generator=g) * 2).float()
        l64, s64 = logits.double(), scores.double()
        cv, ci, lse = BR.row_topk(l64[:nsrc], s64[:nsrc], K)
        picks = BR.merge(cv, ci, V, min(kk + 1, nsrc * K))
        bound = max(_value_bound(V, float(s64[j]), float(l64[j, w]), float(lse[j])) for _, j, w in picks)
        gaps = [picks[i][0] - picks[i + 1][0] for i in range(len(picks) - 1)]
        rowgaps = (cv[:, :-1] - cv[:, 1:]).min() if K > 1 else torch.tensor(1.0)
        if all(gp >= 64 * bound for gp in gaps) and float(rowgaps) >= 64 * bound:
            return logits, scores
    raise AssertionError("no seed separates the candidates")


class State:
    """the state arrays of scnattn_beam_merge on the device, in the order of scnattn_beam_layout (entries 0..11)"""

    def __init__(self, dev, N, K, T, nsrc, kk, scores, ncomp=None, best=None):
        R = N * K
        z = lambda n: torch.zeros(n, dtype=torch.int32)      # noqa: E731
        self.host = [torch.tensor([sum(1 for x in kk if x > 0)], dtype=torch.int32), torch.tensor(nsrc, dtype=torch.int32),
                     torch.tensor(kk, dtype=torch.int32), torch.tensor(ncomp or [0] * N, dtype=torch.int32),
                     torch.tensor([b[0] for b in best] if best else [-1] * N, dtype=torch.int32),
                     torch.tensor([b[1] for b in best] if best else [0.0] * N, dtype=torch.float32),
                     scores.reshape(R).float().clone(), torch.zeros(R), z(R) - 1, z(R), z(T * R) - 7, z(T * R) - 7]
        self.devt = [x.to(dev) for x in self.host]
        self.ptrs = (C.c_void_p * 12)(*[x.data_ptr() for x in self.devt])

    def read(self):
        names = ("open_images", "nsrc", "kk", "ncomp", "best_idx", "best_score", "scores", "comp_score", "comp_step",
                 "comp_parent", "token", "parent")
        return {n: x.cpu() for n, x in zip(names, self.devt)}


# passes = 1: the row is re-read from global memory in every pass (the path of a vocabulary beyond the LDS), at one V
@pytest.mark.parametrize("V,K,passes", [(V, K, 0) for V in (37, 1003, 10000) for K in (1, 3, 5, 8)] +
                         [(1003, K, 1) for K in (1, 3, 5, 8)])
def test_beam_row_topk_and_merge(dev, V, K, passes):
    """three images: all K sources and kk = K; nsrc < K and kk < K; a finished image.  Words equal, values within the bound."""
    nsrc = [K, max(K - 2, 1), 0]
    kk = [K, max(K - 2, 1), 0]
    N, R, end = 3, 3 * K, V - 1
    logits, scores = torch.zeros(N, K, V), torch.zeros(N, K)
    for n in range(2):
        logits[n], scores[n] = _draw(V, K, nsrc[n], kk[n], 100 * V + 10 * K + n)
    live = _live(nsrc, K)
    ld = V + 3
    lg = logits.reshape(R, V).clone()
    sc = scores.reshape(R).clone()
    lg[~live] = NAN
    b_l = GBuf(dev, (R, V), (ld, 1), lg)
    b_s = GBuf(dev, (R,), None, sc)
    b_v, b_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
    nsrc_d = _ints(dev, nsrc)
    _call("scnattn_beam_row_topk", dev, N, K, V, b_l.ptr, ld, b_s.ptr, C.c_void_p(nsrc_d.data_ptr()), b_v.ptr, b_i.ptr, passes)
    gv = _untouched(b_v, live, "row values")
    gi = _untouched(b_i, live, "row words").view(torch.int32)
    l64, s64 = logits.reshape(R, V).double()[live], scores.reshape(R).double()[live]
    cv, ci, lse = BR.row_topk(l64, s64, K)
    assert torch.equal(gi.long(), ci), "row top-K words differ"
    bound = U * ((V + 8) + 2 * (s64.abs().unsqueeze(1) + l64.gather(1, ci).abs() + lse.abs().unsqueeze(1)))
    _bound_ok("beam_row_topk", "value", gv, cv, bound)
    # the merge on the kernel's own candidates
    st = State(dev, N, K, 2, nsrc, kk, scores)
    candv = torch.full((R, K), NAN)
    candi = torch.zeros(R, K, dtype=torch.int32)
    candv[live], candi[live] = gv, gi
    cvd, cid = candv.to(dev), candi.to(dev)
    _call("scnattn_beam_merge", dev, N, K, V, end, 1, C.c_void_p(cvd.data_ptr()), C.c_void_p(cid.data_ptr()), st.ptrs)
    out = st.read()
    row = 0
    for n in range(N):
        ref = BR.ImageState(K)
        ref.nsrc, ref.kk = nsrc[n], kk[n]
        if kk[n] == 0:
            assert out["token"][R + n * K:R + (n + 1) * K].tolist() == [-7] * K       # a finished image: nothing written
            assert int(out["kk"][n]) == 0 and int(out["nsrc"][n]) == 0
            continue
        picks = BR.merge(cv[row:row + nsrc[n]], ci[row:row + nsrc[n]], V, kk[n])
        tok, par = ref.step(picks, 1, end)
        # the merge copies: an open slot's score is, bit for bit, the candidate value it was given
        want = [float(gv[row + j][gi[row + j].tolist().index(w)]) for w, j in zip(tok[:ref.nsrc], par[:ref.nsrc])]
        assert out["scores"][n * K:(n + 1) * K].tolist() == want + [0.0] * (K - ref.nsrc)
        row += nsrc[n]
        assert out["token"][R + n * K:R + (n + 1) * K].tolist() == tok
        assert out["parent"][R + n * K:R + (n + 1) * K].tolist() == par
        assert int(out["nsrc"][n]) == ref.nsrc and int(out["kk"][n]) == ref.kk and int(out["ncomp"][n]) == len(ref.comp)
    assert out["token"][:R].tolist() == [-7] * R, "another step's records were written"
    assert int(out["open_images"]) == sum(1 for n in range(N) if int(out["kk"][n]) > 0)


def test_beam_exact_ties(dev):
    """two live rows with identical score and identical logits, duplicated logits inside a row: equal values leave in
    flat-index order j*V + v, in the row selection and in the merge"""
    V, K, N = 37, 4, 1
    row = torch.linspace(-2, 1, V)
    row[[3, 9, 20]] = 2.5           # three equal maxima
    row[[5, 6]] = 2.0               # two equal runners-up
    logits = torch.stack([row, row, torch.full((V,), NAN), torch.full((V,), NAN)])
    scores = torch.tensor([-1.25, -1.25, 0.0, 0.0])
    nsrc = _ints(dev, [2])
    ld = V
    b_l, b_s = GBuf(dev, (K, V), None, logits), GBuf(dev, (K,), None, scores)
    b_v, b_i = GBuf(dev, (K, K), None, out=True), GBuf(dev, (K, K), None, out=True)
    for passes in (0, 1):
        _call("scnattn_beam_row_topk", dev, N, K, V, b_l.ptr, ld, b_s.ptr, C.c_void_p(nsrc.data_ptr()), b_v.ptr, b_i.ptr, passes)
        gi = b_i.read("words").view(torch.int32)
        gv = b_v.read("values")
        assert gi[:2].tolist() == [[3, 9, 20, 5]] * 2
        assert torch.equal(gv[0], gv[1]) and float(gv[0, 0]) == float(gv[0, 2]) and float(gv[0, 2]) > float(gv[0, 3])
    st = State(dev, N, K, 1, [2], [4], scores)
    cvd, cid = gv.to(dev), gi.to(dev)
    _call("scnattn_beam_merge", dev, N, K, V, V - 1, 0, C.c_void_p(cvd.data_ptr()), C.c_void_p(cid.data_ptr()), st.ptrs)
    out = st.read()
    assert out["token"].tolist() == [3, 9, 20, 3] and out["parent"].tolist() == [0, 0, 0, 1]
    assert out["nsrc"].tolist() == [4] and out["kk"].tolist() == [4] and out["ncomp"].tolist() == [0]


def test_beam_merge_end_at_ranks_0_and_2(dev):
    """<end> picked at ranks 0 and 2 of 4: the others are compacted in rank order, counters drop by two, the running best
    is replaced only by a strictly greater score, a second image that finishes decrements open_images"""
    V, K, N, end = 11, 4, 2, 10
    candv = torch.tensor([[-0.5, -0.8, -3.0, -4.0], [-0.6, -0.7, -3.5, -4.5], [NAN] * 4, [NAN] * 4,
                          [-1.0, -9.0, -9.5, -9.9], [NAN] * 4, [NAN] * 4, [NAN] * 4])
    candi = torch.tensor([[end, 4, 1, 2], [7, end, 1, 2], [0] * 4, [0] * 4, [end, 1, 2, 3], [0] * 4, [0] * 4, [0] * 4],
                         dtype=torch.int32)
    # image 0: two sources, kk = 4, one earlier completion with score -0.5 (an equal score must not replace it);
    # image 1: one source, kk = 1 and its pick is <end>: the image finishes
    st = State(dev, N, K, 3, [2, 1], [4, 1], torch.zeros(N * K), ncomp=[1, 3], best=[(0, -0.5), (1, -0.2)])
    cvd, cid = candv.to(dev), candi.to(dev)
    _call("scnattn_beam_merge", dev, N, K, V, end, 2, C.c_void_p(cvd.data_ptr()), C.c_void_p(cid.data_ptr()), st.ptrs)
    out = st.read()
    R = N * K
    # ranks: (-0.5, j0, end) (-0.6, j1, 7) (-0.7, j1, end) (-0.8, j0, 4)
    assert out["token"][2 * R:2 * R + K].tolist() == [7, 4, 7, 7] and out["parent"][2 * R:2 * R + K].tolist() == [1, 0, 1, 1]
    assert out["scores"][:K].tolist() == pytest.approx([-0.6, -0.8, 0.0, 0.0])
    assert out["nsrc"].tolist() == [2, 0] and out["kk"].tolist() == [2, 0] and out["ncomp"].tolist() == [3, 4]
    assert out["comp_score"][1:3].tolist() == pytest.approx([-0.5, -0.7]) and out["comp_step"][1:3].tolist() == [2, 2]
    assert out["comp_parent"][1:3].tolist() == [0, 1]
    assert out["best_idx"].tolist() == [0, 1] and out["best_score"].tolist() == pytest.approx([-0.5, -0.2])
    assert out["comp_score"][K + 3].item() == pytest.approx(-1.0) and out["comp_step"][K + 3].item() == 2
    assert int(out["open_images"]) == 1
    assert out["token"][2 * R + K:3 * R].tolist() == [0] * K and out["token"][:2 * R].tolist() == [-7] * (2 * R)


def test_beam_advance_is_exact(dev):
    g = _gen(5)
    N, K, D, M, V = 3, 5, 37, 19, 23
    R = N * K
    h, c, table = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g), torch.randn(V, M, generator=g)
    parent = torch.randint(0, K, (R,), generator=g).int()
    token = torch.randint(0, V, (R,), generator=g).int()
    b_h, b_c, b_t = GBuf(dev, h.shape, None, h), GBuf(dev, c.shape, None, c), GBuf(dev, table.shape, None, table)
    b_hd, b_cd, b_e = (GBuf(dev, s, None, out=True) for s in ((R, D), (R, D), (R, M)))
    pd, td = parent.to(dev), token.to(dev)
    _call("scnattn_beam_advance", dev, N, K, D, M, V, b_h.ptr, b_c.ptr, C.c_void_p(pd.data_ptr()), C.c_void_p(td.data_ptr()),
          b_t.ptr, b_hd.ptr, b_cd.ptr, b_e.ptr)
    h2, c2, emb = BR.advance(h, c, parent.tolist(), token.long().tolist(), table, K)
    assert torch.equal(b_hd.read("h"), h2) and torch.equal(b_cd.read("c"), c2) and torch.equal(b_e.read("emb"), emb)
