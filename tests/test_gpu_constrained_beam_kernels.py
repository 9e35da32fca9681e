"""The two kernels a constrained search changes (csrc/beam.hip), through the C ABI, one launch per call, against the fp64
restatement of tests/constrained_beam_refs.py; buffers are guarded windows (tests/kernel_harness.py).

  * scnattn_beam_row_topk_con / _row_topk_ens_con, the selection that also emits the REQUIRED candidates.  Every live row
    has a head of words at least 0.3 apart in every member's logits, far above the bulk, with -- from the top -- the required
    word the row must offer (or <end>, where the row has met everything), <end>, the other required words, the head.  So an
    unmet required word and <end> sit in the plain top K of every live row, and a kernel that ignored the masks fails.  The
    fp64 top K + 1 ORDINARY candidates of every live row are separated by at least 64 x the value bound (asserted on the CPU
    before the launch: 2^-24 ((V + 8) + 2 (|score| + |logit| + |lse|)); the ensemble: ensemble_refs.value_bounds); then the
    words must be EQUAL and the values within the bound -- the judge of tests/test_gpu_beam_options_kernels.py.  A required
    candidate's value equals BIT FOR BIT the plain kernel's first output on the rows where that word is the row's top-1, and
    all four outputs agree in bits between the staged and the forced-pass launch.
  * scnattn_beam_merge_banks on hand-made candidates against constrained_beam_refs.merge_state.  EXACT: values are small
    multiples of 1/4, so ties are real ties.  Every state array and met sit in guarded windows."""
import ctypes as C

import pytest
import torch

import beam_options_refs as OR
import constrained_beam_refs as CR
import ensemble_refs as ER
from kernel_harness import GBuf, GBufI, NAN, SENT, U, _bound_ok, _call, _write_report  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
REPORT_TITLE = "constrained beam-search selection vs fp64: worst |got - ref| / bound over all cases"
WEIGHTS = {1: None, 3: (0.5, 0.3, 0.2)}
FLOATS = ("best_score", "scores", "comp_score")
NEG = -float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _ints(dev, vals):
    return torch.tensor(vals, dtype=torch.int32, device=dev)


def _copts(o):
    from scnattn._lib import SearchOpts
    c = SearchOpts(min_length=o.min_length, no_repeat_ngram=o.no_repeat_ngram, n_banned=len(o.banned_tokens))
    for i, b in enumerate(o.banned_tokens):
        c.banned[i] = b
    return c


# ---- the selection --------------------------------------------------------------------------------------------------------
def _select(dev, M, rows, ld, w, mode, K, V, N, b_s, nsrc_d, o, end, t, b_h, T, req_d, met_d, passes, single, con=True):
    """one launch -> the four output windows (outv, outi, reqv, reqi); con False: the plain kernel (two windows)"""
    R = N * K
    b_v, b_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
    nsp = C.c_void_p(nsrc_d.data_ptr())
    pl = (C.c_void_p * M)(*[r.ptr.value for r in rows])
    ll = (C.c_long * M)(*([ld] * M))
    wl = (C.c_float * M)(*w)
    if not con:
        if single:
            _call("scnattn_beam_row_topk", dev, N, K, V, rows[0].ptr, ld, b_s.ptr, nsp, b_v.ptr, b_i.ptr, passes)
        else:
            _call("scnattn_beam_row_topk_ens", dev, N, K, V, M, pl, ll, wl, mode, b_s.ptr, nsp, b_v.ptr, b_i.ptr, passes)
        return b_v, b_i
    b_rv, b_ri = GBuf(dev, (R, 4), None, out=True), GBuf(dev, (R, 4), None, out=True)
    co = C.byref(_copts(o)) if o is not None else None
    hp = b_h.ptr if b_h is not None else None
    tail = (co, end, t, hp, T, C.c_void_p(req_d.data_ptr()), C.c_void_p(met_d.data_ptr()), b_v.ptr, b_i.ptr, b_rv.ptr, b_ri.ptr,
            passes)
    if single:
        _call("scnattn_beam_row_topk_con", dev, N, K, V, rows[0].ptr, ld, b_s.ptr, nsp, *tail)
    else:
        _call("scnattn_beam_row_topk_ens_con", dev, N, K, V, M, pl, ll, wl, mode, b_s.ptr, nsp, *tail)
    if b_h is not None:
        b_h.read("history")
    return b_v, b_i, b_rv, b_ri


def _build(V, K, M, g, T, t, seed):
    """three images: 4 required words and all K sources live; 2 required words and nsrc < K, row 0 having met both; a finished
    image.  Row j of image 0 has met word (j + 2) % 4 only, must offer word j % 4 (its top-1) and word (j + 3) % 4, and --
    with the unigram rule (g = 1) -- holds word (j + 1) % 4 in its history although its mask says unmet: excluded by the
    options, so not offered.  -> everything the case needs"""
    gen = torch.Generator().manual_seed(seed)
    end, N = V - 1, 3
    nsrc = [K, max(K - 2, 1), 0]
    words = torch.randperm(V - 1, generator=gen).tolist()
    reqs = [words[:4], words[4:6], words[6:7]]
    table = torch.full((N, 4), -1, dtype=torch.int32)
    for n, r in enumerate(reqs):
        table[n, :len(r)] = torch.tensor(r, dtype=torch.int32)
    met = torch.zeros(N, K, dtype=torch.int32)
    for j in range(K):
        met[0, j] = 1 << ((j + 2) % 4)
        met[1, j] = 0b11 if j == 0 else 0b01
    logits = [(torch.randn(N, K, V, generator=gen) * 3).float() for _ in range(M)]
    hist = torch.full((N, K, T), -1, dtype=torch.int32)
    top1 = {}
    for n in range(2):
        req = reqs[n]
        pool = [v for v in words if v not in req]
        for j in range(K):
            nh = min(K + 12, len(pool))
            head = [pool[i] for i in torch.randperm(len(pool), generator=gen)[:nh].tolist()]
            complete = int(met[n, j]) == CR.full_mask(req)
            first = req[j % 4] if n == 0 else req[1]            # unmet in the row unless the row is complete
            ladder = head + [v for v in req if v != first]         # ascending: the head, the other required words, ...
            ladder += [first, end] if complete else [end, first]    # ... then <end> and the row's top-1
            top1[(n, j)] = ladder[-1]
            for m in range(M):
                lv = 12.0 + (0.5 + 0.1 * m) * torch.arange(len(ladder)) + 0.2 * torch.rand(len(ladder), generator=gen)
                logits[m][n, j, ladder] = lv
            h = [head[-1], head[-2]] + [pool[i] for i in torch.randint(0, len(pool), (T,), generator=gen).tolist()]
            if n == 0:
                h[2] = req[(j + 1) % 4]
            hist[n, j, :t] = torch.tensor(h[:t], dtype=torch.int32)
    scores = (torch.randn(N, K, generator=gen) * 2).float()
    banned = (words[7],)                                        # some word that is not required
    o = OR.Opts(min_length=0, no_repeat_ngram=g, banned_tokens=banned)
    return dict(end=end, N=N, nsrc=nsrc, reqs=reqs, table=table, met=met, logits=logits, hist=hist, scores=scores, o=o,
                top1=top1)


def _case(dev, V, K, M, mode, g, T, t, ens, with_opt=True):
    I = _build(V, K, M, g, T, t, 7000 + 10 * V + K + 100 * g + M)
    end, N, nsrc = I["end"], I["N"], I["nsrc"]
    R = N * K
    o = I["o"] if with_opt else None
    oo = I["o"] if with_opt else OR.Opts()
    w = ER.member_weights(WEIGHTS[M], M) if ens else [1.0]
    live = torch.tensor([j < n for n in nsrc for j in range(K)])
    ld = V + (3 if V % 2 else 4)
    rows = []
    for m in range(M):
        x = I["logits"][m].reshape(R, V).clone()
        x[~live] = NAN
        rows.append(GBuf(dev, (R, V), (ld, 1), x))
    b_s = GBuf(dev, (R,), None, I["scores"].reshape(R))
    b_h = GBufI(dev, R * T, I["hist"].reshape(-1)) if with_opt else None
    nsrc_d, req_d, met_d = _ints(dev, nsrc), I["table"].to(dev), I["met"].reshape(-1).to(dev)
    lrows = [r for r in range(R) if bool(live[r])]
    l64 = [x.reshape(R, V).double()[live] for x in I["logits"]]
    s64 = I["scores"].reshape(R).double()[live]
    val = s64.unsqueeze(1) + ER.combine(l64, w, mode)
    sets = [OR.excluded(I["hist"].reshape(R, T)[r].tolist(), t, V, end, oo) for r in lrows]
    reqs = [I["reqs"][r // K] for r in lrows]
    mets = [int(I["met"].reshape(-1)[r]) for r in lrows]
    K1 = K + 1
    cv1, ci1, rv, ri = CR.row_select(val, sets, reqs, mets, K1, end)
    cv, ci = cv1[:, :K], ci1[:, :K]
    if ens:
        bv = ER.value_bounds(l64, w, mode, s64)[1]
    else:
        lse = torch.logsumexp(l64[0], dim=1, keepdim=True)
        bv = U * ((V + 8) + 2 * (s64.abs().unsqueeze(1) + l64[0].abs() + lse.abs()))
    assert float((cv1[:, :-1] - cv1[:, 1:]).min()) >= 64 * float(bv.gather(1, ci1).max()), "the draw does not separate"
    plain = torch.sort(-val, dim=1, stable=True)[1][:, :K]
    for q, r in enumerate(lrows):           # the masks matter: an unmet required word or <end> is the plain top-1
        unmet = {wd for c, wd in enumerate(reqs[q]) if not (mets[q] >> c) & 1}
        assert int(plain[q, 0]) in unmet | {end} and int(plain[q, 0]) == I["top1"][(r // K, r % K)]
    out = []
    for passes in (0, 1):
        bufs = _select(dev, M, rows, ld, w, mode, K, V, N, b_s, nsrc_d, o, end, t, b_h, T, req_d, met_d, passes, not ens)
        got = []
        for b, what in zip(bufs, ("row values", "row words", "required values", "required words")):
            x = b.read(what)
            assert bool((x[~live].view(torch.int32) == SENT).all()), "%s: rows of dead slots were written" % what
            got.append(x[live])
        gv, gi, grv, gri = got[0], got[1].view(torch.int32), got[2], got[3].view(torch.int32)
        assert torch.equal(gi.long(), ci), "ordinary words differ (passes = %d)" % passes
        assert torch.equal(gri.long(), ri), "required words differ (passes = %d)" % passes
        for q in range(len(lrows)):
            unmet = {wd for c, wd in enumerate(reqs[q]) if not (mets[q] >> c) & 1}
            assert not (set(gi[q].tolist()) & unmet), "an unmet required word among the ordinary candidates"
            assert (end in gi[q].tolist()) == (not unmet and K >= 1 and end not in sets[q]), "<end> and the mask disagree"
        assert bool((grv[gri < 0] == NEG).all()), "an entry without a word must be -inf"
        out.append((gv, gi, grv, gri))
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the staged and the multi-pass launch differ in bits"
    gv, gi, grv, gri = out[0]
    # what must be (-inf, -1): met words, words at index c >= C_n, and (g = 1) the unmet word in the row's history
    for q, r in enumerate(lrows):
        n, j = r // K, r % K
        if n == 0:
            want = {j % 4, (j + 3) % 4} | (set() if (with_opt and g == 1 and t >= 3) else {(j + 1) % 4})
            assert {c for c in range(4) if int(gri[q, c]) >= 0} == want, (n, j, gri[q].tolist())
        else:
            assert gri[q].tolist() == ([-1] * 4 if j == 0 else [-1, I["reqs"][1][1], -1, -1])
    # bit for bit the plain kernel's first output where the required word is the row's top-1
    for passes in (0, 1):
        p_v, p_i = _select(dev, M, rows, ld, w, mode, K, V, N, b_s, nsrc_d, None, end, t, None, T, None, None, passes, not ens,
                           con=False)
        pv, pi = p_v.read("plain values")[live], p_i.read("plain words").view(torch.int32)[live]
        checked = 0
        for q, r in enumerate(lrows):
            c = [c for c in range(4) if int(gri[q, c]) == int(pi[q, 0])]
            if c:
                assert int(grv[q, c[0]].view(torch.int32)) == int(pv[q, 0].view(torch.int32)), (passes, q, c)
                checked += 1
        assert checked >= nsrc[0]
    finite = gri >= 0
    return gv, cv, ci, grv, rv, ri, finite, bv, l64, s64, w


CASES = [(1003, 51, 5, 1), (1003, 51, 0, 0), (1004, 51, 2, 2), (23, 8, 5, 1), (23, 8, 0, 0)]     # V, max_steps, t, g


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("V,T,t,g", CASES)
def test_row_topk_con_vs_fp64(dev, V, T, t, g, K):
    gv, cv, ci, grv, rv, ri, finite, bv, *_ = _case(dev, V, K, 1, 0, g, T, t, ens=False)
    _bound_ok("beam_row_topk_con", "value", gv, cv, bv.gather(1, ci), kind="=2^-24 ((V + 8) + 2 (|score| + |logit| + |lse|))")
    b = bv.gather(1, ri.clamp_min(0))
    _bound_ok("beam_row_topk_con", "required value", torch.where(finite, grv, torch.zeros_like(grv)),
              torch.where(finite, rv, torch.zeros_like(rv)), b, kind="=2^-24 ((V + 8) + 2 (|score| + |logit| + |lse|))")


@pytest.mark.parametrize("V,T,K", [(1003, 51, 3), (23, 8, 8)])
def test_row_topk_con_without_options(dev, V, T, K):
    """opt = NULL: nothing but the requirements is excluded"""
    gv, cv, ci, *_, bv, _, _, _ = _case(dev, V, K, 1, 0, 0, T, 4, ens=False, with_opt=False)
    _bound_ok("beam_row_topk_con (no options)", "value", gv, cv, bv.gather(1, ci), kind="=2^-24 ((V + 8) + 2 (...))")


@pytest.mark.parametrize("M,mode", [(1, 0), (1, 1), (3, 0), (3, 1)])
@pytest.mark.parametrize("V,T,t,g,K", [(1003, 51, 5, 1, 3), (23, 8, 5, 1, 8), (1004, 51, 0, 0, 1)])
def test_row_topk_ens_con_vs_fp64(dev, V, T, t, g, K, M, mode):
    gv, cv, ci, grv, rv, ri, finite, bv, *_ = _case(dev, V, K, M, mode, g, T, t, ens=True)
    _bound_ok("beam_row_topk_ens_con %s" % ("logprob", "prob")[mode], "value", gv, cv, bv.gather(1, ci),
              kind="=ensemble_refs.value_bounds")
    _bound_ok("beam_row_topk_ens_con %s" % ("logprob", "prob")[mode], "required value",
              torch.where(finite, grv, torch.zeros_like(grv)), torch.where(finite, rv, torch.zeros_like(rv)),
              bv.gather(1, ri.clamp_min(0)), kind="=ensemble_refs.value_bounds")


@pytest.mark.parametrize("V", [23, 1003])
def test_no_required_words_is_the_plain_kernel_in_bits(dev, V):
    """every list empty: outv / outi hold the bits of scnattn_beam_row_topk, the required outputs are (-inf, -1)"""
    K, N = 5, 3
    nsrc = [K, 2, 0]
    R, end = N * K, V - 1
    gen = torch.Generator().manual_seed(V)
    x = (torch.randn(R, V, generator=gen) * 3).float()
    x[:, 7] = x[:, 11]
    x[:, end] = 20.0
    live = torch.tensor([j < n for n in nsrc for j in range(K)])
    x[~live] = NAN
    b_l, b_s = GBuf(dev, (R, V), (V + 1, 1), x), GBuf(dev, (R,), None, torch.randn(R, generator=gen))
    nsrc_d, req_d = _ints(dev, nsrc), torch.full((N, 4), -1, dtype=torch.int32, device=dev)
    met_d = torch.zeros(R, dtype=torch.int32, device=dev)
    for passes in (0, 1):
        p_v, p_i = _select(dev, 1, [b_l], V + 1, [1.0], 0, K, V, N, b_s, nsrc_d, None, end, 0, None, 8, None, None, passes, True,
                           con=False)
        for single in (True, False):
            g_v, g_i, g_rv, g_ri = _select(dev, 1, [b_l], V + 1, [1.0], 0, K, V, N, b_s, nsrc_d, None, end, 0, None, 8, req_d,
                                           met_d, passes, single)
            assert torch.equal(g_v.read("v").view(torch.int32), p_v.read("v").view(torch.int32))
            assert torch.equal(g_i.read("i").view(torch.int32), p_i.read("i").view(torch.int32))
            assert bool((g_rv.read("rv")[live] == NEG).all()) and bool((g_ri.read("ri").view(torch.int32)[live] == -1).all())
            assert int(g_i.read("i").view(torch.int32)[0, 0]) == end


def test_selection_refusals(dev):
    V, K, N, T = 80, 2, 1, 51
    x = GBuf(dev, (N * K, V), None, torch.zeros(N * K, V))
    b_s = GBuf(dev, (N * K,), None, torch.zeros(N * K))
    nsrc, req, met = _ints(dev, [1]), _ints(dev, [[50, -1, -1, -1]]), _ints(dev, [0, 0])
    b_h = GBufI(dev, N * K * T, torch.zeros(N * K * T, dtype=torch.int32))

    def go(K=K, V=V, g=0, banned=(), end=None, req=req, met=met, opt=True):
        end = V - 1 if end is None else end
        o = OR.Opts(no_repeat_ngram=g, banned_tokens=banned) if opt else None
        return _select(dev, 1, [x], V, [1.0], 0, K, V, N, b_s, nsrc, o, end, 0, b_h, T, req, met, 0, True)

    bufs = go(g=1, banned=tuple(range(22)))             # 80 - 22 - 1 - 51 - 4 = 2 = K: the boundary is accepted
    assert bufs[3].read("ri").view(torch.int32)[0].tolist() == [50, -1, -1, -1]
    go(opt=False)
    for kw in (dict(g=1, banned=tuple(range(23))), dict(K=0), dict(K=9), dict(end=V), dict(end=-1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            go(**kw)
    for name in ("req", "met"):
        with pytest.raises(RuntimeError):
            _call("scnattn_beam_row_topk_con", dev, N, K, V, x.ptr, V, b_s.ptr, C.c_void_p(nsrc.data_ptr()), None, V - 1, 0,
                  None, T, None if name == "req" else C.c_void_p(req.data_ptr()),
                  None if name == "met" else C.c_void_p(met.data_ptr()), x.ptr, x.ptr, x.ptr, x.ptr, 0)


# ---- the merge ------------------------------------------------------------------------------------------------------------
class State:
    """the 12 state arrays of scnattn_beam_merge_banks and met, each in a guarded window of its own"""

    def __init__(self, dev, host):
        self.host = host
        self.buf = {}
        for name in CR.STATE + ("met",):
            x = host[name].reshape(-1)
            self.buf[name] = GBuf(dev, x.shape, None, x, out=True) if name in FLOATS else GBufI(dev, x.numel(), x)
        self.ptrs = (C.c_void_p * 12)(*[self.buf[name].ptr.value for name in CR.STATE])

    def read(self):
        return {name: self.buf[name].read(name).reshape(self.host[name].shape).to(self.host[name].dtype)
                for name in CR.STATE + ("met",)}


def _merge(dev, host, candv, candi, reqv, reqi, table, N, K, V, end, t):
    st = State(dev, host)
    cv, rv = GBuf(dev, candv.shape, None, candv), GBuf(dev, reqv.shape, None, reqv)
    ci, ri, tb = candi.to(dev), reqi.to(dev), table.to(dev)
    _call("scnattn_beam_merge_banks", dev, N, K, V, end, t, cv.ptr, C.c_void_p(ci.data_ptr()), rv.ptr,
          C.c_void_p(ri.data_ptr()), C.c_void_p(tb.data_ptr()), st.buf["met"].ptr, st.ptrs)
    return st.read()


def _same(got, want, where):
    for name in CR.STATE + ("met",):
        assert torch.equal(got[name], want[name]), (where, name, got[name].tolist(), want[name].tolist())


REQ = [20, 21, 22, 23]


def _merge_inputs(g, N, K, V, T, t, Cs, nsrcs):
    """Image n has Cs[n] required words (REQ[:C]) and nsrcs[n] live sources (0: finished, its candidates NaN).  A live row has a
    random mask, K distinct ordinary words of a pool of ten (<end> among them only where the mask is complete), and offers
    its unmet required words.  Values in {0, -1/4, .., -3}: ties within and across rows and banks."""
    end, R = V - 1, N * K
    pool = list(range(9)) + [end]
    candv, candi = torch.full((R, K), NAN), torch.zeros(R, K, dtype=torch.int32)
    reqv, reqi = torch.full((R, 4), NAN), torch.full((R, 4), -1, dtype=torch.int32)
    met = torch.zeros(R, dtype=torch.int32)
    table = torch.full((N, 4), -1, dtype=torch.int32)
    for n in range(N):
        C_n = Cs[n]
        table[n, :C_n] = torch.tensor(REQ[:C_n], dtype=torch.int32)
        for j in range(nsrcs[n]):
            r = n * K + j
            m = int(torch.randint(0, 1 << C_n, (1,), generator=g)) if (C_n and t > 0) else 0
            if j == 0 and C_n and t > 0:
                m = (1 << C_n) - 1                       # one row that may end
            met[r] = m
            mine = pool if m == (1 << C_n) - 1 else pool[:9]     # <end> only where the mask is complete
            words = [mine[i] for i in torch.randperm(len(mine), generator=g)[:K].tolist()]
            vals = (-0.25 * torch.randint(0, 13, (K,), generator=g)).tolist()
            order = sorted(range(K), key=lambda q: (-vals[q], words[q]))
            candv[r] = torch.tensor([vals[q] for q in order])
            candi[r] = torch.tensor([words[q] for q in order], dtype=torch.int32)
            reqv[r] = NEG
            for c in range(C_n):
                if not (m >> c) & 1 and float(torch.rand(1, generator=g)) < 0.85:
                    reqv[r, c], reqi[r, c] = -0.25 * int(torch.randint(0, 13, (1,), generator=g)), REQ[c]
    kk = list(nsrcs)
    ncomp = [K - k if t > 0 else 0 for k in kk]
    if t == 0:
        kk = [K if k else 0 for k in kk]
        ncomp = [0 if k else K for k in kk]
    comp_score, comp_step = torch.zeros(R), torch.full((R,), -1, dtype=torch.int32)
    for n in range(N):
        for q in range(ncomp[n]):
            comp_score[n * K + q], comp_step[n * K + q] = -0.5 - 0.25 * q, 0
    host = {"open_images": torch.tensor([sum(1 for k in kk if k)], dtype=torch.int32),
            "nsrc": torch.tensor(nsrcs, dtype=torch.int32), "kk": torch.tensor(kk, dtype=torch.int32),
            "ncomp": torch.tensor(ncomp, dtype=torch.int32),
            "best_idx": torch.tensor([0 if c else -1 for c in ncomp], dtype=torch.int32),
            "best_score": torch.tensor([-0.5 if c else 0.0 for c in ncomp]),
            "scores": -0.125 * torch.randint(0, 9, (R,), generator=g).float(), "comp_score": comp_score, "comp_step": comp_step,
            "comp_parent": torch.zeros(R, dtype=torch.int32), "token": torch.full((T, R), -7, dtype=torch.int32),
            "parent": torch.full((T, R), -7, dtype=torch.int32), "met": met}
    return host, candv, candi, reqv, reqi, table


@pytest.mark.parametrize("V", [30, 1003])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_merge_banks_is_exact_on_hand_made_candidates(dev, K, V):
    """N = 5 images: 4 required words and all K sources live (K = 8: 96 candidates); 2 words and kk < K; a finished image;
    no required word (the plain merge); 1 word and one live source.  Every array of the state and met EQUAL to the
    restatement's, records of other steps and all guard words untouched.  Several seeds: <end> picks at every rank."""
    N, T, t, end = 5, 3, 1, V - 1
    ends = set()
    for seed in range(6):
        g = torch.Generator().manual_seed(1000 * seed + 10 * K + V)
        nsrcs = [K, max(K - 2, 1), 0, K, 1]
        host, candv, candi, reqv, reqi, table = _merge_inputs(g, N, K, V, T, t, [4, 2, 3, 0, 1], nsrcs)
        want = CR.merge_state(host, candv, candi, reqv, reqi, table, N, K, V, end, t)
        got = _merge(dev, host, candv, candi, reqv, reqi, table, N, K, V, end, t)
        _same(got, want, (K, V, seed))
        assert bool((got["token"][0] == -7).all()) and bool((got["token"][2] == -7).all())
        for n in range(N):
            new = int(got["ncomp"][n]) - int(host["ncomp"][n])
            if new:
                ends.add(new)
        # the image without required words (image 3): what scnattn_beam_merge writes from the same candidates
        from test_gpu_diverse_beam_kernels import State as PlainState
        ps = PlainState(dev, {k: v for k, v in host.items() if k != "met"})
        cvb, cib = GBuf(dev, candv.shape, None, candv), candi.to(dev)
        _call("scnattn_beam_merge", dev, N, K, V, end, t, cvb.ptr, C.c_void_p(cib.data_ptr()), ps.ptrs)
        pm = ps.read()
        r0 = 3 * K
        for name in ("token", "parent"):
            assert torch.equal(pm[name][t, r0:r0 + K], got[name][t, r0:r0 + K]), name
        for name in ("scores", "comp_score", "comp_step", "comp_parent"):
            assert torch.equal(pm[name][r0:r0 + K], got[name][r0:r0 + K]), name
        for name in ("nsrc", "kk", "ncomp", "best_idx", "best_score"):
            assert torch.equal(pm[name][3], got[name][3]), name
    assert ends, "no seed picked <end>"


def test_merge_banks_first_step_and_hand_worked_picks(dev):
    """t = 0 (one live source, kk = K, masks 0): the round-robin gives every required word a beam; then the hand-worked cases
    of tests/test_constrained_beam_refs.py through the kernel: <end> at ranks 0 and 2, a bank that runs dry, ties"""
    V, end = 100, 99
    for K in (1, 5, 8):
        g = torch.Generator().manual_seed(40 + K)
        host, candv, candi, reqv, reqi, table = _merge_inputs(g, 2, K, V, 2, 0, [4, 1], [1, 1])
        reqv[0], reqi[0] = torch.tensor([-3.0, -2.0, -3.0, -1.0]), torch.tensor(REQ, dtype=torch.int32)
        want = CR.merge_state(host, candv, candi, reqv, reqi, table, 2, K, V, end, 0)
        got = _merge(dev, host, candv, candi, reqv, reqi, table, 2, K, V, end, 0)
        _same(got, want, ("first step", K))
        # bank 1 in order: word 3 (-1.0), word 1 (-2.0), word 0 (-3.0), word 2 (-3.0); banks 1 and 0 take turns
        assert sorted(x for x in got["met"][:K].tolist() if x) == {1: [8], 5: [1, 2, 8], 8: [1, 2, 4, 8]}[K]
        if K == 1:
            assert int(got["token"][0, 0]) == REQ[3]

    def state(K, nsrc, kk, met, ncomp=0):
        R = K
        return {"open_images": torch.tensor([1], dtype=torch.int32), "nsrc": torch.tensor([nsrc], dtype=torch.int32),
                "kk": torch.tensor([kk], dtype=torch.int32), "ncomp": torch.tensor([ncomp], dtype=torch.int32),
                "best_idx": torch.tensor([-1], dtype=torch.int32), "best_score": torch.zeros(1), "scores": torch.zeros(R),
                "comp_score": torch.zeros(R), "comp_step": torch.full((R,), -1, dtype=torch.int32),
                "comp_parent": torch.zeros(R, dtype=torch.int32), "token": torch.full((1, R), -7, dtype=torch.int32),
                "parent": torch.full((1, R), -7, dtype=torch.int32), "met": torch.tensor(met, dtype=torch.int32)}

    def rows(spec, K):
        cv, ci = torch.full((K, K), NAN), torch.zeros(K, K, dtype=torch.int32)
        rv, ri = torch.full((K, 4), NAN), torch.full((K, 4), -1, dtype=torch.int32)
        for j, (o, r) in enumerate(spec):
            cv[j], ci[j] = torch.tensor([v for v, _ in o]), torch.tensor([wd for _, wd in o], dtype=torch.int32)
            rv[j] = torch.tensor([NEG if x is None else x[0] for x in r])
            ri[j] = torch.tensor([-1 if x is None else x[1] for x in r], dtype=torch.int32)
        return cv, ci, rv, ri

    # <end> at rank 2 (and recorded), kk = 3
    K = 3
    spec = [([(-1.0, 5), (-2.0, 6), (-3.0, 7)], [(-4.0, 42), None, None, None]), ([(-1.5, 8), (-2.5, 99), (-3.5, 9)], [None] * 4)]
    tb = torch.tensor([[42, -1, -1, -1]], dtype=torch.int32)
    host = state(K, 2, 3, [0, 1, 0])
    got = _merge(dev, host, *rows(spec, K), tb, 1, K, V, end, 0)
    _same(got, CR.merge_state(host, *rows(spec, K), tb, 1, K, V, end, 0), "end at rank 2")
    assert got["token"][0].tolist() == [5, 8, 5] and got["parent"][0].tolist() == [0, 1, 0] and got["met"].tolist() == [0, 1, 0]
    assert got["comp_score"].tolist()[0] == -2.5 and int(got["comp_parent"][0]) == 1 and int(got["kk"]) == 2
    # <end> at rank 0: row 1's <end> raised above everything
    spec[1] = ([(-0.5, 99), (-1.5, 8), (-3.5, 9)], [None] * 4)
    host = state(K, 2, 3, [0, 1, 0])
    got = _merge(dev, host, *rows(spec, K), tb, 1, K, V, end, 0)
    _same(got, CR.merge_state(host, *rows(spec, K), tb, 1, K, V, end, 0), "end at rank 0")
    assert got["comp_score"].tolist()[0] == -0.5 and got["token"][0].tolist() == [5, 8, 5] and got["scores"].tolist() == [-1.0, -1.5, 0.0]
    # kk < K: the highest bank first
    host = state(K, 2, 1, [0, 1, 0], ncomp=2)
    got = _merge(dev, host, *rows(spec, K), tb, 1, K, V, end, 0)
    assert int(got["ncomp"]) == 3 and int(got["kk"]) == 0 and int(got["open_images"]) == 0
    again = _merge(dev, got, *rows(spec, K), tb, 1, K, V, end, 0)          # a finished image: a no-op
    _same(again, got, "finished image")
    # a bank that runs dry, four required words
    K = 4
    spec = [([(-1.0, 10), (-2.0, 11), (-3.0, 12), (-3.5, 13)], [None, None, (-5.0, 52), (-0.5, 53)])]
    tb = torch.tensor([[50, 51, 52, 53]], dtype=torch.int32)
    host = state(K, 1, 4, [0b0011, 0, 0, 0])
    got = _merge(dev, host, *rows(spec, K), tb, 1, K, V, end, 0)
    assert got["token"][0].tolist() == [53, 10, 11, 52] and got["met"].tolist() == [0b1011, 0b0011, 0b0011, 0b0111]
    # ties across rows and banks
    K = 2
    row = ([(-1.0, 7), (-2.0, 8)], [(-1.0, 3), None, None, None])
    tb = torch.tensor([[3, -1, -1, -1]], dtype=torch.int32)
    host = state(K, 2, 2, [0, 0])
    got = _merge(dev, host, *rows([row, row], K), tb, 1, K, V, end, 0)
    assert got["token"][0].tolist() == [3, 7] and got["parent"][0].tolist() == [0, 0] and got["met"].tolist() == [1, 0]


def test_merge_banks_refusals(dev):
    V, K = 30, 3
    g = torch.Generator().manual_seed(1)
    host, candv, candi, reqv, reqi, table = _merge_inputs(g, 1, K, V, 1, 0, [2], [1])
    for k in (0, 9):
        with pytest.raises(RuntimeError):
            _merge(dev, host, candv, candi, reqv, reqi, table, 1, k, V, V - 1, 0)
    st = State(dev, host)
    with pytest.raises(RuntimeError):       # met is NULL
        _call("scnattn_beam_merge_banks", dev, 1, K, V, V - 1, 0, GBuf(dev, candv.shape, None, candv).ptr,
              C.c_void_p(candi.to(dev).data_ptr()), GBuf(dev, reqv.shape, None, reqv).ptr,
              C.c_void_p(reqi.to(dev).data_ptr()), C.c_void_p(table.to(dev).data_ptr()), None, st.ptrs)
