"""The kernels of the search OPTIONS (csrc/beam.hip: the selection with exclusions, the advance with the history) through
the C ABI, one launch per call, against the fp64 restatement of tests/beam_options_refs.py; buffers are guarded windows
(tests/kernel_harness.py: sentinel around outputs, NaN around inputs and in the rows of dead slots).

How a case is judged (the value judge and guard bands of tests/test_gpu_beam_kernels.py):
  * selection: every live row has its own history, built so that the rule FIRES ON THE ROW'S BEST WORDS -- asserted: in
    every case an excluded word sits in the plain top K of a live row, so a kernel that ignored the bitmap fails.  Inputs
    are drawn from a fixed seed list until the fp64 top K+1 of every live row AFTER exclusion and the merged top kk+1 are
    separated by at least 64 x the value bound (2^-24 ((V + 8) + 2 (|score| + |logit| + |lse|)); the ensemble:
    ensemble_refs.value_bounds) -- asserted on the CPU before the kernel is called; then the words must be EQUAL and the
    values within the bound.  The staged and the multi-pass (force_passes) launch must agree bit for bit.
  * nothing excluded: the bits of scnattn_beam_row_topk / _ens, also across the staging threshold the bitmap moves.
  * exact ties: equal values leave in index order with the excluded ones skipped; <end> at t = min_length - 1 / min_length.
  * advance: exact (a gather); dead slots a copy of slot 0; nothing written behind the history."""
import ctypes as C

import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
import ensemble_refs as ER
from kernel_harness import GBuf, GBufI, NAN, SENT, SENTI, U, _bound_ok, _call, _write_report  # noqa: F401  (the fixture)
from test_gpu_decoder_kernels import _gen

pytestmark = pytest.mark.gpu
REPORT_TITLE = "beam-search selection with exclusions vs fp64: worst |got - ref| / bound over all cases"
T = 51
WEIGHTS = {1: None, 3: (0.5, 0.3, 0.2)}


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
    got = buf.read(what)
    dead = got[~live].view(torch.int32)
    assert bool((dead == SENT).all()), "%s: %d words of dead slots were written" % (what, int((dead != SENT).sum()))
    return got[live]


def _copts(o):
    from scnattn._lib import SearchOpts
    c = SearchOpts(min_length=o.min_length, no_repeat_ngram=o.no_repeat_ngram, n_banned=len(o.banned_tokens))
    for i, b in enumerate(o.banned_tokens):
        c.banned[i] = b
    return c


def _select(dev, M, rows, lds, w, mode, K, V, N, b_s, nsrc_d, o, end, t, b_h, passes, single=False):
    """one launch of the selection with exclusions -> (values, words int32) windows read back, guards checked"""
    R = N * K
    b_v, b_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
    co = _copts(o)
    hp = b_h.ptr if b_h is not None else None
    if single:
        _call("scnattn_beam_row_topk_opt", dev, N, K, V, rows[0].ptr, lds[0], b_s.ptr, C.c_void_p(nsrc_d.data_ptr()),
              C.byref(co), end, t, hp, T, b_v.ptr, b_i.ptr, passes)
    else:
        pl = (C.c_void_p * M)(*[r.ptr.value for r in rows])
        ll = (C.c_long * M)(*lds)
        wl = (C.c_float * M)(*w)
        _call("scnattn_beam_row_topk_ens_opt", dev, N, K, V, M, pl, ll, wl, mode, b_s.ptr, C.c_void_p(nsrc_d.data_ptr()),
              C.byref(co), end, t, hp, T, b_v.ptr, b_i.ptr, passes)
    if b_h is not None:
        b_h.read("history")             # an input: its margins must be intact as well
    return b_v, b_i


def _history(head, t, g, gen):
    """t words over the row's best words, such that the rule (when it fires) excludes the row's BEST head word: periodic
    with period g + 1, phased so that the best word continues the period at position t; g <= 1: drawn from them at
    random, the best word last"""
    pool = head[-min(max(g, 1) + 1, len(head)):]
    if g <= 1:
        return ([pool[int(torch.randint(0, len(pool), (1,), generator=gen))] for _ in range(t - 1)] + [pool[-1]])[:t]
    return [pool[(i - t - 1) % len(pool)] for i in range(t)]


def _draw(V, K, M, w, mode, nsrc, kk, o, end, t, g, seed0, ens_bound):
    """M logits [K,V], scores [K] and K histories of ONE image: a head of min(3K + 2, V - 1) words above the bulk in every
    row (the same words for every member), <end> above the head while the options exclude it, until the fp64 top K+1 of
    every live row after exclusion and the merged top kk+1 are separated by >= 64 x the bound.  Where `o` bans nothing
    yet, two words are banned: the best (K = 1) or second-best head word of row 0, and a word of the bulk.
    -> (logits, scores, hists, sets, o)"""
    for seed in range(seed0, seed0 + 50):
        gen = _gen(seed)
        logits = [(torch.randn(K, V, generator=gen) * 3).float() for _ in range(M)]
        hists, heads = [], []
        for j in range(K):
            nh = min(3 * K + 2, V - 1)
            head = torch.randperm(V - 1, generator=gen)[:nh]            # <end> = V - 1 is not a head word
            for m in range(M):
                logits[m][j, head] = 12.0 + (0.5 + 0.1 * m) * torch.arange(nh) + 0.2 * torch.rand(nh, generator=gen)
                if t < o.min_length:
                    logits[m][j, end] = 13.0 + (0.5 + 0.1 * m) * nh + 0.2 * float(torch.rand(1, generator=gen))
            heads.append(head.tolist())
            hists.append(_history(heads[j], t, g, gen))
        scores = (torch.randn(K, generator=gen) * 2).float()
        oo = o
        if not o.banned_tokens:
            bulk = next(v for v in range(V - 1) if v not in heads[0])
            oo = o._replace(banned_tokens=tuple(sorted({heads[0][-1 if K == 1 else -2], bulk})))
        sets = [OR.excluded(hists[j], t, V, end, oo) for j in range(nsrc)]
        l64, s64 = [x.double()[:nsrc] for x in logits], scores.double()[:nsrc]
        val = s64.unsqueeze(1) + ER.combine(l64, w, mode)
        K1 = min(K + 1, V - max(len(s) for s in sets))
        cv, ci = OR.row_topk_excl(val, sets, K1)
        if ens_bound:
            bv = ER.value_bounds(l64, w, mode, s64)[1]
        else:
            lse = torch.logsumexp(l64[0], dim=1, keepdim=True)
            bv = U * ((V + 8) + 2 * (s64.abs().unsqueeze(1) + l64[0].abs() + lse.abs()))
        bound = float(bv.gather(1, ci).max())
        picks = BR.merge(cv[:, :K], ci[:, :K], V, min(kk + 1, nsrc * K))
        gaps = [picks[i][0] - picks[i + 1][0] for i in range(len(picks) - 1)]
        rowgaps = float((cv[:, :-1] - cv[:, 1:]).min()) if K1 > 1 else 1.0
        if all(gp >= 64 * bound for gp in gaps) and rowgaps >= 64 * bound:
            return logits, scores, hists, sets, oo
    raise AssertionError("no seed separates the candidates")


def _case(dev, V, K, M, mode, g, t, ens, ld_extra=3):
    """three images: all K sources live; nsrc < K; a finished image.  Both launches; -> what the caller compares further"""
    end = V - 1
    nsrc = [K, max(K - 2, 1), 0]
    kk = [K, max(K - 2, 1), 0]
    N, R = 3, 3 * K
    w = ER.member_weights(WEIGHTS[M], M) if ens else [1.0]
    min_length = t + 1 if (t + g) % 2 == 0 and t < T - 1 else t         # <end>, the best word of every row: out / in
    o = OR.Opts(min_length=min_length, no_repeat_ngram=g)              # image 0's draw adds the banned words
    logits = [torch.zeros(N, K, V) for _ in range(M)]
    scores = torch.zeros(N, K)
    hist = torch.full((N, K, T), -1, dtype=torch.int32)                 # dead rows / entries past t: never read
    sets = []
    for n in range(2):
        lg, scores[n], hs, st, o = _draw(V, K, M, w, mode, nsrc[n], kk[n], o, end, t, g, 100 * V + 10 * K + n + 1000 * g + t,
                                         ens)
        for m in range(M):
            logits[m][n] = lg[m]
        for j in range(K):
            hist[n, j, :t] = torch.tensor(hs[j], dtype=torch.int32)
        sets += st
    assert OR.refusal(o, V, K, T, end) is None and len(o.banned_tokens) == 2
    live = _live(nsrc, K)
    ld = V + ld_extra
    rows = []
    for m in range(M):
        x = logits[m].reshape(R, V).clone()
        x[~live] = NAN
        rows.append(GBuf(dev, (R, V), (ld, 1), x))
    b_s = GBuf(dev, (R,), None, scores.reshape(R))
    b_h = GBufI(dev, R * T, hist.reshape(-1))
    nsrc_d = _ints(dev, nsrc)
    l64 = [x.reshape(R, V).double()[live] for x in logits]
    s64 = scores.reshape(R).double()[live]
    val = s64.unsqueeze(1) + ER.combine(l64, w, mode)
    cv, ci = OR.row_topk_excl(val, sets, K)
    plain = torch.sort(-val, dim=1, stable=True)[1][:, :K]
    assert any(set(plain[r].tolist()) & sets[r] for r in range(len(sets))), "the exclusions do not touch any top K"
    out = []
    for passes in (0, 1):
        b_v, b_i = _select(dev, M, rows, [ld] * M, w, mode, K, V, N, b_s, nsrc_d, o, end, t, b_h, passes, single=not ens)
        gv = _untouched(b_v, live, "row values")
        gi = _untouched(b_i, live, "row words").view(torch.int32)
        assert torch.equal(gi.long(), ci), "row top-K words differ (passes = %d)" % passes
        out.append((gv, gi))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)) and torch.equal(out[0][1], out[1][1]), \
        "the staged and the multi-pass launch differ in bits"
    return out[0][0], cv, ci, l64, s64, w


GT = [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (8, 7), (8, 8), (1, 50), (2, 50), (3, 50), (8, 50)]


@pytest.mark.parametrize("g,t", GT)
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("V", [67, 1003, 1004])
def test_row_topk_opt_vs_fp64(dev, V, K, g, t):
    """the single decoder; histories of length t in {0, 1, g - 1, g, 50}; V odd (scalar tail) and a multiple of 4"""
    gv, cv, ci, l64, s64, _ = _case(dev, V, K, 1, 0, g, t, ens=False, ld_extra=3 if V % 2 else 4)
    lse = torch.logsumexp(l64[0], dim=1)
    bound = U * ((V + 8) + 2 * (s64.abs().unsqueeze(1) + l64[0].gather(1, ci).abs() + lse.abs().unsqueeze(1)))
    _bound_ok("beam_row_topk_opt", "value", gv, cv, bound, kind="=2^-24 ((V + 8) + 2 (|score| + |logit| + |lse|))")


@pytest.mark.parametrize("g,t", [(2, 50), (3, 3), (1, 1)])
@pytest.mark.parametrize("M,mode", [(1, 0), (1, 1), (3, 0), (3, 1)])
@pytest.mark.parametrize("V,K", [(67, 8), (1003, 3), (1004, 1)])
def test_row_topk_ens_opt_vs_fp64(dev, V, K, M, mode, g, t):
    gv, cv, ci, l64, s64, w = _case(dev, V, K, M, mode, g, t, ens=True, ld_extra=5 if V % 2 else 4)
    _, bv = ER.value_bounds(l64, w, mode, s64)
    _bound_ok("beam_row_topk_ens_opt %s" % ("logprob", "prob")[mode], "value", gv, cv, bv.gather(1, ci),
              kind="=ensemble_refs.value_bounds")


# 15800 / 15900: the row with its bitmap and history just fits / no longer fits the 64 KiB of LDS, where the plain kernel
# still stages (16 + V floats): the staging threshold moved by the bitmap's size
@pytest.mark.parametrize("V", [1003, 15800, 15900])
def test_nothing_excluded_is_beam_row_topk_in_bits_and_one_member_is_the_single_kernel(dev, V):
    K, N = 5, 3
    nsrc = [K, 2, 0]
    R, end = N * K, V - 1
    gen = _gen(V)
    x = (torch.randn(R, V, generator=gen) * 3).float()
    x[:, 7] = x[:, 11]                  # ties inside a row do not disturb the identity
    hist = torch.randint(0, V - 1, (R, T), generator=gen).int()
    for r in range(R):                  # a head of 16 words >= 0.3 apart, far above the bulk; two of them in the history
        head = torch.randperm(V - 1, generator=gen)[:16]
        x[r, head] = 15.0 + 0.5 * torch.arange(16) + 0.2 * torch.rand(16, generator=gen)
        hist[r, 2], hist[r, 6] = int(head[15]), int(head[12])
    x[:, V - 1] = 30.0                  # ... and <end> above them
    sc = (torch.randn(R, generator=gen) * 2).float()
    live = _live(nsrc, K)
    x[~live] = NAN
    ld = V + 1
    b_l, b_s = GBuf(dev, (R, V), (ld, 1), x), GBuf(dev, (R,), None, sc)
    nsrc_d = _ints(dev, nsrc)
    b_h = GBufI(dev, R * T, hist.reshape(-1))
    top = torch.sort(-x[live].double(), dim=1, stable=True)[1][:, :K]
    some = OR.Opts(min_length=9, no_repeat_ngram=1, banned_tokens=(int(top[0, 2]), int(top[1, 3])))      # head words
    for passes in (0, 1):
        r_v, r_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
        _call("scnattn_beam_row_topk", dev, N, K, V, b_l.ptr, ld, b_s.ptr, C.c_void_p(nsrc_d.data_ptr()), r_v.ptr, r_i.ptr, passes)
        want_v, want_i = r_v.read("values").view(torch.int32), r_i.read("words").view(torch.int32)
        # options that exclude nothing at this step: g = 3 at t = 2, min_length = t, no bans
        for o, t in ((OR.Opts(), 0), (OR.Opts(min_length=2, no_repeat_ngram=3), 2)):
            for single in (True, False):
                b_v, b_i = _select(dev, 1, [b_l], [ld], [1.0], 0, K, V, N, b_s, nsrc_d, o, end, t, b_h, passes, single=single)
                assert torch.equal(b_v.read("values").view(torch.int32), want_v), (passes, t, single)
                assert torch.equal(b_i.read("words").view(torch.int32), want_i), (passes, t, single)
    # with exclusions: staged == multi-pass in bits, one member == the single entry point, no excluded word is picked
    got = []
    for passes in (0, 1):
        for single in (True, False):
            b_v, b_i = _select(dev, 1, [b_l], [ld], [1.0], 0, K, V, N, b_s, nsrc_d, some, end, 8, b_h, passes, single=single)
            got.append((b_v.read("values").view(torch.int32), b_i.read("words").view(torch.int32)))
    assert all(torch.equal(a[0], got[0][0]) and torch.equal(a[1], got[0][1]) for a in got[1:])
    words = got[0][1][live]
    sets = [OR.excluded(hist[r].tolist(), 8, V, end, some) for r in torch.nonzero(live).reshape(-1).tolist()]
    want = OR.row_topk_excl(sc[live].double().unsqueeze(1) + x[live].double() - torch.logsumexp(x[live].double(), 1, True),
                            sets, K)[1]
    assert all(len(s) >= 4 for s in sets) and torch.equal(words.long(), want)       # gaps >= 0.3: no tolerance needed


def test_exact_ties_and_the_min_length_boundary(dev):
    """equal logits: the excluded lower index is skipped and the next index wins; <end> as the arg-max is skipped at
    t = min_length - 1 and taken at t = min_length; in the staged and in the multi-pass launch"""
    V, K, N = 67, 4, 1                  # 67 - 3 - 1 - 51 >= 4: the smallest V of this file passes the candidate-count rule
    end = V - 1
    row = torch.linspace(-2, 1, V)
    row[[3, 9, 20]] = 2.5
    row[[5, 6]] = 2.0
    logits = torch.stack([row, row, torch.full((V,), NAN), torch.full((V,), NAN)])
    scores = torch.tensor([-1.25, -1.25, 0.0, 0.0])
    nsrc = _ints(dev, [2])
    b_l, b_s = GBuf(dev, (K, V), None, logits), GBuf(dev, (K,), None, scores)
    hist = torch.full((K, T), -1, dtype=torch.int32)
    hist[0, 0], hist[1, 0] = 9, 20                   # t = 1: row 0 has emitted word 9, row 1 word 20
    b_h = GBufI(dev, K * T, hist.reshape(-1))
    V2 = 1003
    wide = torch.full((1, V2), -1.0)
    wide[0, V2 - 1] = 4.0                            # <end> is the arg-max
    wide[0, [10, 500]] = 3.0
    b_w, b_ws = GBuf(dev, (1, V2), None, wide), GBuf(dev, (1,), None, torch.zeros(1))
    one = _ints(dev, [1])
    for passes in (0, 1):
        for single in (True, False):
            def words(o, t, h=b_h):
                b_v, b_i = _select(dev, 1, [b_l], [V], [1.0], 0, K, V, N, b_s, nsrc, o, end, t, h, passes, single=single)
                gi = b_i.read("words").view(torch.int32)
                assert bool((gi[2:] == SENT).all())
                return gi[:2].tolist(), b_v.read("values")

            assert words(OR.Opts(), 0)[0] == [[3, 9, 20, 5]] * 2
            assert words(OR.Opts(banned_tokens=(3,)), 0)[0] == [[9, 20, 5, 6]] * 2
            assert words(OR.Opts(banned_tokens=(3, 20, 5)), 0)[0] == [[9, 6, 66, 65]] * 2
            got, gv = words(OR.Opts(no_repeat_ngram=1), 1)
            assert got == [[3, 20, 5, 6], [3, 9, 5, 6]]          # each row skips ITS OWN word
            assert float(gv[0, 0]) == float(gv[0, 1]) == float(gv[1, 1]) and float(gv[0, 1]) > float(gv[0, 2])
            assert words(OR.Opts(no_repeat_ngram=2), 1)[0] == [[3, 9, 20, 5]] * 2        # t < g: nothing yet
            for t, want in ((4, [10, 500, 0]), (5, [V2 - 1, 10, 500])):
                b_v, b_i = _select(dev, 1, [b_w], [V2], [1.0], 0, 3, V2, 1, b_ws, one, OR.Opts(min_length=5), V2 - 1, t, None,
                                   passes, single=single)
                gi = b_i.read("words").view(torch.int32)
                assert gi[0].tolist() == want and bool((gi[1:] == SENT).all()), (t, passes, single)


@pytest.mark.parametrize("t", [0, 1, 50])
def test_advance_opt_is_exact(dev, t):
    """h / c / emb as beam_advance; history rows: the parent's first t words, then the step's word, nothing behind; dead
    slots (parent / token records copied from slot 0, as beam_merge leaves them) get slot 0's history"""
    g = _gen(5 + t)
    N, K, D, M, V = 3, 5, 37, 19, 23
    R = N * K
    h, c, table = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g), torch.randn(V, M, generator=g)
    parent = torch.randint(0, K, (R,), generator=g).int()
    token = torch.randint(0, V, (R,), generator=g).int()
    nopen = [K, 2, 0]
    for n in range(N):                      # dead slots: slot 0's records (zeros where nothing is open)
        for s in range(nopen[n], K):
            parent[n * K + s] = parent[n * K] if nopen[n] else 0
            token[n * K + s] = token[n * K] if nopen[n] else 0
    src = torch.randint(0, V, (R, T), generator=g).int()
    b_h, b_c, b_t = GBuf(dev, h.shape, None, h), GBuf(dev, c.shape, None, c), GBuf(dev, table.shape, None, table)
    b_hd, b_cd, b_e = (GBuf(dev, s, None, out=True) for s in ((R, D), (R, D), (R, M)))
    b_src, b_dst = GBufI(dev, R * T, src.reshape(-1)), GBufI(dev, R * T)
    pd, td = parent.to(dev), token.to(dev)
    _call("scnattn_beam_advance_opt", dev, N, K, D, M, V, t, T, b_h.ptr, b_c.ptr, C.c_void_p(pd.data_ptr()),
          C.c_void_p(td.data_ptr()), b_t.ptr, b_src.ptr, b_dst.ptr, b_hd.ptr, b_cd.ptr, b_e.ptr)
    h2, c2, emb = BR.advance(h, c, parent.tolist(), token.long().tolist(), table, K)
    assert torch.equal(b_hd.read("h"), h2) and torch.equal(b_cd.read("c"), c2) and torch.equal(b_e.read("emb"), emb)
    assert torch.equal(b_src.read("history in"), src.reshape(-1))
    dst = b_dst.read("history out").view(R, T)
    rows = (torch.arange(R) // K) * K + parent.long()
    assert torch.equal(dst[:, :t], src[rows][:, :t]) and torch.equal(dst[:, t], token)
    assert bool((dst[:, t + 1:] == SENTI).all()), "entries behind the step's word were written"
    for n in range(N):
        for s in range(max(nopen[n], 1), K):
            assert torch.equal(dst[n * K + s], dst[n * K]), "a dead slot is not a copy of slot 0"


def test_refusals(dev):
    V, K, N = 80, 2, 1
    x = GBuf(dev, (N * K, V), None, torch.zeros(N * K, V))
    b_s = GBuf(dev, (N * K,), None, torch.zeros(N * K))
    nsrc = _ints(dev, [1])
    b_h = GBufI(dev, N * K * T, torch.zeros(N * K * T, dtype=torch.int32))
    b_v, b_i = GBuf(dev, (N * K, K), None, out=True), GBuf(dev, (N * K, K), None, out=True)
    from scnattn._lib import SearchOpts

    def go(K=K, V=V, g=0, min_length=0, banned=(), n_banned=None, end=None, t=0, hist=b_h, Tm=T, opt=True):
        end = V - 1 if end is None else end
        co = SearchOpts(min_length=min_length, no_repeat_ngram=g, n_banned=len(banned) if n_banned is None else n_banned)
        for i, b in enumerate(banned):
            co.banned[i] = b
        _call("scnattn_beam_row_topk_opt", dev, N, K, V, x.ptr, V, b_s.ptr, C.c_void_p(nsrc.data_ptr()),
              C.byref(co) if opt else None, end, t, hist.ptr if hist is not None else None, Tm, b_v.ptr, b_i.ptr, 0)

    go(g=2, min_length=3, banned=(5,))                      # the arguments the refusals below vary are fine
    bad = [dict(g=9), dict(g=-1), dict(min_length=-1), dict(min_length=T), dict(n_banned=65), dict(n_banned=-1),
           dict(banned=(V,)), dict(banned=(-1,)), dict(banned=(V - 1,)), dict(end=V), dict(end=-1), dict(end=5, banned=(5,)), dict(t=-1), dict(t=T + 1),
           dict(g=1, hist=None), dict(Tm=0), dict(opt=False), dict(K=0), dict(K=9),
           dict(g=1, V=53), dict(banned=tuple(range(64)), V=66), dict(g=1, banned=tuple(range(27)))]      # < K candidates
    for kw in bad:
        with pytest.raises(RuntimeError, match="invalid argument"):
            go(**kw)
    go(g=1, banned=tuple(range(26)))                        # 80 - 26 - 1 - 51 = 2 = K: the boundary is accepted
    assert int(b_i.read("words").view(torch.int32)[0, 0]) == 26
