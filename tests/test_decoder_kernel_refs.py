"""The fp64 references of the decode-step primitives (tests/decoder_kernel_refs.py) against the oracle.

The GPU tests of tests/test_gpu_decoder_kernels.py compare every kernel with these references; here the references,
composed in the order scnattn/functional.py composes the C calls, must reproduce oracle/scnattn_ref.py (pinned by the
golden vectors) and its autograd gradients in fp64, at a size where nothing is a multiple of 4.  Runs without a GPU."""
import pytest
import torch

import decoder_kernel_refs as K
from oracle import scnattn_ref as R

TOL = 1e-12


def _close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert a.shape == b.shape and err <= TOL, "%s: %.3e" % (what, err)


def test_attention_references_reproduce_the_oracle_and_its_autograd():
    g = torch.Generator().manual_seed(11)
    B, P, A, E, D = 3, 13, 10, 22, 14
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    prm = {"encoder_att.weight": rnd(A, E) * 0.3, "encoder_att.bias": rnd(A) * 0.1, "decoder_att.weight": rnd(A, D) * 0.3,
           "decoder_att.bias": rnd(A) * 0.1, "full_att.weight": rnd(1, A), "full_att.bias": rnd(1)}
    prm = {k: v.requires_grad_(True) for k, v in prm.items()}
    enc, h = rnd(B, P, E).requires_grad_(True), rnd(B, D).requires_grad_(True)
    dawe, dalpha = rnd(B, E), rnd(B, P)
    awe_o, alpha_o = R.attention_forward(prm, "", enc, h)
    ((awe_o * dawe).sum() + (alpha_o * dalpha).sum()).backward()
    with torch.no_grad():
        awe, alpha, grads = K.attention_module(enc, h, prm["encoder_att.weight"], prm["encoder_att.bias"],
                                               prm["decoder_att.weight"], prm["decoder_att.bias"],
                                               prm["full_att.weight"], prm["full_att.bias"], dawe, dalpha)
    _close(awe, awe_o, "awe"); _close(alpha, alpha_o, "alpha")
    _close(grads["enc"], enc.grad, "d enc"); _close(grads["h"], h.grad, "d h")
    for k, v in prm.items():
        if k == "full_att.bias":      # exactly 0 in exact arithmetic (softmax shift invariance): absolute
            assert abs(float(grads[k]) - float(v.grad)) <= TOL
            continue
        _close(grads[k], v.grad, k)


def test_attention_references_with_slabs_bias_and_gate():
    """What the stand-alone module does not use: slab sums, dec_bias, the f_beta gate, mean_pixels, ragged datt1_post."""
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    rows, P, A, E, T = 3, 13, 10, 22, 4
    att1, slabs, bd, w, b0 = rnd(rows, P, A), rnd(3, rows, A), rnd(A), rnd(A), rnd(1)
    sc = K.attn_scores(att1, slabs, bd, w, b0)
    att2 = slabs[0] + slabs[1] + slabs[2] + bd
    _close(sc["att2"], att2, "att2")
    _close(sc["e"], torch.relu(att1 + att2[:, None]) @ w + b0, "e")
    assert (sc["e_abs"] >= sc["e"].abs() - 1e-12).all()
    enc, gp, bb = rnd(rows, P, E), rnd(2, rows, E), rnd(E)
    cx = K.attn_context(enc, sc["e"], gp, bb)
    _close(cx["alpha"], torch.softmax(sc["e"], 1), "alpha")
    _close(cx["z"], torch.sigmoid(gp.sum(0) + bb) * torch.einsum("bp,bpe->be", torch.softmax(sc["e"], 1), enc), "z")
    _close(K.mean_pixels(enc)["out"], enc.mean(1), "mean")
    # datt1_post over T steps with ragged lengths == autograd of sum_t sum_b<bt (relu(att1 + att2_t) . w + b0) . de_t
    dl = [4, 9, 1]
    a1 = att1.clone().requires_grad_(True)
    wv, bv = w.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    att2_all, de_all = rnd(T, rows, A), rnd(T, rows, P)
    loss = 0
    for t in range(T):
        for b in range(rows):
            if t < min(dl[b], T):
                loss = loss + ((torch.relu(a1[b] + att2_all[t, b]) @ wv + bv) * de_all[t, b]).sum()
    loss.backward()
    bad = att2_all.clone(); bad[1:, 2] = float("nan")          # steps that do not exist must not be read
    post = K.attn_datt1_post(dl, att1, bad, de_all, w)
    _close(post["datt1"], a1.grad, "datt1"); _close(post["dw"], wv.grad, "dw"); _close(post["db0"].view(1), bv.grad, "db0")


def test_scn_cell_references_reproduce_the_oracle_and_its_autograd():
    g = torch.Generator().manual_seed(13)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, I, S, F, H = 5, 22, 7, 9, 14
    prm = {"weight_ia": rnd(I, 4 * F) * 0.3, "weight_ib": rnd(S, 4 * F) * 0.3, "weight_ic": rnd(H, 4 * F) * 0.3,
           "weight_ha": rnd(H, 4 * F) * 0.3, "weight_hb": rnd(S, 4 * F) * 0.3, "weight_hc": rnd(H, 4 * F) * 0.3,
           "bias_ih": rnd(4 * H) * 0.1, "bias_hh": rnd(4 * H) * 0.1}
    prm = {k: v.requires_grad_(True) for k, v in prm.items()}
    u, s = rnd(B, I).requires_grad_(True), rnd(B, S).requires_grad_(True)
    h0, c0 = rnd(B, H).requires_grad_(True), rnd(B, H).requires_grad_(True)
    dh, dc = rnd(B, H), rnd(B, H)
    h_o, c_o = R.scn_cell_forward(prm, "", u, s, (h0, c0))
    ((h_o * dh).sum() + (c_o * dc).sum()).backward()
    with torch.no_grad():
        h, c, grads = K.scn_cell_module(u, s, h0, c0, prm["weight_ia"], prm["weight_ib"], prm["weight_ic"], prm["weight_ha"],
                                        prm["weight_hb"], prm["weight_hc"], prm["bias_ih"], prm["bias_hh"], dh, dc)
    _close(h, h_o, "h"); _close(c, c_o, "c")
    for k, ref in (("u", u), ("s", s), ("h0", h0), ("c0", c0)):
        _close(grads[k], ref.grad, "d " + k)
    for k, v in prm.items():
        _close(grads[k], v.grad, k)


def test_cell_references_with_slabs_rows_next_and_helpers():
    g = torch.Generator().manual_seed(14)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    rows, H, F = 5, 7, 3
    # lstm_bwd with rows_next < rows == autograd where rows >= rows_next get no gradient from the next step
    r = rnd(2, 4, rows, H).requires_grad_(True)
    cp = rnd(rows, H).requires_grad_(True)
    f = K.lstm_fwd(r, None, rnd(4 * H), cp)
    dh_fc, dhn, dcn = rnd(rows, H), rnd(3, rows, H), rnd(rows, H)
    live = (torch.arange(rows) < 3).double().unsqueeze(1)
    ((f["h"] * (dh_fc + live * dhn.sum(0))).sum() + (f["c"] * live * dcn).sum()).backward()
    dhn_bad, dcn_bad = dhn.clone(), dcn.clone()
    dhn_bad[:, 3:], dcn_bad[3:] = float("nan"), float("nan")
    b = K.lstm_bwd(3, dh_fc, dhn_bad, dcn_bad, f["gates"].detach(), cp.detach(), f["tanhc"].detach())
    _close(b["dr"].view(rows, 4, H).permute(1, 0, 2), r.grad[0], "dr"); _close(b["dc"], cp.grad, "dc")
    # gate_bwd == autograd of sigmoid(gpre) * awe
    gp, awe = rnd(rows, H).requires_grad_(True), rnd(rows, H).requires_grad_(True)
    dz = rnd(2, rows, H)
    (torch.sigmoid(gp) * awe * dz.sum(0)).sum().backward()
    gb = K.gate_bwd(dz, awe.detach(), torch.sigmoid(gp).detach())
    _close(gb["dawe"], awe.grad, "dawe"); _close(gb["dgpre"], gp.grad, "dgpre")
    # scn_mix_fwd with ex and slabs
    pz, ex, ph, qx, qh = rnd(2, rows, 4 * F), rnd(rows, 4 * F), rnd(3, rows, 4 * F), rnd(rows, 4 * F), rnd(rows, 4 * F)
    m = K.scn_mix_fwd(pz, ex, ph, qx, qh)
    _close(m["pa"], ex + pz.sum(0), "pa")
    _close(m["xcat"][:, 2, F:], (ph.sum(0) * qh)[:, 2 * F:3 * F], "xcat h side")
    x = rnd(6, 4)
    _close(K.colsum(x, rnd(4), 0.0)["out"], x.sum(0), "colsum")
    xs, q = rnd(2, 3, 4), rnd(3, 4)
    _close(K.mul_bcast(xs, q)["out"][1], xs[1] * q, "mul_bcast")
    _close(K.transpose2d(x)["out"], x.t(), "transpose2d")


# ---- the pooled path (scnattn_pool): references against the dense formulation, autograd and the refusals ------------------
POOLS = [(1, 1, 2, 2), (3, 5, 4, 7), (8, 8, 14, 14)]


def _taps(shape):
    from scnattn.functional import PoolTaps
    return PoolTaps(*shape, "cpu")


@pytest.mark.parametrize("shape", POOLS)
def test_pooled_context_reference_equals_the_dense_one_on_the_pooled_map(shape):
    """attn_context_pooled(x) == attn_context(M x), M = PoolTaps.matrix(), and M x == adaptive_avg_pool2d of the map"""
    g = torch.Generator().manual_seed(21)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pool = _taps(shape)
    hi, wi, ho, wo = shape
    rows, E = 3, 6
    x, e, gp, bb = rnd(rows, pool.Q, E), rnd(rows, pool.P), rnd(2, rows, E), rnd(E)
    M = pool.matrix().double()
    enc = torch.einsum("pq,bqe->bpe", M, x)
    ref = torch.nn.functional.adaptive_avg_pool2d(x.view(rows, hi, wi, E).permute(0, 3, 1, 2), (ho, wo))
    _close(enc, ref.permute(0, 2, 3, 1).reshape(rows, pool.P, E), "M x")
    a, b = K.attn_context_pooled(x, pool, e, gp, bb), K.attn_context(enc, e, gp, bb)
    for k in ("alpha", "awe", "gate", "z"):
        _close(a[k], b[k], k)
    _close(a["alphaq"], b["alpha"] @ M, "alphaq")
    _close(K.attn_context_pooled(x, pool, e)["z"], b["awe"], "z without gpre")
    _close(K.weighted_rows(x, M.sum(0) / pool.P)["out"], enc.mean(1), "weighted_rows with the column sums of M / P")


@pytest.mark.parametrize("shape", POOLS)
def test_pooled_softmax_bwd_reference_equals_autograd(shape):
    """with dalphaq = x . dawe: de = d/de and datt2 = d/d att2 of  awe(alpha) . dawe + alpha . dalpha_in  +  e . 1 taken
    through the mask, where awe = alpha . (M x)"""
    g = torch.Generator().manual_seed(22)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pool = _taps(shape)
    rows, E, A = 3, 6, 5
    M = pool.matrix().double()
    x, dawe, din = rnd(rows, pool.Q, E), rnd(rows, E), rnd(rows, pool.P)
    att1, w = rnd(rows, pool.P, A), rnd(A)
    att2 = rnd(rows, A).requires_grad_(True)
    e = (torch.relu(att1 + att2.unsqueeze(1)) * w).sum(-1)
    e.retain_grad()
    alpha = torch.softmax(e, 1)
    awe = torch.einsum("bp,pq,bqe->be", alpha, M, x)
    ((awe * dawe).sum() + (alpha * din).sum()).backward()
    dalphaq = K.attn_dalpha(x, dawe)["dalpha"]
    for given in (din, None):
        if given is None:
            att2.grad, e.grad = None, None
            e2 = (torch.relu(att1 + att2.unsqueeze(1)) * w).sum(-1)
            e2.retain_grad()
            (torch.einsum("bp,pq,bqe->be", torch.softmax(e2, 1), M, x) * dawe).sum().backward()
            e = e2
        r = K.attn_softmax_bwd_pooled(att1, att2.detach(), w, alpha.detach(), pool, dalphaq, given)
        _close(r["de"], e.grad, "de"); _close(r["datt2"], att2.grad, "datt2")
        assert (r["de_abs"] >= r["de"].abs() - 1e-12).all() and (r["datt2_abs"] >= r["datt2"].abs() - 1e-12).all()
        assert r["de_n"] == pool.P + 7 and r["datt2_n"] == 2 * pool.P + 8
    # the |terms| of the gather are carried: with cancelling taps |dalpha| is small and the carried sum is not
    plain = K.attn_softmax_bwd(att1, att2.detach(), w, alpha.detach(), r["dalpha"])
    assert (r["de_abs"] >= plain["de_abs"] - 1e-12).all()


@pytest.mark.parametrize("shape", POOLS)
def test_pool_transpose_reference_is_the_transpose_of_pool_expand(shape):
    g = torch.Generator().manual_seed(23)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pool = _taps(shape)
    B, A = 2, 8
    y, gr, bias = rnd(B, pool.Q, A), rnd(B, pool.P, A), rnd(A)
    ex, tr = K.pool_expand(y, pool), K.pool_transpose(gr, pool)
    M = pool.matrix().double()
    _close(ex["out"], torch.einsum("pq,bqa->bpa", M, y), "expand")
    _close(tr["out"], torch.einsum("pq,bpa->bqa", M, gr), "transpose")
    assert abs(float((ex["out"] * gr).sum() - (y * tr["out"]).sum())) <= TOL * float((ex["out_abs"] * gr.abs()).sum())
    _close(K.pool_expand(y, pool, bias)["out"], ex["out"] + bias, "expand + bias")
    assert tr["out_n"].shape == (pool.Q, 1) and int(tr["out_n"].sum()) == int((pool.tap_w > 0).sum())
    o0, wts, v = rnd(B, pool.Q, A), rnd(pool.Q), rnd(B, A)
    _close(K.add_bcast_rows_w(o0, wts, v)["out"], o0 + torch.einsum("q,ba->bqa", wts, v), "add_bcast_rows_w")


_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error(), h.scnattn_last_error()


def test_pooled_entries_refuse_before_launching():
    """host-side argument checks: nothing is launched, no GPU is needed"""
    import ctypes as C
    from scnattn import _lib as L
    h = L.lib()

    def pool(Q=64, qmax=4, **null):
        t = {k: (None if k in null else _P) for k in ("tap_idx", "tap_w", "qtap_idx", "qtap_w", "col_w")}
        return C.byref(L.Pool(Q, qmax, t["tap_idx"], t["tap_w"], t["qtap_idx"], t["qtap_w"], t["col_w"]))

    def ctx(p, E=8):
        return h.scnattn_attn_context_pooled(None, 2, 196, E, _P, 0, p, _P, None, 0, 0, 0, None, None, 0, None, None, _P,
                                             None, None)

    def sbw(p, A=8):
        return h.scnattn_attn_softmax_bwd_pooled(None, 2, 196, A, _P, 0, _P, _P, _P, p, _P, None, 0, None, _P, A)

    def exp(p=0, A=8, y=_P, out=_P, bias=None):
        return h.scnattn_pool_expand(None, 2, 196, A, pool() if p == 0 else p, y, bias, out)

    def tra(p=0, A=8, x=_P, out=_P):
        return h.scnattn_pool_transpose(None, 2, 196, A, pool() if p == 0 else p, x, out)

    def abw(E=8, v=_P, out=_P):
        return h.scnattn_add_bcast_rows_w(None, 2, 64, E, _P, v, out)

    for call in (ctx, sbw, exp, tra):
        for name in ("tap_idx", "tap_w", "qtap_idx", "qtap_w", "col_w"):
            _refused(h, call(pool(**{name: 1})), b"null table")
        _refused(h, call(pool(qmax=65)), b"bad Q / qtap_max")
        _refused(h, call(pool(qmax=0)), b"bad Q / qtap_max")
        _refused(h, call(pool(Q=0)), b"bad Q / qtap_max")
        _refused(h, call(None), b"null descriptor")
    _refused(h, sbw(pool(Q=1025)), b"too large for the LDS staging")
    _refused(h, exp(A=6), b"multiple of 4")
    _refused(h, exp(y=_P + 4), b"pool_expand: bad argument")
    _refused(h, exp(out=_P + 4), b"pool_expand: bad argument")
    _refused(h, exp(bias=_P + 4), b"pool_expand: bad argument")
    _refused(h, tra(A=6), b"multiple of 4")
    _refused(h, tra(x=_P + 4), b"pool_transpose: bad argument")
    _refused(h, tra(out=_P + 4), b"pool_transpose: bad argument")
    _refused(h, abw(E=6), b"multiple of 4")
    _refused(h, abw(v=_P + 4), b"add_bcast_rows_w: bad argument")
    _refused(h, abw(out=_P + 4), b"add_bcast_rows_w: bad argument")
    # the drivers' own conditions are not the kernels': a pooled context with E % 4 != 0 is not refused for its width
    d = L.Dims(4, 196, 42, 24, 28, 36, 20, 14, 50, 5, 6, 1)
    sv, sc = C.c_size_t(), C.c_size_t()
    _refused(h, h.scnattn_seq_workspace(C.byref(d), pool(), C.byref(sv), C.byref(sc)), b"must be multiples of 4")
    d.E = 40
    _refused(h, h.scnattn_seq_workspace(C.byref(d), pool(Q=197), C.byref(sv), C.byref(sc)), b"bad Q / qtap_max")
    _refused(h, h.scnattn_seq_workspace(C.byref(d), pool(col_w=1), C.byref(sv), C.byref(sc)), b"null table")
    assert h.scnattn_seq_workspace(C.byref(d), pool(), C.byref(sv), C.byref(sc)) == 0


def test_new_symbols_are_bound_and_declared_and_the_version_stays():
    import os
    from scnattn import _lib as L
    h = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scnattn.h")).read()
    for name in ("scnattn_attn_scores_bf16", "scnattn_attn_context_bf16", "scnattn_attn_dalpha_bf16",
                 "scnattn_attn_softmax_bwd_bf16", "scnattn_attn_datt1_post_bf16", "scnattn_attn_context_pooled",
                 "scnattn_attn_softmax_bwd_pooled", "scnattn_weighted_rows", "scnattn_pool_expand", "scnattn_pool_transpose",
                 "scnattn_add_bcast_rows_w"):
        assert name in L._SIGS and name in L.EXPORTS and hasattr(h, name)
        assert "int %s(void* stream" % name in header
    assert h.scnattn_version() == 109       # new symbols only
