"""The fp64 references of the decode-step primitives (tests/decoder_kernel_refs.py) against the oracle.

The GPU tests of tests/test_gpu_decoder_kernels.py compare every kernel with these references; here the references,
composed in the order scnattn/functional.py composes the C calls, must reproduce oracle/scnattn_ref.py (pinned by the
golden vectors) and its autograd gradients in fp64, at a size where nothing is a multiple of 4.  Runs without a GPU."""
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
