"""Plain-torch references of the decode step's primitives (the `scnattn_*` entry points of include/scnattn.h:196-233).

Written from the header comments and the reference's math (models/attention.py:35-44, the gate of
models/decoders/attention_scn.py:147-148, models/scn_cell.py:62-154), not from the kernels.  Every function takes the
LOGICAL operands of the C call -- split-K slabs as a leading dimension `[nslab, ...]` that is summed, optional operands
as None -- and computes in the dtype of its inputs: called with fp64 tensors it is the reference, called with fp32
tensors it is "the same formula evaluated by torch on the CPU in fp32" that the transcendental results are measured
against.  For every result `x` that is a sum the dict also carries `x_abs`, the sum of the absolute values of the same
terms (what the forward error bound of a summation is relative to), and `x_n`, the number of terms / roundings.

tests/test_decoder_kernel_refs.py pins these against oracle/scnattn_ref.py (itself pinned by the golden vectors), and the
references of the pooled path (scnattn_pool; tests/test_gpu_attn_variant_kernels.py) against the dense ones and autograd.
"""
import torch


def _slab_sum(slabs):
    """slabs [n, ...] -> (sum over n, sum of |.| over n)"""
    return slabs.sum(0), slabs.abs().sum(0)


# ---- models/attention.py:37-39 ---------------------------------------------------------------------------------
def attn_scores(att1, att2_slabs, dec_bias, w, b0):
    """att1 [rows,P,A]; att2_slabs [n,rows,A]; dec_bias [A] or None; w [A]; b0 [1] or None.
    e[b,p] = sum_a relu(att1[b,p,a] + att2[b,a]) * w[a] + b0,  att2 = sum of the slabs + dec_bias (also returned)."""
    att2, att2_abs = _slab_sum(att2_slabs)
    n2 = att2_slabs.shape[0]
    if dec_bias is not None:
        att2, att2_abs, n2 = att2 + dec_bias, att2_abs + dec_bias.abs(), n2 + 1
    pre = att1 + att2.unsqueeze(1)
    e = (torch.relu(pre) * w).sum(-1)
    e_abs = (((pre > 0) * (att1.abs() + att2_abs.unsqueeze(1))) * w.abs()).sum(-1)
    if b0 is not None:
        e, e_abs = e + b0, e_abs + b0.abs()
    return {"e": e, "e_abs": e_abs, "e_n": att1.shape[-1] + n2 + 2, "att2": att2, "att2_abs": att2_abs, "att2_n": n2,
            "pre": pre}


# ---- models/attention.py:40-42 + attention_scn.py:147-148 ------------------------------------------------------
def softmax_rows(e):
    m = e.max(dim=1, keepdim=True)[0]
    ex = torch.exp(e - m)
    return ex / ex.sum(dim=1, keepdim=True)


def attn_context(enc, e, gpre_slabs=None, gate_bias=None):
    """enc [rows,P,E]; e [rows,P]; gpre_slabs [n,rows,E] or None; gate_bias [E] or None.
    alpha = softmax(e); awe = sum_p alpha*enc; gate = sigmoid(sum of slabs + bias); z = gate*awe (awe without gpre)."""
    alpha = softmax_rows(e)
    awe = (enc * alpha.unsqueeze(2)).sum(1)
    out = {"alpha": alpha, "awe": awe, "gate": None, "z": awe}
    if gpre_slabs is not None:
        gp = gpre_slabs.sum(0)
        if gate_bias is not None:
            gp = gp + gate_bias
        out["gate"] = torch.sigmoid(gp)
        out["z"] = out["gate"] * awe
    return out


def mean_pixels(enc):
    return {"out": enc.mean(1), "out_abs": enc.abs().mean(1), "out_n": enc.shape[1] + 1}


# ---- backward of the context / softmax / scores ----------------------------------------------------------------
def attn_dalpha(enc, dawe, dalpha_in=None):
    """dalpha[b,p] = sum_c enc[b,p,c] * dawe[b,c] (+ dalpha_in[b,p])"""
    t = enc * dawe.unsqueeze(1)
    d, d_abs = t.sum(-1), t.abs().sum(-1)
    if dalpha_in is not None:
        d, d_abs = d + dalpha_in, d_abs + dalpha_in.abs()
    return {"dalpha": d, "dalpha_abs": d_abs, "dalpha_n": enc.shape[-1] + 1}


def attn_softmax_bwd(att1, att2, w, alpha, dalpha, dalpha_abs=None, dalpha_n=0):
    """de = alpha * (dalpha - sum_p alpha*dalpha)   (softmax backward)
    datt2[b,a] = w[a] * sum_p de[b,p] * [att1[b,p,a] + att2[b,a] > 0]   (through full_att and the ReLU)
    dalpha_abs / dalpha_n: when dalpha is itself a sum the kernel forms (the pooled form below), the sum of its |terms| and
    the roundings it costs; they are carried into de and datt2."""
    P = alpha.shape[1]
    if dalpha_abs is None:
        dalpha_abs = dalpha.abs()
    dot = (alpha * dalpha).sum(1, keepdim=True)
    dot_abs = (alpha.abs() * dalpha_abs).sum(1, keepdim=True)
    de = alpha * (dalpha - dot)
    de_abs = alpha.abs() * (dalpha_abs + dot_abs)            # |terms| of de written out as one sum of P + 1 products
    pre = att1 + att2.unsqueeze(1)
    mask = (pre > 0).to(att1.dtype)
    datt2 = w * (mask * de.unsqueeze(2)).sum(1)
    datt2_abs = w.abs() * (mask * de_abs.unsqueeze(2)).sum(1)
    return {"de": de, "de_abs": de_abs, "de_n": P + 2 + dalpha_n, "datt2": datt2, "datt2_abs": datt2_abs,
            "datt2_n": 2 * P + 3 + dalpha_n, "pre": pre}


# ---- the pooled path: encoder_out = M x, M = the fixed pooling matrix a scnattn_pool encodes (include/scnattn.h) ----
# `pool` is anything with the tables of scnattn.functional.PoolTaps: tap_idx / tap_w [P,4] (row p of M; unused taps weight 0),
# qtap_idx / qtap_w [Q,qmax] (column q of M; unused taps index -1).
def _qtaps(pool, like):
    idx = pool.qtap_idx.long().cpu()
    live = idx >= 0
    return idx.clamp_min(0), pool.qtap_w.cpu().to(like.dtype) * live.to(like.dtype), live


def attn_context_pooled(x, pool, e, gpre_slabs=None, gate_bias=None):
    """x [rows,Q,E]; e [rows,P].  alpha = softmax(e) over P; alphaq[q] = sum_k qtap_w[q][k] * alpha[qtap_idx[q][k]];
    awe = sum_q alphaq[q] * x[q]; gate / z as attn_context."""
    alpha = softmax_rows(e)
    idx, qw, _ = _qtaps(pool, x)
    alphaq = (alpha[:, idx] * qw).sum(-1)
    awe = (x * alphaq.unsqueeze(2)).sum(1)
    out = {"alpha": alpha, "alphaq": alphaq, "awe": awe, "gate": None, "z": awe}
    if gpre_slabs is not None:
        gp = gpre_slabs.sum(0)
        if gate_bias is not None:
            gp = gp + gate_bias
        out["gate"] = torch.sigmoid(gp)
        out["z"] = out["gate"] * awe
    return out


def attn_softmax_bwd_pooled(att1, att2, w, alpha, pool, dalphaq, dalpha_in=None):
    """dalpha[p] = dalpha_in[p] + sum_k tap_w[p][k] * dalphaq[tap_idx[p][k]] (dalphaq [rows,Q]), then attn_softmax_bwd: the
    |terms| of that gather go into de_abs / datt2_abs, and its 4 products + the sum with dalpha_in are 5 more roundings."""
    t = dalphaq[:, pool.tap_idx.long().cpu()] * pool.tap_w.cpu().to(dalphaq.dtype)          # [rows,P,4]
    d, d_abs = t.sum(-1), t.abs().sum(-1)
    if dalpha_in is not None:
        d, d_abs = d + dalpha_in, d_abs + dalpha_in.abs()
    out = attn_softmax_bwd(att1, att2, w, alpha, d, d_abs, 5)
    out["dalpha"] = d
    return out


def pool_expand(y, pool, bias=None):
    """y [B,Q,A] -> out[b,p,:] = sum_k tap_w[p][k] * y[b,tap_idx[p][k],:] + bias   (M y + bias)"""
    t = y[:, pool.tap_idx.long().cpu()] * pool.tap_w.cpu().to(y.dtype).unsqueeze(-1)        # [B,P,4,A]
    o, o_abs, n = t.sum(2), t.abs().sum(2), 4
    if bias is not None:
        o, o_abs, n = o + bias, o_abs + bias.abs(), n + 1
    return {"out": o, "out_abs": o_abs, "out_n": n}


def pool_transpose(g, pool):
    """g [B,P,A] -> out[b,q,:] = sum over the live taps of qtap_w[q][k] * g[b,qtap_idx[q][k],:]   (M^T g).
    out_n is per source pixel: [Q,1], its live taps."""
    idx, qw, live = _qtaps(pool, g)
    t = g[:, idx] * qw.unsqueeze(-1)                                                        # [B,Q,qmax,A]
    return {"out": t.sum(2), "out_abs": t.abs().sum(2), "out_n": live.sum(1, keepdim=True)}


def add_bcast_rows_w(out0, wts, v):
    """out[b,q,:] = out0[b,q,:] + wts[q] * v[b,:]"""
    t = wts.view(1, -1, 1) * v.unsqueeze(1)
    return {"out": out0 + t, "out_abs": out0.abs() + t.abs(), "out_n": 2}


def weighted_rows(x, wts):
    """out[b,:] = sum_q wts[q] * x[b,q,:]"""
    t = x * wts.view(1, -1, 1)
    return {"out": t.sum(1), "out_abs": t.abs().sum(1), "out_n": x.shape[1]}


def attn_datt1_post(dl, att1, att2_all, de_all, w):
    """dl [B] ints; att1 [B,P,A]; att2_all [T,B,A]; de_all [T,B,P]; w [A].  Steps t >= min(dl[b], T) of row b do not
    exist (their att2 / de may hold anything).
    datt1[b,p,a] = w[a] * sum_t de[t,b,p] * [att1[b,p,a] + att2[t,b,a] > 0]
    dw[a] = sum_{t,b,p} de[t,b,p] * relu(att1[b,p,a] + att2[t,b,a]);  db0 = sum_{t,b,p} de[t,b,p]
    (the kernel leaves dw / db0 as per-workgroup partial rows [A+1]: their sum over the workgroups is compared)."""
    T, B, P = de_all.shape
    A = att1.shape[-1]
    acc = torch.zeros_like(att1)
    acc_abs = torch.zeros_like(att1)
    dw, dw_abs = att1.new_zeros(A), att1.new_zeros(A)
    db, db_abs = att1.new_zeros(()), att1.new_zeros(())
    pre_min = float("inf")
    nterms = 0
    for b in range(B):
        for t in range(min(int(dl[b]), T)):
            pre = att1[b] + att2_all[t, b].unsqueeze(0)          # [P,A]
            pre_min = min(pre_min, float(pre.abs().min()))
            d = de_all[t, b].unsqueeze(1)                        # [P,1]
            m = (pre > 0).to(att1.dtype)
            acc[b] += m * d
            acc_abs[b] += m * d.abs()
            dw += (d * torch.relu(pre)).sum(0)
            dw_abs += (d.abs() * m * (att1[b].abs() + att2_all[t, b].abs().unsqueeze(0))).sum(0)
            db += d.sum()
            db_abs += d.abs().sum()
            nterms += P
    return {"datt1": w * acc, "datt1_abs": w.abs() * acc_abs, "datt1_n": T + 1, "dw": dw, "dw_abs": dw_abs,
            "dw_n": nterms + 2, "db0": db, "db0_abs": db_abs, "db0_n": nterms, "pre_min": pre_min}


# ---- models/scn_cell.py:73-91 / 134-144, element-wise parts ----------------------------------------------------
def scn_mix_fwd(pz_slabs, ex, ph_slabs, qx, qh):
    """pz_slabs [n,rows,4F] or None; ex [rows,4F] or None; ph_slabs [m,rows,4F]; qx, qh [rows,4F] (the tag factors).
    pa = ex + sum pz;  phs = sum ph;  xcat[b,g] = [ pa_g * qx_g | phs_g * qh_g ]   (gate blocks g = i,f,o,c of width F)"""
    rows, F4 = qx.shape
    F = F4 // 4
    pa, pa_abs, n = torch.zeros_like(qx), torch.zeros_like(qx), 0
    if ex is not None:
        pa, pa_abs, n = pa + ex, pa_abs + ex.abs(), n + 1
    if pz_slabs is not None:
        s, a = _slab_sum(pz_slabs)
        pa, pa_abs, n = pa + s, pa_abs + a, n + pz_slabs.shape[0]
    phs, phs_abs = _slab_sum(ph_slabs)
    xcat = torch.cat([(pa * qx).view(rows, 4, F), (phs * qh).view(rows, 4, F)], dim=2)
    xcat_abs = torch.cat([(pa_abs * qx.abs()).view(rows, 4, F), (phs_abs * qh.abs()).view(rows, 4, F)], dim=2)
    return {"pa": pa, "pa_abs": pa_abs, "pa_n": max(n, 1), "phs": phs, "phs_abs": phs_abs, "phs_n": ph_slabs.shape[0],
            "xcat": xcat, "xcat_abs": xcat_abs, "xcat_n": max(n, ph_slabs.shape[0]) + 1}


def scn_mix_bwd(dxcat_slabs, qx, qh, pa, phs, dqx_acc, dqh_acc):
    """dxcat_slabs [n,4,rows,2F] (gradient of xcat, gate-major as the product that makes it leaves it).
    dpx = dmx*qx, dph = dmh*qh (gradients of pa / phs);  dq*_acc += dmx*pa / dmh*phs (gradients of the tag factors)."""
    n, _, rows, F2 = dxcat_slabs.shape
    F = F2 // 2
    s, a = _slab_sum(dxcat_slabs)                                   # [4,rows,2F]
    dmx, dmx_abs = (x[:, :, :F].permute(1, 0, 2).reshape(rows, 4 * F) for x in (s, a))
    dmh, dmh_abs = (x[:, :, F:].permute(1, 0, 2).reshape(rows, 4 * F) for x in (s, a))
    return {"dpx": dmx * qx, "dpx_abs": dmx_abs * qx.abs(), "dpx_n": n + 1,
            "dph": dmh * qh, "dph_abs": dmh_abs * qh.abs(), "dph_n": n + 1,
            "dqx_acc": dqx_acc + dmx * pa, "dqx_acc_abs": dqx_acc.abs() + dmx_abs * pa.abs(), "dqx_acc_n": n + 2,
            "dqh_acc": dqh_acc + dmh * phs, "dqh_acc_abs": dqh_acc.abs() + dmh_abs * phs.abs(), "dqh_acc_n": n + 2}


# ---- models/scn_cell.py:146-152 --------------------------------------------------------------------------------
def lstm_fwd(r_slabs, bih, bhh, c_prev):
    """r_slabs [n,4,rows,H] pre-activations (gate order i,f,o,c~); bih, bhh [4H] or None; c_prev [rows,H].
    gates [rows,4H] = (sigmoid i, sigmoid f, sigmoid o, tanh c~); c = f*c_prev + i*c~; tanhc = tanh(c); h = o*tanhc"""
    _, _, rows, H = r_slabs.shape
    pre = r_slabs.sum(0)
    for bias in (bih, bhh):
        if bias is not None:
            pre = pre + bias.view(4, 1, H)
    i, f, o, g = torch.sigmoid(pre[0]), torch.sigmoid(pre[1]), torch.sigmoid(pre[2]), torch.tanh(pre[3])
    c = f * c_prev + i * g
    tc = torch.tanh(c)
    return {"gates": torch.cat([i, f, o, g], dim=1), "c": c, "h": o * tc, "tanhc": tc}


def lstm_bwd(rows_next, dh_fc, dh_next_slabs, dc, gates, c_prev, tanhc):
    """Backward of lstm_fwd for `rows` rows of which only the first `rows_next` were still decoding at the next step:
    dh = dh_fc (+ sum of dh_next slabs for b < rows_next); the incoming dc counts for b < rows_next only.
    dr [rows,4H] = gradient of the pre-activations; dc_out = gradient of c_prev."""
    rows, H = c_prev.shape
    live = (torch.arange(rows) < rows_next).to(c_prev.dtype).unsqueeze(1)
    dh = torch.zeros_like(c_prev) if dh_fc is None else dh_fc.clone()
    if dh_next_slabs is not None:
        dh = dh + torch.where(live > 0, dh_next_slabs.sum(0), torch.zeros_like(dh))
    dcn = torch.where(live > 0, dc, torch.zeros_like(dc))
    i, f, o, g = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
    dcc = dcn + dh * o * (1 - tanhc * tanhc)
    dr = torch.cat([dcc * g * i * (1 - i), dcc * c_prev * f * (1 - f), dh * tanhc * o * (1 - o), dcc * i * (1 - g * g)],
                   dim=1)
    return {"dr": dr, "dc": dcc * f}


# ---- attention_scn.py:147-148 backward, helpers ----------------------------------------------------------------
def gate_bwd(dz_slabs, awe, gate):
    """z = gate*awe, gate = sigmoid(gpre):  dawe = dz*gate;  dgpre = dz*awe*gate*(1-gate)"""
    d, d_abs = _slab_sum(dz_slabs)
    n = dz_slabs.shape[0]
    k = awe * gate * (1 - gate)
    return {"dawe": d * gate, "dawe_abs": d_abs * gate.abs(), "dawe_n": n + 1,
            "dgpre": d * k, "dgpre_abs": d_abs * k.abs(), "dgpre_n": n + 4}


def transpose2d(x):
    return {"out": x.t()}


def colsum(x, out0, beta):
    """out[n] = beta*out0[n] + sum_r x[r,n]"""
    o, o_abs = x.sum(0), x.abs().sum(0)
    if beta != 0:
        o, o_abs = o + beta * out0, o_abs + (beta * out0).abs()
    return {"out": o, "out_abs": o_abs, "out_n": x.shape[0] + 2}


def mul_bcast(x, q):
    """x [T,B,N] * q [B,N]"""
    return {"out": x * q.unsqueeze(0), "out_abs": (x * q.unsqueeze(0)).abs(), "out_n": 1}


# ---- the composition of scnattn/functional.py::_Attention (forward + backward) -------------------------------
def attention_module(enc, h, We, be, Wd, bd, wf, b0, dawe, dalpha_in):
    """The primitives in the order the stand-alone attention module calls them, dense products in between.
    Returns (awe, alpha, gradients dict keyed like the oracle's parameters + 'enc', 'h')."""
    B, P, E = enc.shape
    att1 = (enc.reshape(B * P, E) @ We.t() + be).view(B, P, -1)
    att2 = h @ Wd.t() + bd
    sc = attn_scores(att1, att2.unsqueeze(0), None, wf.view(-1), b0)
    ctx = attn_context(enc, sc["e"])
    da = attn_dalpha(enc, dawe, dalpha_in)
    sb = attn_softmax_bwd(att1, att2, wf.view(-1), ctx["alpha"], da["dalpha"])
    post = attn_datt1_post([1] * B, att1, att2.unsqueeze(0), sb["de"].unsqueeze(0), wf.view(-1))
    datt1 = post["datt1"].reshape(B * P, -1)
    g = {"enc": (datt1 @ We).view(B, P, E) + ctx["alpha"].unsqueeze(2) * dawe.unsqueeze(1),
         "h": sb["datt2"] @ Wd,
         "encoder_att.weight": datt1.t() @ enc.reshape(B * P, E), "encoder_att.bias": datt1.sum(0),
         "decoder_att.weight": sb["datt2"].t() @ h, "decoder_att.bias": sb["datt2"].sum(0),
         "full_att.weight": post["dw"].view(1, -1), "full_att.bias": post["db0"].view(1)}
    return ctx["awe"], ctx["alpha"], g


def scn_cell_module(u, s, h0, c0, Wa, Wb, Wc, Ha, Hb, Hc, bih, bhh, dh, dc):
    """One SCN-LSTM step from the element-wise primitives (scn_mix_fwd -> lstm_fwd; lstm_bwd -> scn_mix_bwd) with the
    dense contractions in between, the way the sequence driver chains them: x and h sides share one xcat.
    Returns (h, c, gradients dict)."""
    rows, H = h0.shape
    F4 = Wa.shape[1]
    F = F4 // 4
    qx, qh = s @ Wb, s @ Hb
    mix = scn_mix_fwd((u @ Wa).unsqueeze(0), None, (h0 @ Ha).unsqueeze(0), qx, qh)
    xcat = mix["xcat"]                                               # [rows,4,2F]
    WD = torch.stack([torch.cat([Wc[:, g * F:(g + 1) * F], Hc[:, g * F:(g + 1) * F]], dim=1) for g in range(4)])  # [4,H,2F]
    r = torch.einsum("bgk,ghk->gbh", xcat, WD)                       # [4,rows,H]
    cell = lstm_fwd(r.unsqueeze(0), bih, bhh, c0)
    back = lstm_bwd(rows, dh, None, dc, cell["gates"], c0, cell["tanhc"])
    dr = back["dr"].view(rows, 4, H)
    dxcat = torch.einsum("bgh,ghk->gbk", dr, WD)                     # [4,rows,2F]
    zero = torch.zeros_like(qx)
    mb = scn_mix_bwd(dxcat.unsqueeze(0), qx, qh, mix["pa"], mix["phs"], zero, zero)
    dWD = torch.einsum("bgh,bgk->ghk", dr, xcat)
    g = {"u": mb["dpx"] @ Wa.t(), "h0": mb["dph"] @ Ha.t(), "c0": back["dc"],
         "s": mb["dqx_acc"] @ Wb.t() + mb["dqh_acc"] @ Hb.t(),
         "weight_ia": u.t() @ mb["dpx"], "weight_ha": h0.t() @ mb["dph"],
         "weight_ib": s.t() @ mb["dqx_acc"], "weight_hb": s.t() @ mb["dqh_acc"],
         "weight_ic": torch.cat([dWD[g_, :, :F] for g_ in range(4)], dim=1),
         "weight_hc": torch.cat([dWD[g_, :, F:] for g_ in range(4)], dim=1),
         "bias_ih": dr.sum(0).reshape(-1), "bias_hh": dr.sum(0).reshape(-1)}
    return cell["h"], cell["c"], g
