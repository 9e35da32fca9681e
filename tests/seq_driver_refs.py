"""The driver tier: what tests/test_seq_driver_refs.py (CPU) and tests/test_gpu_seq_driver.py (GPU) share.

  make_case   one problem of scnattn_seq_fwd / scnattn_seq_bwd from a seed -- weights from a CPU AttentionSCN / PureSCN
              state_dict, the driver's own inputs (sorted captions, decode lengths, bt_host, a pre-scaled dropout mask,
              dpreds / dalphas as the upstream gradients, garbage in every dead cell and padding token) -- with the results
              of oracle/scnattn_ref.py in fp64 and in fp32: preds, alphas, every parameter gradient, d encoder_out (d x
              through AdaptiveAvgPool2d on the pooled path) and d tags.
  run_driver  the C-ABI call pair on buffers the caller fills and sizes (scnattn_seq_workspace gives the extents).
  row_ok      the judge: every row of a result against the fp64 row's own maximum, the yardstick being the worst
              row-relative error of the same formula in plain CPU fp32 (never anything the library computed).
  saved_layout  the carve of `saved` (csrc/sequence.cpp carve_saved), restated so that a test can compare the saved state
              of single batch rows; run_driver asserts that it ends where scnattn_seq_workspace says.
A plain module (tests/ is on sys.path)."""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

from kernel_harness import GBuf, _note

TOL_OUT = 1e-4
TOL_GRAD = 2e-4
LIVE = 1e-6               # a row is live when its fp64 maximum is at least this fraction of the tensor's
FACTOR = 4.0              # the kernel tier's margin over the CPU-fp32 yardstick (_yard_ok)
ZERO_BIAS = "g.attention.full_att.bias"       # exactly 0 in exact arithmetic (softmax shift invariance): absolute
ZERO_BIAS_TOL = 1e-4

M4 = (24, 20, 28, 36, 12, 40)         # A, M, D, F, S, E: pooled and bf16 are possible
ODD = (26, 21, 30, 37, 13, 42)        # scalar instances, fp32 only

# id, has_att, dims, V, pooled, B, lengths, L - T, dropout mask, option ksplit, decoder_bf16 modes beyond 0, seed
# (axes paired round-robin, no cross product; `ragged` reaches one row at the last step: [8,8,6,4,2,1] at B = 6).
# The seed is 0 unless the draw fails the judge's precondition, which looks at the CPU references alone: seed 0 of
# att-m4-pool-B33-ties draws a row of d decoder_att.weight at 2.5e-4 of the tensor's maximum that is cancellation noise
# (rho = 1.9e-4 in CPU fp32).
CASES = [
    ("att-m4-B6-ragged",        1, M4,  50, 0, 6,  "ragged", 1, 0, 0, (1, 2), 0),
    ("att-odd-B33-ragged-k3",   1, ODD, 51, 0, 33, "ragged", 3, 1, 3, (), 0),
    ("att-m4-pool-B6-ragged-k3", 1, M4, 51, 1, 6,  "ragged", 1, 1, 3, (1, 2), 0),
    ("att-m4-pool-B33-ties",    1, M4,  50, 1, 33, "ties",   0, 0, 0, (), 1),
    ("scn-m4-B6-ragged-k3",     0, M4,  50, 0, 6,  "ragged", 1, 1, 3, (1, 2), 0),
    ("scn-odd-B33-ties",        0, ODD, 51, 0, 33, "ties",   3, 0, 0, (), 0),
    ("att-odd-B1",              1, ODD, 51, 0, 1,  "ragged", 1, 0, 0, (), 0),
    ("att-m4-B6-full-k3",       1, M4,  50, 0, 6,  "full",   1, 1, 3, (2,), 0),
    ("att-odd-B6-T1-k3",        1, ODD, 50, 0, 6,  "T1",     1, 0, 3, (), 0),
    ("scn-m4-pool-B6-full",     0, M4,  51, 1, 6,  "full",   0, 0, 0, (), 0),
    ("scn-odd-B1-T1-k3",        0, ODD, 50, 0, 1,  "T1",     2, 1, 3, (), 0),
    ("att-m4-pool-B1-k3",       1, M4,  51, 1, 1,  "ragged", 3, 0, 3, (), 0),
    ("att-m4-B33-full",         1, M4,  51, 0, 33, "full",   1, 0, 0, (1,), 0),
]
CASE_IDS = [c[0] for c in CASES]
HIN, HOUT = 3, 4          # the pooled cases: a 3x3 map (Q = 9) up-sampled to 4x4 (P = 16); dense: P = 9


def decode_lengths(kind, B):
    if kind == "ragged":            # one row left at the last step
        if B == 6:
            return [8, 8, 6, 4, 2, 1]
        return [8] + [7 - ((b - 1) * 7) // max(B - 1, 1) for b in range(1, B)]
    if kind == "ties":
        return sorted(([5, 3, 2] * B)[:B], reverse=True)
    return [5 if kind == "full" else 1] * B


class Case:
    """inputs (CPU, fp32), dims in scnattn_dims order, ref64 / ref32: result name -> tensor ("preds", "alphas", "denc" -- d x
    on the pooled path --, "dtags", "g." + state_dict key)"""

    def variant(self, **kw):
        """the same problem with some inputs replaced; the references do not carry over"""
        v = Case()
        v.__dict__.update(self.__dict__)
        v.__dict__.update(kw)
        v.ref64 = v.ref32 = None
        return v

    @property
    def live(self):
        """(B, T) bool: cell (b, t) is decoded"""
        return torch.arange(self.T).unsqueeze(0) < torch.tensor(self.dl).unsqueeze(1)


def _field_keys(sd):
    from models.decoders.attention_scn import _KEY_OF_FIELD
    from scnattn._lib import PARAM_FIELDS
    return [(f, _KEY_OF_FIELD[f] if _KEY_OF_FIELD[f] in sd else None) for f in PARAM_FIELDS]


def oracle(case, dtype):
    """the oracle's results for the driver's own inputs: loss = <preds, dpreds> + <alphas, dalphas>"""
    from oracle import scnattn_ref as R
    P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in case.sd.items()}
    src = case.enc.detach().clone().to(dtype).requires_grad_(True)        # a copy: .to() of the same dtype is the tensor itself
    tags = case.tags.detach().clone().to(dtype).requires_grad_(True)
    if case.pooled:     # (B, Q, E) -> AdaptiveAvgPool2d -> (B, P, E)
        x4 = src.view(case.B, HIN, HIN, case.E).permute(0, 3, 1, 2)
        enc = F.adaptive_avg_pool2d(x4, HOUT).permute(0, 2, 3, 1).reshape(case.B, HOUT * HOUT, case.E)
    else:
        enc = src
    caplens = (torch.tensor(case.dl) + 1).unsqueeze(1)
    si = torch.arange(case.B)
    mask = None if case.mask is None else case.mask.to(dtype)
    if case.has_att:
        preds, _, dl, alphas, _ = R.attention_scn_forward(P, enc, tags, case.caps, caplens, drop_mask=mask, sort_ind=si)
    else:
        (preds, _, dl, _), alphas = R.pure_scn_forward(P, enc, tags, case.caps, caplens, drop_mask=mask, sort_ind=si), None
    assert list(dl) == list(case.dl) and preds.shape[1] == case.T
    loss = (preds * case.dpreds.to(dtype)).sum()
    if alphas is not None and case.dalphas is not None:
        loss = loss + (alphas * case.dalphas.to(dtype)).sum()
    keys = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in keys] + [src, tags], allow_unused=True)
    out = {"preds": preds.detach()}
    if alphas is not None:
        out["alphas"] = alphas.detach()
    for k, g in zip(keys + ["denc", "dtags"], grads):
        ref = P[k] if k in P else (src if k == "denc" else tags)
        out[k if k in ("denc", "dtags") else "g." + k] = torch.zeros_like(ref) if g is None else g
    return out


def make_case(cid, has_att, dims6, V, pooled, B, lengths, extra_L, with_mask, ksplit=0, bf16=(), seed=0, refs=True):
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_scn import PureSCN
    A, M, D, Fd, S, E = dims6
    torch.manual_seed(1000 + seed)
    m = AttentionSCN(A, M, D, Fd, S, V, encoder_dim=E, dropout=0.0) if has_att else \
        PureSCN(M, D, Fd, S, V, encoder_dim=E, dropout=0.0)
    g = torch.Generator().manual_seed(2000 + seed)
    c = Case()
    c.id, c.has_att, c.pooled, c.ksplit, c.bf16 = cid, has_att, bool(pooled), ksplit, tuple(bf16)
    c.sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    c.fields = _field_keys(c.sd)
    c.dl = decode_lengths(lengths, B)
    c.B, c.E, c.V, c.T = B, E, V, max(c.dl)
    c.L = c.T + extra_L
    c.P, c.Q = (HOUT * HOUT, HIN * HIN) if pooled else (HIN * HIN, 0)
    c.dims = (B, c.P, E, A if has_att else 0, D, Fd, M, S, V, c.T, c.L, has_att)
    c.bt_host = [sum(l > t for l in c.dl) for t in range(c.T)]
    c.enc = torch.rand(B, c.Q if pooled else c.P, E, generator=g)      # the un-pooled map x on the pooled path
    c.tags = torch.rand(B, S, generator=g)
    c.caps = torch.randint(1, V - 3, (B, c.L), generator=g)            # padding cells hold tokens too: nothing reads them
    c.mask = (torch.rand(B, c.T, D, generator=g) < 0.5).float() * 2.0 if with_mask else None
    c.dpreds = torch.randn(B, c.T, V, generator=g)                     # dead cells included: they must not matter
    c.dalphas = torch.randn(B, c.T, c.P, generator=g) if has_att else None
    c.ref64 = c.ref32 = None
    if refs:
        c.ref64, c.ref32 = oracle(c, torch.float64), oracle(c, torch.float32)
    return c


@functools.lru_cache(maxsize=None)
def case(cid):
    return make_case(*CASES[CASE_IDS.index(cid)])


def other_problem(cid, seed=99):
    """another problem of the same dims, lengths and options (no references)"""
    return make_case(*CASES[CASE_IDS.index(cid)][:-1], seed=seed, refs=False)


def tokens_present(c):
    """(V,) bool: the token is the input of some decoded cell"""
    present = torch.zeros(c.V, dtype=torch.bool)
    present[c.caps[:, :c.T][c.live]] = True
    return present


# ---- the row judge ----------------------------------------------------------------------------------------------------------
def _rows(x):
    x = x.double()
    return x.reshape(1, -1) if x.dim() <= 1 else x.reshape(-1, x.shape[-1])


def row_yardstick(name, ref64, ref32):
    """(rho, per-element bound [rows, n], rows that are not live) from the references alone"""
    want, r32 = _rows(ref64), _rows(ref32)
    if name == ZERO_BIAS:
        return 0.0, torch.full_like(want, ZERO_BIAS_TOL), 0
    tmax = float(want.abs().max()) if want.numel() else 0.0
    rmax = want.abs().amax(dim=1)
    err = (r32 - want).abs()
    e32, e32_r = (float(err.max()) if err.numel() else 0.0), err.amax(dim=1)
    live = (rmax >= LIVE * tmax) & (rmax > 0)
    rho = float((e32_r[live] / rmax[live]).max()) if bool(live.any()) else 0.0
    bound = torch.where(live, FACTOR * rho * rmax, torch.full_like(rmax, FACTOR * e32))
    return rho, bound.unsqueeze(1).expand_as(want), int((~live).sum())


def row_precondition(name, ref64, ref32, tol):
    """rho <= tol / 4: no row's bar is looser than the tensor-level tolerance the suite had, taken against the row's maximum"""
    rho, _, dead = row_yardstick(name, ref64, ref32)
    assert rho <= tol / FACTOR, "%s: CPU-fp32 row-relative error %.3e exceeds %.1e / 4: the case is ill-conditioned" % (
        name, rho, tol)
    return rho, dead


def row_ok(kernel, name, got, ref64, ref32, tol):
    """|got - ref64| <= 4 rho |row max| on a live row, 4 x (CPU-fp32 worst element error) on a row below 1e-6 of the
    tensor's maximum; full_att.bias: absolute 1e-4"""
    rho, bound, _ = row_yardstick(name, ref64, ref32)
    assert rho <= tol / FACTOR, "%s %s: yardstick rho %.3e > %.1e / 4" % (kernel, name, rho, tol)      # before `got` is looked at
    want = _rows(ref64)
    got = got.double().reshape(want.shape)
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * 1e30).nan_to_num(1e30)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s %s: worst err/bound %.3f (rho %.3e)" % (kernel, name, worst, rho))
    ok = bool((err <= bound).all())
    if ok:
        _note(kernel, name, worst, "=absolute 1e-4 (a zero in exact arithmetic)" if name == ZERO_BIAS else "row", rho)
    assert ok, "%s %s: worst err/bound %.3f in row %d (rho %.3e), %d NaN" % (
        kernel, name, worst, int(ratio.amax(dim=1).argmax()), rho, int(got.isnan().sum()))


def tol_of(name):
    return TOL_OUT if name in ("preds", "alphas") else TOL_GRAD


# ---- the carve of `saved` (csrc/sequence.cpp carve_saved) -------------------------------------------------------------------
def saved_layout(c):
    """[(name, offset, shape, batch axis)] in floats; the two bf16 copies are (name, offset, (B, n), 0) in 16-bit elements"""
    B, P, E, A, D, Fd, M, S, V, T, L, att = c.dims
    F4, Q = 4 * Fd, c.Q
    items = []
    if att:
        items.append(("att1", (B, P, A), 0))
    items += [("qx", (B, F4), 0), ("qh", (B, F4), 0), ("ex", (T, B, F4), 1), ("emb_tm", (T, B, M), 1), ("mean_enc", (B, E), 0),
              ("Hs", (T + 1, B, D), 1), ("Cs", (T + 1, B, D), 1)]
    if att:
        items += [("att2_all", (T, B, A), 1), ("alpha_tm", (T, B, P), 1), ("awe_all", (T, B, E), 1), ("gate_all", (T, B, E), 1),
                  ("z_all", (T, B, E), 1)]
    items += [("pa_all", (T, B, F4), 1), ("ph_all", (T, B, F4), 1), ("gates_all", (T, B, 4 * D), 1), ("tanhc_all", (T, B, D), 1),
              ("Hd_bm", (B, T, D), 0), ("rowmask", (B, T), 0)]
    if att and Q:
        items.append(("alphaq_tm", (T, B, Q), 1))
    out, off = [], 0
    for name, shape, ax in items:
        n = 1
        for s in shape:
            n *= s
        out.append((name, off, shape, ax))
        off += (n + 63) & ~63
    if att:
        for name, n in (("att1h", P * A), ("ench", (Q or P) * E)):
            out.append((name, off, (B, n), 0))
            off += ((B * n + 1) // 2 + 63) & ~63
    return out, off


def saved_rows(c, saved, keep):
    """the saved state of the batch rows `keep` (index tensor): name -> tensor"""
    layout, _ = saved_layout(c)
    got = {}
    for name, off, shape, ax in layout:
        if name in ("att1h", "ench"):
            n = shape[0] * shape[1]
            t = saved[off:off + (n + 1) // 2].view(torch.int16)[:n].view(shape)
        else:
            n = 1
            for s in shape:
                n *= s
            t = saved[off:off + n].view(shape)
        got[name] = t.index_select(ax, keep)
    return got


# ---- the call pair ----------------------------------------------------------------------------------------------------------
class PBuf:
    """a dense window the caller owns (a view of a module-wide allocation): .ptr / .read() like GBuf"""

    def __init__(self, t):
        self.t, self.ptr = t, C.c_void_p(t.data_ptr())

    def read(self, what):
        return self.t.cpu()


def workspace_floats(dev, c):
    """(saved, scratch) in floats, as scnattn_seq_workspace reports them; the pool descriptor or None"""
    from scnattn import _lib
    from scnattn.functional import pool_taps
    pool = pool_taps(HIN, HIN, HOUT, HOUT, dev) if c.pooled else None
    d = _lib.Dims(*c.dims)
    sv, sc = C.c_size_t(), C.c_size_t()
    _lib.call("scnattn_seq_workspace", C.byref(d), None if pool is None else C.byref(pool.cstruct), C.byref(sv), C.byref(sc))
    assert sv.value % 4 == 0 and sc.value % 4 == 0
    assert saved_layout(c)[1] == sv.value // 4, "tests/seq_driver_refs.py saved_layout disagrees with carve_saved"
    return sv.value // 4, sc.value // 4, pool


def run_driver(dev, c, saved, fscratch, bscratch, skip=(), dalphas="given", alphas_fill=0.0, bwd=True, fwd=True):
    """scnattn_seq_fwd, then scnattn_seq_bwd, on the caller's workspaces (objects with .ptr and .read(): GBig, PBuf), which
    the caller sized by workspace_floats and filled.  Every output is a guarded window (GBuf) in the sentinel -- alphas
    pre-filled with `alphas_fill`, the embedding gradient with zeros, as the header asks.  skip: names of gradient fields,
    "denc", "dtags" passed as NULL.  dalphas: "given", "zeros" or None (NULL).  fwd = False: the backward alone on a `saved`
    that a forward filled.  Returns name -> host tensor: preds, alphas, saved, "g." + key, denc, dtags."""
    from scnattn import _lib
    from scnattn.functional import _params_struct
    _, _, pool = workspace_floats(dev, c)
    cpool = None if pool is None else C.byref(pool.cstruct)
    d = _lib.Dims(*c.dims)
    B, P, E, A, D, Fd, M, S, V, T, L, att = c.dims
    up = lambda t: None if t is None else t.to(dev).contiguous()      # noqa: E731
    wts = [None if k is None else up(c.sd[k]) for _, k in c.fields]
    enc, tags, caps, mask, dpreds = up(c.enc), up(c.tags), up(c.caps), up(c.mask), up(c.dpreds)
    dl = torch.tensor(c.dl, dtype=torch.int32, device=dev)
    dal = None
    if att and dalphas is not None:
        dal = up(c.dalphas if dalphas == "given" else torch.zeros_like(c.dalphas))
    bt = (C.c_int32 * T)(*c.bt_host)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = _lib.ptr
    w = _params_struct(wts)
    out, bufs = {}, {}
    if fwd:
        bufs["preds"] = GBuf(dev, (B, T, V), out=True)
        if att:
            bufs["alphas"] = GBuf(dev, (B, T, P), vals=torch.full((B, T, P), alphas_fill), out=True)
        _lib.call("scnattn_seq_fwd", st, C.byref(d), C.byref(w), ptr(enc), ptr(tags), ptr(caps), ptr(dl), C.cast(bt, C.c_void_p),
                  ptr(mask), saved.ptr, fscratch.ptr, bufs["preds"].ptr, bufs["alphas"].ptr if att else None, cpool)
        torch.cuda.synchronize()
        if hasattr(fscratch, "check"):
            fscratch.check("forward scratch")
    if bwd:
        gbufs = []
        for f, k in c.fields:
            if k is None or f in skip:
                gbufs.append(None)
                continue
            shape = c.sd[k].shape
            gb = GBuf(dev, shape, vals=torch.zeros(shape) if f == "embedding_weight" else None, out=True)
            gbufs.append(gb)
            bufs["g." + k] = gb
        gs = _lib.Params()
        for (f, _), gb in zip(c.fields, gbufs):
            setattr(gs, f, None if gb is None else gb.ptr.value)
        if "denc" not in skip:
            bufs["denc"] = GBuf(dev, c.enc.shape, out=True)
        if "dtags" not in skip:
            bufs["dtags"] = GBuf(dev, c.tags.shape, out=True)
        _lib.call("scnattn_seq_bwd", st, C.byref(d), C.byref(w), ptr(enc), ptr(tags), ptr(caps), ptr(dl), C.cast(bt, C.c_void_p),
                  ptr(mask), saved.ptr, bscratch.ptr, ptr(dpreds), ptr(dal), C.byref(gs),
                  bufs["denc"].ptr if "denc" in bufs else None, bufs["dtags"].ptr if "dtags" in bufs else None, cpool)
        torch.cuda.synchronize()
        if hasattr(bscratch, "check"):
            bscratch.check("backward scratch")
    for name, b in bufs.items():
        out[name] = b.read("%s %s" % (c.id, name))
    out["saved"] = saved.read("saved")
    return out


def same_bits(a, b, what, names=None):
    """two result dicts of run_driver: the named results (default: all that both have but `saved`) are torch.equal"""
    names = [n for n in a if n in b and n != "saved"] if names is None else names
    bad = [n for n in names if not torch.equal(a[n], b[n])]
    assert not bad, "%s: %s differ" % (what, ", ".join(bad))


# ---- module-level cases: the Python glue (sort, permutation, bt_host) judged the same way -----------------------------------
MODULE_KINDS = ("attention_scn", "pure_scn", "pure_attention")


@functools.lru_cache(maxsize=None)
def module_case(kind):
    """an unsorted ragged batch through the nn.Module of `kind` (PureAttention reaches the drivers as an SCN whose tag
    factors are switched off): (module on the CPU, inputs, upstream weights, ref64, ref32)"""
    from oracle import scnattn_ref as R
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    A, M, D, Fd, Sd, E = M4
    V, B, L = 50, 6, 9
    torch.manual_seed(3000 + MODULE_KINDS.index(kind))
    m = {"attention_scn": lambda: AttentionSCN(A, M, D, Fd, Sd, V, encoder_dim=E, dropout=0.0),
         "pure_scn": lambda: PureSCN(M, D, Fd, Sd, V, encoder_dim=E, dropout=0.0),
         "pure_attention": lambda: PureAttention(A, M, D, V, encoder_dim=E, dropout=0.0)}[kind]()
    g = torch.Generator().manual_seed(3100 + MODULE_KINDS.index(kind))
    enc, tags = torch.rand(B, HIN, HIN, E, generator=g), torch.rand(B, Sd, generator=g)
    ln = torch.tensor([3, 9, 5, 9, 2, 7])
    caps, caplens = torch.randint(1, V - 3, (B, L), generator=g), ln.unsqueeze(1)
    si = torch.sort(ln, descending=True, stable=True)[1]
    wp, wa = torch.randn(B, L - 1, V, generator=g), torch.randn(B, L - 1, HIN * HIN, generator=g)
    refs = []
    for dtype in (torch.float64, torch.float32):
        P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in m.state_dict().items()}
        e1, t1 = enc.clone().to(dtype).requires_grad_(True), tags.clone().to(dtype).requires_grad_(True)
        if kind == "attention_scn":
            pr, _, _, al, _ = R.attention_scn_forward(P, e1, t1, caps, caplens, sort_ind=si)
        elif kind == "pure_scn":
            (pr, _, _, _), al = R.pure_scn_forward(P, e1, t1, caps, caplens, sort_ind=si), None
        else:
            pr, _, _, al, _ = R.pure_attention_forward(P, e1, caps, caplens, sort_ind=si)
        loss = (pr * wp.to(dtype)).sum() + (0 if al is None else (al * wa.to(dtype)).sum())
        wrt = [P[k] for k in P] + [e1] + ([] if kind == "pure_attention" else [t1])
        grads = torch.autograd.grad(loss, wrt, allow_unused=True)
        out = {"preds": pr.detach()}
        if al is not None:
            out["alphas"] = al.detach()
        names = ["g." + k for k in P] + ["denc"] + ([] if kind == "pure_attention" else ["dtags"])
        for n, x, gr in zip(names, wrt, grads):
            out[n] = torch.zeros_like(x) if gr is None else gr
        refs.append(out)
    return m, (enc, tags, caps, caplens, si), (wp, wa), refs[0], refs[1]
