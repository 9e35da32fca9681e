"""torch.autograd.Function wrappers over the C ABI (libscnattn.so).

Everything numerical happens in the HIP kernels; this file only allocates torch tensors (so the
caching allocator and stream semantics apply), passes raw pointers, and wires autograd.  The math each
wrapper covers, by reference file:
  decoder_sequence -> models/decoders/attention_scn.py:124-156, pure_scn.py:114-138
  scn_cell         -> models/scn_cell.py:52-154
  attention        -> models/attention.py:26-44
  pool_permute     -> models/encoders/caption.py:41-43
  tag_head_loss    -> models/encoders/tagger.py:24-31 + trains/tagger.py:161-163,176 (BCELoss, binary_accuracy)
"""
import ctypes as C
import threading

import torch

from . import _lib
from ._lib import Pool, Dims, Params, PARAM_FIELDS, call, ptr, stream_of, f32c, require_cuda


# ----------------------------------------------------------------------------------------------
# thin primitive helpers
# ----------------------------------------------------------------------------------------------
def gemm(a, b, ta=False, tb=False, bias=None, out=None, beta=0.0, alpha=1.0, M=None, N=None, K=None,
         lda=None, ldb=None, ldc=None, batch=1, sa=0, sb=0, sc=0, rowmask=None):
    """out = alpha*op(a).op(b) + beta*out + bias; all sizes/strides may be overridden to address
    sub-blocks of larger row-major buffers."""
    if M is None:
        M = a.shape[1] if ta else a.shape[0]
    if K is None:
        K = a.shape[0] if ta else a.shape[1]
    if N is None:
        N = b.shape[0] if tb else b.shape[1]
    lda = a.stride(0) if lda is None else lda
    ldb = b.stride(0) if ldb is None else ldb
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    ldc = out.stride(0) if ldc is None else ldc
    ws = _gemm_workspace(a.device)
    call("scnattn_sgemm_ws", stream_of(a), int(ta), int(tb), M, N, K, alpha, ptr(a), lda, ptr(b), ldb, beta,
         ptr(out), ldc, ptr(bias), ptr(rowmask), batch, sa, sb, sc, ptr(ws), ws.numel())
    return out


_gemm_ws = {}


def _gemm_workspace(dev):
    """32 MiB of split-K partial sums per (device, stream): the stand-alone modules' GEMMs have few rows (beam
    search: k <= 5, PureAttention at batch 4), where the tile grid alone leaves most of the chip idle."""
    # per host thread too: a GEMM is two launches (partials, then their reduction) and two threads enqueueing on
    # one stream could interleave them
    key = (dev, torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device()),
           threading.get_ident())
    ws = _gemm_ws.get(key)
    if ws is None:
        ws = _gemm_ws[key] = torch.empty(24 << 20, device=dev, dtype=torch.float32)
    return ws


def colsum(x, R=None, N=None, ld=None):
    R = x.shape[0] if R is None else R
    N = x.shape[1] if N is None else N
    ld = x.stride(0) if ld is None else ld
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    call("scnattn_colsum", stream_of(x), R, N, ptr(x), ld, ptr(out), 0.0)
    return out


def set_option(name, value):
    call("scnattn_set_option", name.encode(), int(value))


# ----------------------------------------------------------------------------------------------
# whole-sequence decoder
# ----------------------------------------------------------------------------------------------
def _params_struct(tensors):
    p = Params()
    for name, t in zip(PARAM_FIELDS, tensors):
        setattr(p, name, None if t is None else t.data_ptr())
    return p


class PoolTaps:
    """`encoder_out = AdaptiveAvgPool2d(out)(x)` (models/encoders/caption.py:20,41) as tap tables: pooled pixel p
    averages <= 4 source pixels (the pool up-samples: 8x8 -> 14x14 windows are 1 or 2 wide), `matrix()` is the
    dense (P, Q) pooling matrix they encode.  Device tensors + the scnattn_pool struct the C ABI takes."""

    def __init__(self, in_h, in_w, out_h, out_w, device):
        def windows(n_in, n_out):     # torch's adaptive pooling windows: [floor(i*n/o), ceil((i+1)*n/o))
            return [(i * n_in // n_out, -(-(i + 1) * n_in // n_out)) for i in range(n_out)]
        rows, cols = windows(in_h, out_h), windows(in_w, out_w)
        P, Q = out_h * out_w, in_h * in_w
        tap_idx = torch.zeros(P, 4, dtype=torch.int32)
        tap_w = torch.zeros(P, 4, dtype=torch.float32)
        per_q = [[] for _ in range(Q)]
        for i, (r0, r1) in enumerate(rows):
            for j, (c0, c1) in enumerate(cols):
                p = i * out_w + j
                src = [(r, c) for r in range(r0, r1) for c in range(c0, c1)]
                if len(src) > 4:
                    raise ValueError("pooling window of %d pixels: the pooled path handles up-sampling pools "
                                     "(windows of at most 2x2)" % len(src))
                for k, (r, c) in enumerate(src):
                    q = r * in_w + c
                    tap_idx[p, k] = q
                    tap_w[p, k] = 1.0 / len(src)
                    per_q[q].append((p, 1.0 / len(src)))
        qmax = max(len(l) for l in per_q)
        qtap_idx = torch.full((Q, qmax), -1, dtype=torch.int32)
        qtap_w = torch.zeros(Q, qmax, dtype=torch.float32)
        for q, l in enumerate(per_q):
            for k, (p, wv) in enumerate(l):
                qtap_idx[q, k] = p
                qtap_w[q, k] = wv
        col_w = (qtap_w.double().sum(dim=1) / P).float()
        self.P, self.Q, self.qmax, self.shape = P, Q, qmax, (in_h, in_w, out_h, out_w)
        self.tap_idx, self.tap_w = tap_idx.to(device), tap_w.to(device)
        self.qtap_idx, self.qtap_w, self.col_w = qtap_idx.to(device), qtap_w.to(device), col_w.to(device)
        self.cstruct = Pool(Q, qmax, self.tap_idx.data_ptr(), self.tap_w.data_ptr(), self.qtap_idx.data_ptr(),
                            self.qtap_w.data_ptr(), self.col_w.data_ptr())

    def matrix(self):
        m = torch.zeros(self.P, self.Q, dtype=torch.float32, device=self.tap_w.device)
        m.scatter_add_(1, self.tap_idx.long(), self.tap_w)
        return m


_pool_cache = {}


def pool_taps(in_h, in_w, out_h, out_w, device):
    key = (in_h, in_w, out_h, out_w, str(device))
    if key not in _pool_cache:
        _pool_cache[key] = PoolTaps(in_h, in_w, out_h, out_w, device)
    return _pool_cache[key]


_POISON = False     # tests: NaN-fill workspaces that are claimed to be fully overwritten


def _workspace(nfloats, dev, fully_written):
    if not fully_written:
        return torch.zeros(nfloats, device=dev, dtype=torch.float32)
    ws = torch.empty(nfloats, device=dev, dtype=torch.float32)
    if _POISON:
        ws.fill_(float("nan"))
    return ws


class _DecoderSeq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, enc, tags, caps, dl_dev, drop_mask, *weights):
        dims_t, bt_host, pool = meta       # pool: PoolTaps or None; with it `enc` is the un-pooled map (B, Q, E)
        d = Dims(*dims_t)
        cpool = None if pool is None else C.byref(pool.cstruct)
        require_cuda(enc, tags, caps, dl_dev, *weights)
        dev = enc.device
        enc, tags = f32c(enc), f32c(tags)
        caps = caps.contiguous()
        weights = tuple(None if w is None else f32c(w.detach()) for w in weights)
        drop_mask = f32c(drop_mask)
        sv, sc = C.c_size_t(), C.c_size_t()
        call("scnattn_seq_workspace", C.byref(d), cpool, C.byref(sv), C.byref(sc))
        # Rows (t, b >= b_t) of the time-major buffers are never written by the kernels but are read by the
        # post-loop GEMMs (and returned, for alphas), so they must be zero -- unless every row decodes at every
        # step (fixed-length captions), where each element is written before it is read and the 120 MB fill is
        # skipped.  `_POISON` (tests) fills with NaN instead to prove exactly that.
        full = min(bt_host) == d.B
        saved = _workspace(sv.value // 4, dev, full)
        # the forward's scratch needs no fill, ragged or not (include/scnattn.h): every word is written before it is read
        scratch = _workspace(sc.value // 4, dev, True)
        preds = torch.empty((d.B, d.T, d.V), device=dev, dtype=torch.float32)
        alphas = _workspace(d.B * d.T * d.P, dev, full).view(d.B, d.T, d.P) if d.has_att else None
        bt = (C.c_int32 * d.T)(*bt_host)
        w = _params_struct(weights)
        call("scnattn_seq_fwd", stream_of(enc), C.byref(d), C.byref(w), ptr(enc), ptr(tags), ptr(caps), ptr(dl_dev),
             C.cast(bt, C.c_void_p), ptr(drop_mask), ptr(saved), ptr(scratch), ptr(preds), ptr(alphas), cpool)
        ctx.meta = (dims_t, tuple(bt_host), sc.value, pool)
        ctx.save_for_backward(enc, tags, caps, dl_dev, drop_mask, saved, *[x for x in weights if x is not None])
        ctx.wmask = tuple(x is not None for x in weights)
        if alphas is None:
            alphas = preds.new_zeros(0)
            ctx.mark_non_differentiable(alphas)
        return preds, alphas

    @staticmethod
    def backward(ctx, dpreds, dalphas):
        dims_t, bt_host, scratch_bytes, pool = ctx.meta
        d = Dims(*dims_t)
        cpool = None if pool is None else C.byref(pool.cstruct)
        enc, tags, caps, dl_dev, drop_mask, saved, *wl = ctx.saved_tensors
        it = iter(wl)
        weights = tuple(next(it) if m else None for m in ctx.wmask)
        dev = enc.device
        dpreds = f32c(dpreds)
        dalphas = f32c(dalphas) if (d.has_att and dalphas is not None) else None
        scratch = _workspace(scratch_bytes // 4, dev, min(bt_host) == d.B)
        need = ctx.needs_input_grad  # (meta, enc, tags, caps, dl, mask, *weights)
        grads = []
        for i, (name, wt) in enumerate(zip(PARAM_FIELDS, weights)):
            if wt is None or not need[6 + i]:
                grads.append(None)
            elif name == "embedding_weight":
                grads.append(torch.zeros_like(wt))
            else:
                grads.append(torch.empty_like(wt))
        denc = torch.empty_like(enc) if need[1] else None
        dtags = torch.empty_like(tags) if need[2] else None
        bt = (C.c_int32 * d.T)(*bt_host)
        w, g = _params_struct(weights), _params_struct(grads)
        call("scnattn_seq_bwd", stream_of(enc), C.byref(d), C.byref(w), ptr(enc), ptr(tags), ptr(caps), ptr(dl_dev),
             C.cast(bt, C.c_void_p), ptr(drop_mask), ptr(saved), ptr(scratch), ptr(dpreds), ptr(dalphas),
             C.byref(g), ptr(denc), ptr(dtags), cpool)
        return (None, denc, dtags, None, None, None, *grads)


def decoder_sequence(dims, bt_host, enc, tags, caps, dl_dev, drop_mask, weights, pool=None):
    """dims: 12-tuple in scnattn_dims order; weights: tensors in PARAM_FIELDS order (None = absent).
    pool: PoolTaps -- then `enc` is the un-pooled feature map (B, Q, E) and the pooled encoder_out is never
    built.  Returns (predictions (B,T,V), alphas (B,T,P) or None)."""
    if pool is not None and (enc.dim() != 3 or enc.shape[1] != pool.Q or dims[1] != pool.P):
        raise RuntimeError("decoder_sequence: the un-pooled map must be (B, %d, E) for this pool" % pool.Q)
    preds, alphas = _DecoderSeq.apply((tuple(dims), tuple(bt_host), pool), enc, tags, caps, dl_dev, drop_mask, *weights)
    return preds, (alphas if dims[-1] else None)


# ----------------------------------------------------------------------------------------------
# batched beam search (include/scnattn.h: scnattn_beam_*)
# ----------------------------------------------------------------------------------------------
BEAM_MAX_STEPS = 51       # the reference leaves its loop when `step > 50` holds after a step
BEAM_CHUNK = 8            # steps enqueued between two looks at the open-image counter
_BEAM_RESULTS = ("open_images", "nsrc", "kk", "ncomp", "best_idx", "best_score", "scores", "comp_score", "comp_step",
                 "comp_parent", "token", "parent", "alpha")
_BEAM_FLOAT = ("best_score", "scores", "comp_score", "alpha")


def _run_on_device(fmt, head, noff, init_tail, steps_tail, st, dev, max_steps, chunk, guard):
    """What beam_search_run, ensemble_search_run and rollout_run share.  fmt % "workspace" / "layout" / "init" / "steps" name
    the four calls of one driver and `head` is what all four take first (dims, K, max_steps, ...):
        workspace(*head, &bytes), layout(*head, off[noff])
        the allocation; guard > 0 (tests): that many sentinel words behind the workspace
        init(stream, *head, *init_tail, ws)         zero-fills what needs it
        steps(stream, *head, *steps_tail, t, n, ws) in chunks of `chunk` steps, with one 4-byte copy (and sync) per chunk:
                                                    the driver's open counter at off[0]
    Returns (ws, off, nwords, t): the workspace (float32, nwords + guard words), the offsets, and the steps that ran."""
    nbytes = C.c_size_t()
    call(fmt % "workspace", *head, C.byref(nbytes))
    off = (C.c_long * noff)()
    call(fmt % "layout", *head, off)
    nwords = nbytes.value // 4
    ws = torch.empty(nwords + guard, device=dev, dtype=torch.float32)
    wsi = ws.view(torch.int32)
    if guard:
        wsi[nwords:].fill_(0x7FC5A5A5)
    call(fmt % "init", st, *head, *init_tail, ptr(ws))
    t = 0
    while t < max_steps:
        n = min(chunk, max_steps - t)
        call(fmt % "steps", st, *head, *steps_tail, t, n, ptr(ws))
        t += n
        if int(wsi[off[0]]) == 0:
            break
    return ws, off, nwords, t


def search_options_struct(options, vocab_size, beam_size, max_steps, end_token):
    """a models.decoders.SearchOptions -> scnattn_search_options, after its refusals for this search (ValueError)"""
    options.check(vocab_size, beam_size, max_steps, end_token)
    o = _lib.SearchOpts(min_length=options.min_length, no_repeat_ngram=options.no_repeat_ngram,
                        n_banned=len(options.banned_tokens))
    for i, tok in enumerate(options.banned_tokens):
        o.banned[i] = tok
    return o


def diversity_struct(groups, diversity, beam_size):
    """(groups, diversity) of a search whose TOTAL beam size is beam_size -> scnattn_diversity, after its refusals
    (ValueError): groups >= 1 dividing beam_size, a finite penalty >= 0"""
    import math
    if int(groups) != groups or groups < 1:
        raise ValueError("groups must be an integer >= 1 (got %r)" % (groups,))
    if beam_size % int(groups) != 0:
        raise ValueError("beam_size %d (the total over the groups) is not a multiple of groups %d" % (beam_size, groups))
    diversity = float(diversity)
    if not (math.isfinite(diversity) and diversity >= 0.0):
        raise ValueError("the diversity penalty must be finite and not negative (got %r)" % (diversity,))
    return _lib.Diversity(groups=int(groups), penalty=diversity)


def required_table(required, N, V, beam_size, max_steps, start_token, end_token, pad_token=-1, options=None):
    """The refusals of a constrained search (include/scnattn.h; ValueError) -> the int32 table [N][4] as a ctypes array:
    `required` holds per image a sequence of at most 4 distinct token ids in [0, V), none of them <start>, <end>, <pad> or
    banned by `options`; beam_size in [1, 8]; and every row must still offer beam_size ordinary candidates:
    V - banned - 1 - (no_repeat_ngram ? max_steps : 0) - 4 >= beam_size."""
    if not 1 <= beam_size <= _lib.MAX_BEAM:
        raise ValueError("beam_size must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, beam_size))
    required = [list(r) for r in required]
    if len(required) != N:
        raise ValueError("required: %d lists for %d images" % (len(required), N))
    banned = set(options.banned_tokens) if options is not None else set()
    ngram = options.no_repeat_ngram if options is not None else 0
    tab = (C.c_int32 * (N * _lib.MAX_REQUIRED))(*([-1] * (N * _lib.MAX_REQUIRED)))
    for n, words in enumerate(required):
        if len(words) > _lib.MAX_REQUIRED:
            raise ValueError("required: image %d has %d words, at most %d" % (n, len(words), _lib.MAX_REQUIRED))
        for i, w in enumerate(words):
            if isinstance(w, bool) or int(w) != w:
                raise ValueError("required: image %d: %r is not a token id" % (n, w))
            w = int(w)
            if not 0 <= w < V:
                raise ValueError("required: image %d: token %d lies outside the vocabulary" % (n, w))
            if w in (start_token, end_token, pad_token):
                raise ValueError("required: image %d: <start>, <end> and <pad> may not be required (token %d)" % (n, w))
            if w in banned:
                raise ValueError("required: image %d: token %d is banned by the search options" % (n, w))
            if w in [int(x) for x in words[:i]]:
                raise ValueError("required: image %d: token %d occurs twice" % (n, w))
            tab[n * _lib.MAX_REQUIRED + i] = w
    if V - len(banned) - 1 - (max_steps if ngram >= 1 else 0) - _lib.MAX_REQUIRED < beam_size:
        raise ValueError("options and required words may leave a beam fewer than beam_size candidates (need vocab_size - "
                         "banned - 1 - (no_repeat_ngram ? max_steps : 0) - %d >= beam_size)" % _lib.MAX_REQUIRED)
    return tab


def _search_form(options, groups, diversity, V, beam_size, max_steps, end_token, required=None, N=0, start_token=-1,
                 pad_token=-1):
    """(suffix of the four calls, what they take behind max_steps / alpha_member, offsets): the plain
    calls, the _opt form with options, only when groups > 1 the _div form, whose options may be NULL, and with `required`
    (a list per image, empty lists included) the _con form, likewise -- which groups > 1 may not join"""
    div = diversity_struct(groups, diversity, beam_size)
    opt = None if options is None else search_options_struct(options, V, beam_size, max_steps, end_token)
    if required is not None:
        if div.groups > 1:
            raise ValueError("required words and groups do not compose: a search takes one or the other")
        tab = required_table(required, N, V, beam_size, max_steps, start_token, end_token, pad_token, options)
        con = _lib.Constraints(n_images=N, pad_token=pad_token, required=C.addressof(tab))
        con._table = tab        # the host table lives as long as the struct
        return "_con", (C.byref(opt) if opt is not None else None, C.byref(con)), _lib.BEAM_NOFF_CON
    if div.groups > 1:
        return "_div", (C.byref(opt) if opt is not None else None, C.byref(div)), _lib.BEAM_NOFF_OPT
    if opt is not None:
        return "_opt", (C.byref(opt),), _lib.BEAM_NOFF_OPT
    return "", (), _lib.BEAM_NOFF


def beam_search_run(dims, beam_size, weights, enc, tags, start_token, end_token, max_steps=BEAM_MAX_STEPS,
                    chunk=BEAM_CHUNK, guard=0, options=None, groups=1, diversity=0.0, required=None, pad_token=-1):
    """The whole search of N images on the device.  dims: 12-tuple in scnattn_dims order with B = N (T, L unused);
    enc (N, P, E) as the caller has it (no copy per beam), tags (N, S) un-expanded; weights in PARAM_FIELDS order.
    Returns (results, steps): host tensors by the names of scnattn_beam_layout -- token / parent (steps, N*K),
    alpha (steps, N*K, P) or None -- and the number of steps that ran.  guard > 0 (tests): that many sentinel words
    behind the workspace, returned as results["guard"] (host int32).
    options: a models.decoders.SearchOptions runs the scnattn_beam_*_opt calls (its length_penalty is the caller's
    business: trace_back) and adds results["history"] (N*K, steps) int32, the words of the beam in every slot; None: the
    plain search, and results["history"] is None.
    groups > 1: a DIVERSE search (include/scnattn.h; the scnattn_beam_*_div calls) in `groups` groups of beam_size / groups
    slots with the penalty `diversity`; beam_size is the total.  nsrc / kk / ncomp / best_idx / best_score then hold
    N * groups entries, entry n * groups + g.  groups == 1 takes today's entry points, whatever `diversity` says.
    required: per image a sequence of at most 4 token ids -> a CONSTRAINED search (include/scnattn.h; the scnattn_beam_*_con
    calls, also when every list is empty); results["met"] (N*K,) int32 then holds the masks of the slots after the last step
    and results["required"] the table (N, 4); None: no constraints, and the results have neither entry."""
    require_cuda(enc, tags, *weights)
    if not 1 <= beam_size <= _lib.MAX_BEAM:
        raise ValueError("beam_size must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, beam_size))
    d = Dims(*dims)
    if d.V < beam_size:
        raise ValueError("vocab_size %d is smaller than beam_size %d" % (d.V, beam_size))
    # with options: the same four calls in their _opt form, the options struct after max_steps; in groups: the _div form
    sfx, opt, noff = _search_form(options, groups, diversity, d.V, beam_size, max_steps, end_token, required, d.B,
                                  start_token, pad_token)
    dev = enc.device
    enc, tags = f32c(enc), f32c(tags)
    weights = tuple(None if w is None else f32c(w.detach()) for w in weights)
    w = _params_struct(weights)
    K, N = beam_size, d.B
    ws, off, nwords, t = _run_on_device("scnattn_beam_%s" + sfx, (C.byref(d), K, max_steps, *opt), noff,
                                        (C.byref(w), ptr(enc), ptr(tags), start_token), (C.byref(w), ptr(enc), end_token),
                                        stream_of(enc), dev, max_steps, chunk, guard)
    return _beam_results(ws, off, N, K, d.P, t, nwords, guard, max_steps, groups=int(groups)), t


def _beam_results(ws, off, N, K, P, t, nwords, guard, max_steps=BEAM_MAX_STEPS, groups=1):
    """the host tensors of a finished search (t steps ran), by the names of scnattn_beam_layout; "history" (N*K, t): the
    current one of the two history buffers of a search with options (scnattn_beam_layout_opt), None without; the
    per-group arrays of a search in groups hold N * groups entries; "met" (N*K,) and "required" (N, 4) of a constrained
    search (scnattn_beam_layout_con), absent without"""
    wsi = ws.view(torch.int32)
    R, NG = N * K, N * groups
    met = req = None
    if len(off) >= _lib.BEAM_NOFF_CON:
        met = wsi[off[_lib.BEAM_NOFF_OPT]:off[_lib.BEAM_NOFF_OPT] + R].cpu()
        req = wsi[off[_lib.BEAM_NOFF_OPT + 1]:off[_lib.BEAM_NOFF_OPT + 1] + N * _lib.MAX_REQUIRED].view(N, _lib.MAX_REQUIRED).cpu()
    hist = None
    if len(off) > _lib.BEAM_NOFF and off[_lib.BEAM_NOFF] >= 0:
        cur = off[_lib.BEAM_NOFF] + (t & 1) * R * max_steps
        hist = wsi[cur:cur + R * max_steps].view(R, max_steps)[:, :t].cpu()
    sizes = {"open_images": 1, "nsrc": NG, "kk": NG, "ncomp": NG, "best_idx": NG, "best_score": NG, "scores": R,
             "comp_score": R, "comp_step": R, "comp_parent": R, "token": t * R, "parent": t * R, "alpha": t * R * P}
    out = {}
    for i, name in enumerate(_BEAM_RESULTS):
        if off[i] < 0:
            out[name] = None
            continue
        src = ws if name in _BEAM_FLOAT else wsi
        out[name] = src[off[i]:off[i] + sizes[name]].cpu()
    out["token"], out["parent"] = out["token"].view(t, R), out["parent"].view(t, R)
    if out["alpha"] is not None:
        out["alpha"] = out["alpha"].view(t, R, P)
    out["history"] = hist
    if met is not None:         # only a constrained search has these entries
        out["met"], out["required"] = met, req
    if guard:
        out["guard"] = wsi[nwords:].cpu()
    return out


# ----------------------------------------------------------------------------------------------
# ensemble beam search (include/scnattn.h: scnattn_ensemble_*)
# ----------------------------------------------------------------------------------------------
ENSEMBLE_MODES = {"logprob": 0, "prob": 1}


def normalise_member_weights(weights, M):
    """M positive finite weights -> the fp32 values the kernel takes: normalised to sum 1 in fp64, then rounded.
    None: equal weights."""
    import math
    if weights is None:
        weights = [1.0] * M
    weights = [float(x) for x in weights]
    if len(weights) != M:
        raise ValueError("ensemble: %d weights for %d members" % (len(weights), M))
    if not all(math.isfinite(x) and x > 0.0 for x in weights):
        raise ValueError("ensemble: member weights must be positive and finite (got %r)" % (weights,))
    total = math.fsum(weights)
    out = [C.c_float(x / total).value for x in weights]
    if not all(math.isfinite(x) and x > 0.0 for x in out):
        raise ValueError("ensemble: a member weight vanishes in fp32 after normalisation (got %r)" % (weights,))
    return out


def ensemble_search_run(dims_list, beam_size, weights_list, enc, tags_list, member_weights, mode, start, end, alpha_member,
                        max_steps=BEAM_MAX_STEPS, chunk=BEAM_CHUNK, guard=0, options=None, groups=1, diversity=0.0,
                        required=None, pad_token=-1):
    """beam_search_run for an ensemble of M <= 4 decoders under one search state (csrc/beam_search.cpp:
    scnattn_ensemble_*): dims_list / weights_list / tags_list hold one entry per member, as beam_search_run takes them;
    enc (N, P, E) is shared.  member_weights: M positive numbers (None: equal), normalised here; mode: "logprob" / 0 (the
    weighted mean of the members' log-probabilities) or "prob" / 1 (the log of the weighted mean of their probabilities).
    alpha_member: the member whose attention maps are kept (-1 or None: none).  Returns (results, steps) exactly as
    beam_search_run does; `guard`, `options`, `groups`, `diversity`, `required` and `pad_token` have the same meaning."""
    M = len(dims_list)
    if not 1 <= M <= _lib.MAX_ENSEMBLE:
        raise ValueError("an ensemble has 1 to %d members (got %d)" % (_lib.MAX_ENSEMBLE, M))
    if len(weights_list) != M or len(tags_list) != M:
        raise ValueError("ensemble_search_run: dims, weights and tags must have one entry per member")
    if not 1 <= beam_size <= _lib.MAX_BEAM:
        raise ValueError("beam_size must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, beam_size))
    mode = ENSEMBLE_MODES.get(mode, mode)
    if mode not in (0, 1):
        raise ValueError("ensemble_search_run: mode must be one of %s (got %r)" % (sorted(ENSEMBLE_MODES), mode))
    mw = normalise_member_weights(member_weights, M)
    alpha_member = -1 if alpha_member is None else int(alpha_member)
    if not -1 <= alpha_member < M:
        raise ValueError("ensemble_search_run: alpha_member %d is not a member" % alpha_member)
    d = (Dims * M)(*[Dims(*x) for x in dims_list])
    if any(x.V < beam_size for x in d):
        raise ValueError("vocab_size %d is smaller than beam_size %d" % (d[0].V, beam_size))
    if any((x.B, x.P, x.E, x.V) != (d[0].B, d[0].P, d[0].E, d[0].V) for x in d):
        raise ValueError("the members of an ensemble must agree in batch, pixels, encoder_dim and vocab_size")
    require_cuda(enc, *tags_list, *[t for ws_ in weights_list for t in ws_])
    dev = enc.device
    enc = f32c(enc)
    tags_list = [f32c(t) for t in tags_list]
    weights_list = [tuple(None if x is None else f32c(x.detach()) for x in ws_) for ws_ in weights_list]
    w = (Params * M)(*[_params_struct(ws_) for ws_ in weights_list])
    tg = (C.c_void_p * M)(*[t.data_ptr() for t in tags_list])
    cw = (C.c_float * M)(*mw)
    K, N = beam_size, d[0].B
    # with options: the _opt form of the four calls, the options struct after alpha_member; in groups: the _div form
    sfx, opt, noff = _search_form(options, groups, diversity, d[0].V, beam_size, max_steps, int(end), required, d[0].B,
                                  int(start), pad_token)
    ws, off, nwords, t = _run_on_device("scnattn_ensemble_%s" + sfx, (M, d, K, max_steps, alpha_member, *opt), noff,
                                        (w, ptr(enc), tg, int(start)), (w, ptr(enc), cw, mode, int(end)), stream_of(enc),
                                        dev, max_steps, chunk, guard)
    return _beam_results(ws, off, N, K, d[0].P, t, nwords, guard, max_steps, groups=int(groups)), t


# ----------------------------------------------------------------------------------------------
# sampled rollouts (include/scnattn.h: scnattn_rollout_*)
# ----------------------------------------------------------------------------------------------
_ROLLOUT_RESULTS = ("open_rows", "nsrc", "nopen", "length", "sum_logp", "token", "logp", "alpha")
_ROLLOUT_FLOAT = ("sum_logp", "logp", "alpha")


def sample_filter_struct(top_k, top_p, who="rollout_run"):
    """(top_k, top_p) -> scnattn_sample_filter after the header's refusals (ValueError), or None when both limits are at
    their defaults (0 and 1.0): the plain entry points.  top_k >= the vocabulary is off too, but that is the library's to
    see: it launches the plain kernel."""
    import math
    import operator
    try:
        top_k = operator.index(top_k)
    except TypeError:
        raise ValueError("%s: top_k must be an integer >= 0 (0: off; got %r)" % (who, top_k)) from None
    if not 0 <= top_k <= 2 ** 31 - 1:
        raise ValueError("%s: top_k must be an integer >= 0 (0: off; got %r)" % (who, top_k))
    top_p = float(top_p)
    if math.isnan(top_p) or not (0.0 < top_p <= 1.0):
        raise ValueError("%s: top_p must be in (0, 1] (1: off; got %r)" % (who, top_p))
    if C.c_float(top_p).value <= 0.0:
        raise ValueError("%s: top_p %r vanishes in fp32" % (who, top_p))
    if top_k == 0 and top_p == 1.0:
        return None
    return _lib.SampleFilter(top_k=top_k, top_p=top_p)


def rollout_run(dims, K, weights, enc, tags, start, end, seed, draw, inv_temp=1.0, greedy_first=False,
                max_steps=BEAM_MAX_STEPS, want_alpha=False, guard=0, chunk=BEAM_CHUNK, top_k=0, top_p=1.0, force_filtered=False):
    """K captions per image sampled from the decoder on the device (csrc/rollout.hip; the analogue of beam_search_run):
    every step picks one token per open row from softmax(logits * inv_temp) by the Gumbel arg-max, the noise being
    Philox4x32-10 of (seed, draw, row, step, word) -- the same (seed, draw) gives the same captions, another `draw` fresh
    ones.  greedy_first: slot 0 of every image takes the arg-max instead (lowest index among equal logits).
    dims / weights / enc / tags as for beam_search_run.  Returns (results, steps); the results stay ON THE DEVICE (views of
    the workspace), only the open-row counter is downloaded between chunks:
        tokens (R, steps) int32   the picks of row n*K + j, 0 (<pad>) after the row's <end>
        logp (R, steps)           their log-probabilities under the sampled distribution, 0.0 after <end>
        length (R,) int32         number of tokens up to and including <end>; 0 for a row that was CUT OFF: it produced no
                                  <end> within max_steps, and all `steps` picks are its tokens
        sum_logp (R,)             the sum of the row's logp
        alpha (steps, R, P)       only with want_alpha (and attention), else None
        open_rows, nsrc, nopen    the counters (scnattn_rollout_layout)
        nkeep (R, steps) int32    only with a filter: the size of the kept set the token was drawn from, 0 after <end>;
                                  None without
    top_k / top_p: TRUNCATED sampling (include/scnattn.h: scnattn_sample_filter) -- every token is drawn from the top_k most
    likely words and / or the smallest set holding top_p of the mass, both measured on the full softmax, and logp /
    sum_logp are those of the truncated, renormalised distribution.  The noise of a word does not depend on the filter.
    The defaults (0, 1.0) call the plain entry points; force_filtered (tests) calls the _f ones even then.
    guard > 0 (tests): that many sentinel words behind the workspace, returned as results["guard"]."""
    filt = sample_filter_struct(top_k, top_p)
    if filt is None and force_filtered:
        filt = _lib.SampleFilter(top_k=0, top_p=1.0)
    K = int(K)
    if not 1 <= K <= _lib.MAX_BEAM:
        raise ValueError("rollout_run: K must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, K))
    inv_temp = float(inv_temp)
    if not (inv_temp > 0.0 and inv_temp < float("inf")):
        raise ValueError("rollout_run: inv_temp must be positive and finite (got %r)" % inv_temp)
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(draw) < 2 ** 32:
        raise ValueError("rollout_run: seed must fit 64 bits and draw 32 bits, both unsigned")
    d = Dims(*dims)
    if not (0 <= int(start) < d.V and 0 <= int(end) < d.V):
        raise ValueError("rollout_run: start / end token outside the vocabulary")
    require_cuda(enc, tags, *weights)
    dev = enc.device
    enc, tags = f32c(enc), f32c(tags)
    weights = tuple(None if w is None else f32c(w.detach()) for w in weights)
    w = _params_struct(weights)
    N, wa = d.B, int(bool(want_alpha))
    sfx, fl = ("", ()) if filt is None else ("_f", (C.byref(filt),))       # the filter after want_alpha
    ws, off, nwords, t = _run_on_device("scnattn_rollout_%s" + sfx, (C.byref(d), K, max_steps, wa, *fl),
                                        _lib.ROLLOUT_NOFF if filt is None else _lib.ROLLOUT_NOFF_F,
                                        (C.byref(w), ptr(enc), ptr(tags), int(start)),
                                        (C.byref(w), ptr(enc), int(end), inv_temp, int(seed), int(draw),
                                         int(bool(greedy_first))), stream_of(enc), dev, max_steps, chunk, guard)
    wsi = ws.view(torch.int32)
    R = N * K
    sizes = {"open_rows": 1, "nsrc": N, "nopen": N, "length": R, "sum_logp": R, "token": t * R, "logp": t * R,
             "alpha": t * R * d.P}
    out = {}
    for i, name in enumerate(_ROLLOUT_RESULTS):
        if off[i] < 0:
            out[name] = None
            continue
        src = ws if name in _ROLLOUT_FLOAT else wsi
        out[name] = src[off[i]:off[i] + sizes[name]]
    out["tokens"] = out.pop("token").view(t, R).t()
    out["logp"] = out["logp"].view(t, R).t()
    out["nkeep"] = None if filt is None else wsi[off[_lib.ROLLOUT_NOFF]:off[_lib.ROLLOUT_NOFF] + t * R].view(t, R).t()
    if out["alpha"] is not None:
        out["alpha"] = out["alpha"].view(t, R, d.P)
    if guard:
        out["guard"] = wsi[nwords:]
    return out, t


# ----------------------------------------------------------------------------------------------
# scoring given captions (include/scnattn.h: scnattn_rollout_*_sc)
# ----------------------------------------------------------------------------------------------
_SCORE_RESULTS = ("open_rows", "nsrc", "nopen", "ntok", "sum_logp", "token", "logp", "alpha", "rank", "best", "target")
_SCORE_FLOAT = ("sum_logp", "logp", "alpha")


def score_run(dims, K, weights, enc, tags, start, targets, ntok, inv_temp=1.0, max_steps=BEAM_MAX_STEPS, want_alpha=False,
              guard=0, chunk=BEAM_CHUNK):
    """The log-probabilities of GIVEN captions under the decoder, teacher-forced on the device (csrc/rollout.hip:
    rollout_score; the analogue of rollout_run with the pick told its token).  K captions per image, rows n*K + j:
    targets (R, >= max_steps) int32 on the device, row r holding ntok[r] tokens (what follows <start>); ntok (R,) int32 on
    the device, each in [0, max_steps]; 0 marks an empty slot, and an image whose slots are all empty is closed from the
    start.  dims / weights / enc / tags as for beam_search_run.  Returns (results, steps); the results stay ON THE DEVICE
    (views of the workspace); the open-row counter is downloaded between chunks and the longest ntok once at the end, so
    steps is the length of the longest caption:
        logp (R, steps)           log softmax(logits * inv_temp) at the given token, 0.0 at and beyond ntok
        rank (R, steps) int32     the words strictly before the given one in the order (value descending, index ascending)
        best (R, steps) int32     the model's own first word at that position
        tokens (R, steps) int32   the given tokens as recorded, 0 beyond ntok
        sum_logp (R,)             the fp32 sum of the row's logp
        ntok (R,) int32           as given (clamped into [0, max_steps])
        alpha (steps, R, P)       only with want_alpha (and attention), else None: the attention of the given caption
        open_rows, nsrc, nopen    the counters (scnattn_rollout_layout)
    guard > 0 (tests): that many sentinel words behind the workspace, returned as results["guard"]."""
    K = int(K)
    if not 1 <= K <= _lib.MAX_BEAM:
        raise ValueError("score_run: K must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, K))
    inv_temp = float(inv_temp)
    if not (inv_temp > 0.0 and inv_temp < float("inf")):
        raise ValueError("score_run: inv_temp must be positive and finite (got %r)" % inv_temp)
    d = Dims(*dims)
    if not 0 <= int(start) < d.V:
        raise ValueError("score_run: start token outside the vocabulary")
    N = d.B
    R = N * K
    if targets.dtype != torch.int32 or ntok.dtype != torch.int32:
        raise ValueError("score_run: targets and ntok must be int32")
    if targets.dim() != 2 or targets.shape[0] != R or targets.shape[1] < max_steps or ntok.numel() != R:
        raise ValueError("score_run: targets must be (%d, >= %d) and ntok (%d,) (got %s and %s)"
                         % (R, max_steps, R, tuple(targets.shape), tuple(ntok.shape)))
    require_cuda(enc, tags, targets, ntok, *weights)
    dev = enc.device
    enc, tags = f32c(enc), f32c(tags)
    targets, ntok = targets.contiguous(), ntok.contiguous()
    weights = tuple(None if w is None else f32c(w.detach()) for w in weights)
    w = _params_struct(weights)
    wa = int(bool(want_alpha))
    ws, off, nwords, t = _run_on_device("scnattn_rollout_%s_sc", (C.byref(d), K, max_steps, wa), _lib.ROLLOUT_NOFF_SC,
                                        (C.byref(w), ptr(enc), ptr(tags), int(start), ptr(targets), targets.shape[1],
                                         ptr(ntok)),
                                        (C.byref(w), ptr(enc), inv_temp), stream_of(enc), dev, max_steps, chunk, guard)
    wsi = ws.view(torch.int32)
    # the steps of the last chunk beyond the longest caption were no-ops: leave them out (one more 4-byte download)
    t = min(t, int(wsi[off[3]:off[3] + R].max()))
    sizes = {"open_rows": 1, "nsrc": N, "nopen": N, "ntok": R, "sum_logp": R, "alpha": t * R * d.P}
    out = {}
    for i, name in enumerate(_SCORE_RESULTS):
        if off[i] < 0:
            out[name] = None
            continue
        src = ws if name in _SCORE_FLOAT else wsi
        out[name] = src[off[i]:off[i] + sizes.get(name, t * R)]
    out["tokens"] = out.pop("token")
    for name in ("tokens", "logp", "rank", "best", "target"):
        out[name] = out[name].view(t, R).t()
    if out["alpha"] is not None:
        out["alpha"] = out["alpha"].view(t, R, d.P)
    if guard:
        out["guard"] = wsi[nwords:]
    return out, t


# ----------------------------------------------------------------------------------------------
# scheduled sampling (include/scnattn.h: scnattn_rollout_*_ss)
# ----------------------------------------------------------------------------------------------
_MIX_RESULTS = ("open_rows", "nsrc", "nopen", "nmix", "sum_logp", "token", "logp", "alpha", "sample", "replaced", "gold")
_MIX_FLOAT = ("sum_logp", "logp", "alpha")


def mix_prob(prob, who="mix_run"):
    """the replacement probability as the fp32 number the kernel compares with: in [0, 1], NaN refused (ValueError)"""
    import math
    prob = float(prob)
    if math.isnan(prob) or not 0.0 <= prob <= 1.0:
        raise ValueError("%s: prob must be in [0, 1] (got %r)" % (who, prob))
    return C.c_float(prob).value


def mix_run(dims, K, weights, enc, tags, start, gold, nmix, prob, seed, draw, inv_temp=1.0, greedy=False,
            max_steps=BEAM_MAX_STEPS, want_alpha=False, guard=0, chunk=BEAM_CHUNK):
    """SCHEDULED SAMPLING on the device (csrc/rollout.hip: rollout_pick_mixed; the analogue of score_run with a coin): the
    decoder walks the GOLD words of K captions per image, rows n*K + j, and at every step a coin of (seed, draw, row, step)
    replaces the gold word with the model's own sample with probability `prob`; what was chosen is the next step's input.
    gold (R, >= max_steps) int32 on the device, row r holding nmix[r] words (what follows <start>); nmix (R,) int32 on the
    device, each in [0, max_steps]; 0 marks an empty slot.  A sample is rollout_run's pick with its noise (greedy: the
    arg-max in every row); <end> is a word like any other and the gold length alone ends a row.  dims / weights / enc / tags
    as for beam_search_run.  Returns (results, steps); the results stay ON THE DEVICE (views of the workspace); the open-row
    counter is downloaded between chunks and the longest nmix once at the end, so steps is the longest row:
        tokens (R, steps) int32    the word chosen at step t, the input of step t + 1: gold or the sample; 0 beyond nmix
        replaced (R, steps) int32  1 where the sample was taken
        sample (R, steps) int32    the sample where one was taken, else -1 (0 at the steps after the image's last row
                                   closed, which no kernel visits)
        logp (R, steps)            the sample's log-probability under softmax(logits * inv_temp), 0.0 elsewhere
        sum_logp (R,)              the fp32 sum of the row's logp
        gold (R, steps) int32      the gold words as given
        nmix (R,) int32            as given (clamped into [0, max_steps])
        alpha (steps, R, P)        only with want_alpha (and attention), else None: the attention over the mixed inputs
        open_rows, nsrc, nopen     the counters (scnattn_rollout_layout)
    guard > 0 (tests): that many sentinel words behind the workspace, returned as results["guard"]."""
    K = int(K)
    if not 1 <= K <= _lib.MAX_BEAM:
        raise ValueError("mix_run: K must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, K))
    inv_temp = float(inv_temp)
    if not (inv_temp > 0.0 and inv_temp < float("inf")):
        raise ValueError("mix_run: inv_temp must be positive and finite (got %r)" % inv_temp)
    prob = mix_prob(prob)
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(draw) < 2 ** 32:
        raise ValueError("mix_run: seed must fit 64 bits and draw 32 bits, both unsigned")
    d = Dims(*dims)
    if not 0 <= int(start) < d.V:
        raise ValueError("mix_run: start token outside the vocabulary")
    N = d.B
    R = N * K
    if gold.dtype != torch.int32 or nmix.dtype != torch.int32:
        raise ValueError("mix_run: gold and nmix must be int32")
    if gold.dim() != 2 or gold.shape[0] != R or gold.shape[1] < max_steps or nmix.numel() != R:
        raise ValueError("mix_run: gold must be (%d, >= %d) and nmix (%d,) (got %s and %s)"
                         % (R, max_steps, R, tuple(gold.shape), tuple(nmix.shape)))
    require_cuda(enc, tags, gold, nmix, *weights)
    dev = enc.device
    enc, tags = f32c(enc), f32c(tags)
    gold, nmix = gold.contiguous(), nmix.contiguous()
    weights = tuple(None if w is None else f32c(w.detach()) for w in weights)
    w = _params_struct(weights)
    wa = int(bool(want_alpha))
    ws, off, nwords, t = _run_on_device("scnattn_rollout_%s_ss", (C.byref(d), K, max_steps, wa), _lib.ROLLOUT_NOFF_SS,
                                        (C.byref(w), ptr(enc), ptr(tags), int(start), ptr(gold), gold.shape[1], ptr(nmix)),
                                        (C.byref(w), ptr(enc), inv_temp, prob, int(seed), int(draw), int(bool(greedy))),
                                        stream_of(enc), dev, max_steps, chunk, guard)
    wsi = ws.view(torch.int32)
    # the steps of the last chunk beyond the longest row were no-ops: leave them out (one more 4-byte download)
    t = min(t, int(wsi[off[3]:off[3] + R].max()))
    sizes = {"open_rows": 1, "nsrc": N, "nopen": N, "nmix": R, "sum_logp": R, "alpha": t * R * d.P}
    out = {}
    for i, name in enumerate(_MIX_RESULTS):
        if off[i] < 0:
            out[name] = None
            continue
        src = ws if name in _MIX_FLOAT else wsi
        out[name] = src[off[i]:off[i] + sizes.get(name, t * R)]
    out["tokens"] = out.pop("token")
    for name in ("tokens", "logp", "sample", "replaced", "gold"):
        out[name] = out[name].view(t, R).t()
    if out["alpha"] is not None:
        out["alpha"] = out["alpha"].view(t, R, d.P)
    if guard:
        out["guard"] = wsi[nwords:]
    return out, t


# ----------------------------------------------------------------------------------------------
# stand-alone SCN cell (any batch size), split exactly where the reference splits it:
#   scn_input      = SCNCell.forward's x side      (models/scn_cell.py:64-91)
#   scn_recurrent  = SCNCell.recurrent_step        (models/scn_cell.py:112-154)
# Dense contractions run on the MFMA sgemm, the rest on mul_bcast / lstm kernels.
# ----------------------------------------------------------------------------------------------
def _mul(x, q):
    out = torch.empty_like(x)
    call("scnattn_mul_bcast", stream_of(x), 1, x.shape[0], x.shape[1], ptr(x), ptr(q), ptr(out))
    return out


def _off(t, nfloats):
    return C.c_void_p(t.data_ptr() + 4 * nfloats)


class _SCNInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, s, Wa, Wb, Wc, bih):
        require_cuda(u, s, Wa, Wb, Wc, bih)
        u, s = f32c(u), f32c(s)
        Wa, Wb, Wc = (f32c(x.detach()) for x in (Wa, Wb, Wc))
        bih = None if bih is None else f32c(bih.detach())
        B, H, F4 = u.shape[0], Wc.shape[0], Wa.shape[1]
        F = F4 // 4
        pa, qx = gemm(u, Wa), gemm(s, Wb)
        mx = _mul(pa, qx)
        x = torch.empty((4, B, H), device=u.device, dtype=torch.float32)
        for g in range(4):  # x_g = mx_g . Wc_g^T + b_ih_g
            call("scnattn_sgemm", stream_of(u), 0, 1, B, H, F, 1.0, _off(mx, g * F), F4, _off(Wc, g * F), F4, 0.0,
                 _off(x, g * B * H), H, None if bih is None else _off(bih, g * H), None, 1, 0, 0, 0)
        ctx.save_for_backward(u, s, Wa, Wb, Wc, pa, qx, mx)
        ctx.has_bias = bih is not None
        return x[0], x[1], x[2], x[3]

    @staticmethod
    def backward(ctx, *dxs):
        u, s, Wa, Wb, Wc, pa, qx, mx = ctx.saved_tensors
        B, H, F4 = u.shape[0], Wc.shape[0], Wa.shape[1]
        F = F4 // 4
        dev = u.device
        dx = torch.stack([torch.zeros((B, H), device=dev) if d is None else f32c(d) for d in dxs])  # [4,B,H]
        dmx = torch.empty((B, F4), device=dev, dtype=torch.float32)
        gemm(dx, Wc, out=dmx, M=B, N=F, K=H, lda=H, ldb=F4, ldc=F4, batch=4, sa=B * H, sb=F, sc=F)
        dpa, dqx = _mul(dmx, qx), _mul(dmx, pa)
        need = ctx.needs_input_grad
        du = gemm(dpa, Wa, tb=True) if need[0] else None
        ds = gemm(dqx, Wb, tb=True) if need[1] else None
        dWa = gemm(u, dpa, ta=True) if need[2] else None
        dWb = gemm(s, dqx, ta=True) if need[3] else None
        dWc = None
        if need[4]:
            dWc = torch.empty_like(Wc)
            gemm(dx, mx, ta=True, out=dWc, M=H, N=F, K=B, lda=H, ldb=F4, ldc=F4, batch=4, sa=B * H, sb=F, sc=F)
        dbih = None
        if ctx.has_bias and need[5]:
            dbih = torch.empty(4 * H, device=dev, dtype=torch.float32)
            for g in range(4):
                call("scnattn_colsum", stream_of(u), B, H, _off(dx, g * B * H), H, _off(dbih, g * H), 0.0)
        return du, ds, dWa, dWb, dWc, dbih


class _SCNRecurrent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_i, x_f, x_o, x_c, s, h, c, Ha, Hb, Hc, bhh):
        require_cuda(x_i, x_f, x_o, x_c, s, h, c, Ha, Hb, Hc, bhh)
        s, h, c = f32c(s), f32c(h), f32c(c)
        Ha, Hb, Hc = (f32c(x.detach()) for x in (Ha, Hb, Hc))
        bhh = None if bhh is None else f32c(bhh.detach())
        B, H, F4 = h.shape[0], Hc.shape[0], Ha.shape[1]
        F = F4 // 4
        st = stream_of(h)
        r = torch.stack([f32c(x_i), f32c(x_f), f32c(x_o), f32c(x_c)])  # [4,B,H]: r starts as x
        ph, qh = gemm(h, Ha), gemm(s, Hb)
        mh = _mul(ph, qh)
        gemm(mh, Hc, tb=True, out=r, beta=1.0, M=B, N=H, K=F, lda=F4, ldb=F4, ldc=H, batch=4, sa=F, sb=F, sc=B * H)
        gates = torch.empty((B, 4 * H), device=h.device, dtype=torch.float32)
        c_new, h_new, tanhc = torch.empty_like(c), torch.empty_like(c), torch.empty_like(c)
        call("scnattn_lstm_fwd", st, B, H, ptr(r), 1, 0, H, B * H, None, ptr(bhh), ptr(c), ptr(gates), ptr(c_new),
             ptr(h_new), ptr(tanhc))
        ctx.save_for_backward(s, h, c, Ha, Hb, Hc, ph, qh, mh, gates, tanhc)
        ctx.has_bias = bhh is not None
        return h_new, c_new

    @staticmethod
    def backward(ctx, dh, dc_in):
        s, h, c, Ha, Hb, Hc, ph, qh, mh, gates, tanhc = ctx.saved_tensors
        B, H, F4 = h.shape[0], Hc.shape[0], Ha.shape[1]
        F = F4 // 4
        st = stream_of(h)
        dev = h.device
        dh = torch.zeros_like(c) if dh is None else f32c(dh)
        dc = torch.zeros_like(c) if dc_in is None else f32c(dc_in).clone()
        dr = torch.empty((B, 4 * H), device=dev, dtype=torch.float32)
        call("scnattn_lstm_bwd", st, B, B, H, ptr(dh), None, 0, 0, H, ptr(dc), ptr(gates), ptr(c), ptr(tanhc), ptr(dr))
        need = ctx.needs_input_grad
        dxs = [dr[:, g * H:(g + 1) * H].contiguous() if need[g] else None for g in range(4)]
        dmh = torch.empty((B, F4), device=dev, dtype=torch.float32)
        gemm(dr, Hc, out=dmh, M=B, N=F, K=H, lda=4 * H, ldb=F4, ldc=F4, batch=4, sa=H, sb=F, sc=F)
        dph, dqh = _mul(dmh, qh), _mul(dmh, ph)
        ds = gemm(dqh, Hb, tb=True) if need[4] else None
        dhp = gemm(dph, Ha, tb=True) if need[5] else None
        dHa = gemm(h, dph, ta=True) if need[7] else None
        dHb = gemm(s, dqh, ta=True) if need[8] else None
        dHc = None
        if need[9]:
            dHc = torch.empty_like(Hc)
            gemm(dr, mh, ta=True, out=dHc, M=H, N=F, K=B, lda=4 * H, ldb=F4, ldc=F4, batch=4, sa=H, sb=F, sc=F)
        dbhh = colsum(dr) if (ctx.has_bias and need[10]) else None
        return (*dxs, ds, dhp, dc if need[6] else None, dHa, dHb, dHc, dbhh)


def scn_input(u, s, Wa, Wb, Wc, bih):
    return _SCNInput.apply(u, s, Wa, Wb, Wc, bih)


def scn_recurrent(x_i, x_f, x_o, x_c, s, h, c, Ha, Hb, Hc, bhh):
    return _SCNRecurrent.apply(x_i, x_f, x_o, x_c, s, h, c, Ha, Hb, Hc, bhh)


# ----------------------------------------------------------------------------------------------
# stand-alone soft attention
# ----------------------------------------------------------------------------------------------
class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, h, We, be, Wd, bd, wf, b0):
        require_cuda(enc, h, We, be, Wd, bd, wf, b0)
        enc, h = f32c(enc), f32c(h)
        We, be, Wd, bd, wf, b0 = (f32c(x.detach()) for x in (We, be, Wd, bd, wf, b0))
        B, P, E = enc.shape
        A = We.shape[0]
        st = stream_of(enc)
        dev = enc.device
        att1 = gemm(enc.view(B * P, E), We, tb=True, bias=be)
        att2 = gemm(h, Wd, tb=True, bias=bd)
        e = torch.empty((B, P), device=dev, dtype=torch.float32)
        call("scnattn_attn_scores", st, B, P, A, ptr(att1), ptr(att2), 1, 0, A, None, ptr(wf), ptr(b0), ptr(e), None)
        alpha = torch.empty((B, P), device=dev, dtype=torch.float32)
        awe = torch.empty((B, E), device=dev, dtype=torch.float32)
        call("scnattn_attn_context", st, B, P, E, ptr(enc), ptr(e), None, 0, 0, 0, None, ptr(alpha), P, None,
             ptr(awe), None, None)
        ctx.save_for_backward(enc, h, We, Wd, wf, att1, att2, alpha)
        return awe, alpha

    @staticmethod
    def backward(ctx, dawe, dalpha_in):
        enc, h, We, Wd, wf, att1, att2, alpha = ctx.saved_tensors
        B, P, E = enc.shape
        A = We.shape[0]
        st = stream_of(enc)
        dev = enc.device
        dawe = torch.zeros((B, E), device=dev) if dawe is None else f32c(dawe)
        dalpha_in = None if dalpha_in is None else f32c(dalpha_in)
        dalpha = torch.empty((B, P), device=dev, dtype=torch.float32)
        call("scnattn_attn_dalpha", st, B, P, E, ptr(enc), ptr(dawe), ptr(dalpha_in), P, ptr(dalpha))
        de = torch.empty((B, P), device=dev, dtype=torch.float32)
        datt2 = torch.empty((B, A), device=dev, dtype=torch.float32)
        call("scnattn_attn_softmax_bwd", st, B, P, A, ptr(att1), ptr(att2), ptr(wf), ptr(alpha), ptr(dalpha), ptr(de),
             ptr(datt2), A)
        nblk = _lib.lib().scnattn_attn_datt1_post_blocks(B, P)
        datt1 = torch.empty((B * P, A), device=dev, dtype=torch.float32)
        dwpart = torch.empty((nblk, A + 1), device=dev, dtype=torch.float32)
        ones = torch.ones(B, device=dev, dtype=torch.int32)
        call("scnattn_attn_datt1_post", st, B, P, A, 1, ptr(ones), ptr(att1), ptr(att2), ptr(de), ptr(wf), ptr(datt1),
             ptr(dwpart))
        dwb = colsum(dwpart)
        need = ctx.needs_input_grad
        denc = None
        if need[0]:
            denc = gemm(datt1, We).view(B, P, E)
            # denc[b] += alpha_b (P x 1) . dawe_b (1 x E)
            gemm(alpha, dawe, ta=True, out=denc, beta=1.0, M=P, N=E, K=1, lda=B * P, ldb=B * E, ldc=E, batch=B,
                 sa=P, sb=E, sc=P * E)
        dh = gemm(datt2, Wd) if need[1] else None
        dWe = gemm(datt1, enc.view(B * P, E), ta=True) if need[2] else None
        dbe = colsum(datt1) if need[3] else None
        dWd = gemm(datt2, h, ta=True) if need[4] else None
        dbd = colsum(datt2) if need[5] else None
        dwf = dwb[:A].reshape(1, A).clone() if need[6] else None
        db0 = dwb[A:A + 1].clone() if need[7] else None
        return denc, dh, dWe, dbe, dWd, dbd, dwf, db0


def attention(enc, h, We, be, Wd, bd, wf, b0):
    return _Attention.apply(enc, h, We, be, Wd, bd, wf, b0)


# ----------------------------------------------------------------------------------------------
# nn.Linear on the MFMA sgemm (init_h / init_c / f_beta / fc outside the fused sequence path)
# ----------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b):
        require_cuda(x, W, b)
        x2 = f32c(x).reshape(-1, x.shape[-1])
        W = f32c(W.detach())
        y = gemm(x2, W, tb=True, bias=None if b is None else f32c(b.detach()))
        ctx.save_for_backward(x2, W)
        ctx.xshape = x.shape
        ctx.has_bias = b is not None
        return y.view(*x.shape[:-1], W.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, W = ctx.saved_tensors
        dy2 = f32c(dy).reshape(-1, W.shape[0])
        need = ctx.needs_input_grad
        dx = gemm(dy2, W).view(ctx.xshape) if need[0] else None
        dW = gemm(dy2, x2, ta=True) if need[1] else None
        db = colsum(dy2) if (ctx.has_bias and need[2]) else None
        return dx, dW, db


def linear(x, W, b=None):
    return _Linear.apply(x, W, b)


# ----------------------------------------------------------------------------------------------
# encoder tail: AdaptiveAvgPool2d + permute(0,2,3,1), fused, any input memory format
# ----------------------------------------------------------------------------------------------
class _PoolPermute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, out_size):
        require_cuda(x)
        ctx.in_dtype = x.dtype
        if x.dtype != torch.float32:     # bf16 trunk: the decoder side is fp32
            x = x.float()
        B, Cn, Hin, Win = x.shape
        y = torch.empty((B, out_size, out_size, Cn), device=x.device, dtype=torch.float32)
        sb, scs, sh, sw = x.stride()
        call("scnattn_pool_permute_fwd", stream_of(x), B, Cn, Hin, Win, out_size, out_size, ptr(x), sb, scs, sh, sw, ptr(y))
        ctx.shape = (B, Cn, Hin, Win, out_size)
        ctx.channels_last = x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()
        return y

    @staticmethod
    def backward(ctx, dy):
        B, Cn, Hin, Win, out_size = ctx.shape
        dy = f32c(dy)
        dx = torch.empty((B, Cn, Hin, Win), device=dy.device, dtype=torch.float32,
                         memory_format=torch.channels_last if ctx.channels_last else torch.contiguous_format)
        sb, scs, sh, sw = dx.stride()
        call("scnattn_pool_permute_bwd", stream_of(dy), B, Cn, Hin, Win, out_size, out_size, ptr(dy), ptr(dx), sb, scs, sh, sw)
        return (dx if ctx.in_dtype == torch.float32 else dx.to(ctx.in_dtype)), None


def pool_permute(x, out_size):
    return _PoolPermute.apply(x, out_size)


# ----------------------------------------------------------------------------------------------
# tagger head: global average pool (+ dropout mask) -> Linear -> Sigmoid -> BCELoss + binary accuracy  (csrc/taghead.hip);
# TagLoss: positive weights, focal and asymmetric terms on the logits in the place of BCELoss
# ----------------------------------------------------------------------------------------------
def _pixel_strides(x4):
    """(sb, sp, sc) of a (B, C, H, W) map read as x[b, q, c], q = h * W + w; None when the pixels have no common stride."""
    _, _, H, Wd = x4.shape
    sb, sc, sh, sw = x4.stride()
    if H == 1:
        return sb, sw, sc
    if Wd == 1 or sh == Wd * sw:
        return sb, (sh if Wd == 1 else sw), sc
    return None


class TagLoss:
    """A tagger loss for rare tags (include/scnattn.h: "Tagger losses for rare tags"): per element of the logits
        t w_s (1 - p)^gamma_pos (-log p) + (1 - t) p_m^gamma_neg (-log(1 - p_m)),   p_m = max(p - margin, 0),
    averaged over B * S like nn.BCELoss.  `pos_weight`: float32 tensor [S] of weights >= 0 on the device, or None (all 1).
    Immutable; the constructor refuses what the library refuses (ValueError).  TagLoss() is the identity: tag_head_loss then
    runs the reference's BCELoss path."""
    __slots__ = ("pos_weight", "gamma_pos", "gamma_neg", "margin")

    def __init__(self, pos_weight=None, gamma_pos=0.0, gamma_neg=0.0, margin=0.0):
        gp, gn, m = float(gamma_pos), float(gamma_neg), float(margin)
        if not (0.0 <= gp <= 16.0 and 0.0 <= gn <= 16.0):        # false for a NaN
            raise ValueError("TagLoss: gamma_pos and gamma_neg must be finite and in [0, 16] (got %r, %r)" % (gamma_pos, gamma_neg))
        if not 0.0 <= m < 1.0:
            raise ValueError("TagLoss: margin must be in [0, 1) (got %r)" % (margin,))
        if m > 0.0 and 0.0 < gn < 1.0:
            raise ValueError("TagLoss: a margin with 0 < gamma_neg < 1 has an unbounded gradient at p -> margin")
        if pos_weight is not None:
            if not torch.is_tensor(pos_weight) or pos_weight.dtype != torch.float32 or pos_weight.dim() != 1:
                raise ValueError("TagLoss: pos_weight must be a float32 tensor [S]")
            pos_weight = pos_weight.detach().contiguous()
            if not bool((pos_weight >= 0).all()) or not bool(torch.isfinite(pos_weight).all()):
                raise ValueError("TagLoss: pos_weight must be finite and >= 0")
        for k, v in zip(self.__slots__, (pos_weight, gp, gn, m)):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError("TagLoss is immutable")

    def __repr__(self):
        return "TagLoss(pos_weight=%s, gamma_pos=%g, gamma_neg=%g, margin=%g)" % (
            "None" if self.pos_weight is None else "[%d]" % self.pos_weight.numel(), self.gamma_pos, self.gamma_neg, self.margin)

    @property
    def is_identity(self):
        return self.pos_weight is None and self.gamma_pos == 0.0 and self.gamma_neg == 0.0 and self.margin == 0.0

    def struct(self):
        return _lib.TagLossOpts(self.gamma_pos, self.gamma_neg, self.margin)

    @classmethod
    def asl(cls, gamma_neg=4.0, gamma_pos=0.0, margin=0.05):
        """the asymmetric loss (Ridnik et al. 2021) with its published defaults"""
        return cls(None, gamma_pos, gamma_neg, margin)

    @classmethod
    def focal(cls, gamma=2.0, pos_weight=None):
        """the focal loss (Lin et al. 2017); its alpha balance is carried by pos_weight"""
        return cls(pos_weight, gamma, gamma, 0.0)

    @classmethod
    def balanced(cls, targets, power=0.5, cap=100.0, **kw):
        """w_s = clamp(((N - n_s) / max(n_s, 1))^power, 1, cap) from the positives n_s = #(t >= 0.5) of the [N, S] target
        matrix `targets`; **kw: gamma_pos, gamma_neg, margin.  Plain torch: it runs once per training run."""
        n = (targets >= 0.5).sum(dim=0).double()
        w = ((targets.shape[0] - n) / n.clamp_min(1.0)).pow(power).clamp(1.0, cap)
        return cls(w.float(), **kw)


def prior_bias(targets, smooth=1.0):
    """log((n_s + smooth) / (N - n_s + smooth)) [S] from the positives n_s = #(t >= 0.5) of the [N, S] matrix `targets`: the
    RetinaNet initialisation of the head's bias (sigmoid(bias) = the tag's prior), which keeps the first steps of a focal run
    from being swamped by the negatives"""
    n = (targets >= 0.5).sum(dim=0).double()
    return torch.log((n + smooth) / (targets.shape[0] - n + smooth)).float()


class _TagHeadLoss(torch.autograd.Function):
    """probs = sigmoid(linear(mean_pixels(x4) * ks)), loss = BCELoss()(probs, targets), agree = #((probs >= .5) == (targets >= .5)).
    The two reductions and the element-wise chain are the kernels of csrc/taghead.hip, the three products stay on the GEMM.
    `loss`: None or an identity TagLoss for that path; any other TagLoss puts scnattn_tagloss_fwd / _bwd in the place of the
    BCE pair and keeps the logits instead of the probabilities for the backward pass."""

    @staticmethod
    def forward(ctx, x4, ks, W, b, targets, pooled_bf16=False, loss=None):
        if loss is not None and loss.is_identity:
            loss = None
        require_cuda(x4, ks, W, b, targets, None if loss is None else loss.pos_weight)
        if x4.dtype not in (torch.float32, torch.bfloat16):
            x4 = x4.float()
        if _pixel_strides(x4) is None:
            x4 = x4.contiguous(memory_format=torch.channels_last)
        Bn, Cn, H, Wd = x4.shape
        S = W.shape[0]
        bf16 = 1 if x4.dtype == torch.bfloat16 else 0
        ks, targets = f32c(ks), f32c(targets)
        W = f32c(W.detach())
        b = None if b is None else f32c(b.detach())
        dev, st = x4.device, stream_of(x4)
        f32 = dict(device=dev, dtype=torch.float32)
        xd = torch.empty((Bn, Cn), **f32)
        sb, sp, sc = _pixel_strides(x4)
        call("scnattn_tag_pool_fwd", st, Bn, H * Wd, Cn, ptr(x4), 2 if (bf16 and pooled_bf16) else bf16, sb, sp, sc, ptr(ks), Cn,
             ptr(xd), Cn)
        z = gemm(xd, W, tb=True, bias=b)
        probs = torch.empty((Bn, S), **f32)
        rows = torch.empty(2 * Bn, **f32)
        out = torch.empty(2, **f32)
        if loss is None:
            call("scnattn_bce_fwd", st, Bn, S, ptr(z), S, ptr(targets), S, ptr(probs), S, ptr(rows), ptr(out))
            ctx.save_for_backward(xd, ks, W, probs, targets)
        else:
            if loss.pos_weight is not None and loss.pos_weight.numel() != S:
                raise ValueError("tag_head_loss: pos_weight has %d weights for %d tags" % (loss.pos_weight.numel(), S))
            call("scnattn_tagloss_fwd", st, Bn, S, ptr(z), S, ptr(targets), S, ptr(loss.pos_weight), C.byref(loss.struct()),
                 ptr(probs), S, ptr(rows), ptr(out))
            ctx.save_for_backward(xd, ks, W, z, targets)
        ctx.loss = loss
        ctx.map = (x4.dtype, H, Wd)
        ctx.has_bias = b is not None
        loss, agree = out[0], out[1]
        ctx.mark_non_differentiable(probs, agree)
        ctx.set_materialize_grads(False)      # no zero-filled (B, S) gradient for probs
        return probs, loss, agree

    @staticmethod
    def backward(ctx, _dprobs, dloss, _dagree):
        if dloss is None:
            return None, None, None, None, None, None, None
        xd, ks, W, probs, targets = ctx.saved_tensors          # `probs` holds the logits under a TagLoss
        dtype, H, Wd = ctx.map
        Bn, Cn = xd.shape
        S = W.shape[0]
        need = ctx.needs_input_grad          # (x4, ks, W, b, targets)
        st = stream_of(xd)
        dz = torch.empty((Bn, S), device=xd.device, dtype=torch.float32)
        if ctx.loss is None:
            call("scnattn_bce_bwd", st, Bn, S, ptr(probs), S, ptr(targets), S, ptr(f32c(dloss).reshape(1)), ptr(dz), S)
        else:
            call("scnattn_tagloss_bwd", st, Bn, S, ptr(probs), S, ptr(targets), S, ptr(ctx.loss.pos_weight),
                 C.byref(ctx.loss.struct()), ptr(f32c(dloss).reshape(1)), ptr(dz), S)
        dW = gemm(dz, xd, ta=True) if need[2] else None
        db = colsum(dz) if (ctx.has_bias and need[3]) else None
        dx = None
        if need[0]:
            dxd = gemm(dz, W)
            # channels-last in the map's dtype: what the last Bottleneck's backward reads in place (scnattn/conv.py, conv16.py)
            dx = torch.empty((Bn, Cn, H, Wd), device=xd.device, dtype=dtype, memory_format=torch.channels_last)
            sb, sp, sc = _pixel_strides(dx)
            call("scnattn_tag_pool_bwd", st, Bn, H * Wd, Cn, ptr(dxd), Cn, ptr(ks), Cn, ptr(dx),
                 1 if dtype == torch.bfloat16 else 0, sb, sp, sc)
        return dx, None, dW, db, None, None, None


def tag_head_loss(x4, ks, W, b, targets, pooled_bf16=False, loss=None):
    """The tagger's head and loss on the (B, C, H, W) trunk map `x4` (fp32 or bf16, any strides): returns (probs (B, S),
    loss, agree), loss and agree 0-d device tensors.  `ks`: pre-scaled dropout keep mask (B, C) or None.  Gradients flow
    from `loss` to x4 (its own dtype, channels-last), W and b; probs and agree carry none.  `pooled_bf16` (bf16 maps only): round
    the pooled mean to bf16 as nn.AdaptiveAvgPool2d does on a bf16 map, i.e. compute what EncoderTagger.forward computes under
    bf16 autocast; off, the mean keeps its fp32 accumulation.  `loss`: a TagLoss (weighted, focal or asymmetric terms on the
    logits); None or the identity TagLoss() is the reference's BCELoss, bit for bit the path without the argument.  probs and
    agree do not depend on it."""
    if loss is not None and not isinstance(loss, TagLoss):
        raise TypeError("tag_head_loss: loss must be a TagLoss or None")
    return _TagHeadLoss.apply(x4, ks, W, b, targets, pooled_bf16, loss)


# ----------------------------------------------------------------------------------------------
# fused BatchNorm2d (+ residual) (+ ReLU), channels-last  (csrc/batchnorm.hip)
# ----------------------------------------------------------------------------------------------
BN_MASK_FROM_Z = True    # bn -> relu groups without residual: recompute the ReLU mask from z in the backward pass
_bn_ws = {}
_bn_fn = None


def _bn_workspace(dev, C):
    # stream-ordered reuse: one buffer per (device, stream) -- two trunks may run on two streams at once (the frozen
    # tagger beside the caption encoder, trains/harness.py)
    key = (dev, torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device()))
    ws = _bn_ws.get(key)
    if ws is None or ws.numel() < 512 * C:
        need = max(_lib.lib().scnattn_bn_workspace_floats(C), 1 << 20)
        ws = torch.empty(need, device=dev, dtype=torch.float32)
        _bn_ws[key] = ws
    return ws


def _bn_fns():
    """Pre-bound ctypes entry points: the BN group runs ~300 times per train step, so the Python cost per
    call matters (the GPU kernels take 5-20 us each)."""
    global _bn_fn
    if _bn_fn is None:
        h = _lib.lib()
        _bn_fn = (h.scnattn_bn_stats, h.scnattn_bn_apply, h.scnattn_bn_bwd, torch._C._cuda_getCurrentRawStream)
    return _bn_fn


class _BNAct(torch.autograd.Function):
    """Feature maps may be fp32 or bf16 (trunk under bf16 autocast); parameters/statistics are fp32."""

    @staticmethod
    def forward(ctx, z, res, gamma, beta, run_mean, run_var, training, momentum, eps, relu):
        if not z.is_cuda:
            raise RuntimeError("scnattn: fused BatchNorm needs tensors on an MI355X device; there is no CPU fallback")
        if z.dtype not in (torch.float32, torch.bfloat16):
            z = z.float()
        bf16 = 1 if z.dtype == torch.bfloat16 else 0
        if not z.is_contiguous(memory_format=torch.channels_last):
            z = z.contiguous(memory_format=torch.channels_last)
        if res is not None and (res.dtype != z.dtype or not res.is_contiguous(memory_format=torch.channels_last)):
            res = res.to(z.dtype).contiguous(memory_format=torch.channels_last)
        N, Cn, H, W = z.shape
        R = N * H * W
        f_stats, f_apply, _, raw_stream = _bn_fns()
        st = raw_stream(z.device.index)
        if training:
            stats = torch.empty((2, Cn), device=z.device, dtype=torch.float32)
            mean, invstd = stats[0], stats[1]
            rc = f_stats(st, R, Cn, z.data_ptr(), bf16, eps, momentum, _bn_workspace(z.device, Cn).data_ptr(),
                         mean.data_ptr(), invstd.data_ptr(), run_mean.data_ptr(), run_var.data_ptr())
            if rc:
                _lib.check(rc, "scnattn_bn_stats")
        else:
            mean, invstd = run_mean.float(), torch.rsqrt(run_var.float() + eps)
        y = torch.empty_like(z)   # preserves the channels-last strides
        rc = f_apply(st, R, Cn, z.data_ptr(), None if res is None else res.data_ptr(), bf16, mean.data_ptr(),
                     invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), int(relu), y.data_ptr())
        if rc:
            _lib.check(rc, "scnattn_bn_apply")
        # bn -> relu without a residual in between (bn1/bn2 of a bottleneck), fp32: the backward pass recomputes the
        # ReLU mask from z and never reads y
        mask_from_z = BN_MASK_FROM_Z and bool(relu) and res is None and not bf16
        ctx.save_for_backward(z, y if (relu and not mask_from_z) else None, mean, invstd, gamma,
                              beta if mask_from_z else None)
        ctx.cfg = (bool(training), bool(relu), res is not None, bf16)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, y, mean, invstd, gamma, beta = ctx.saved_tensors
        training, relu, has_res, bf16 = ctx.cfg
        N, Cn, H, W = z.shape
        R = N * H * W
        if dy.dtype != z.dtype or not dy.is_contiguous(memory_format=torch.channels_last):
            dy = dy.to(z.dtype).contiguous(memory_format=torch.channels_last)
        need = ctx.needs_input_grad
        dz = torch.empty_like(z) if need[0] else None
        dres = torch.empty_like(z) if (has_res and need[1]) else None
        dgb = torch.empty((2, Cn), device=z.device, dtype=torch.float32)
        _, _, f_bwd, raw_stream = _bn_fns()
        rc = f_bwd(raw_stream(z.device.index), R, Cn, dy.data_ptr(), None if y is None else y.data_ptr(), z.data_ptr(),
                   bf16, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), None if beta is None else beta.data_ptr(),
                   int(relu), int(training),
                   _bn_workspace(z.device, Cn).data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(),
                   None if dz is None else dz.data_ptr(), None if dres is None else dres.data_ptr())
        if rc:
            _lib.check(rc, "scnattn_bn_bwd")
        return (dz, dres, dgb[1] if need[2] else None, dgb[0] if need[3] else None, None, None, None, None, None, None)


def bn_act(z, res, gamma, beta, run_mean, run_var, training, momentum, eps, relu):
    return _BNAct.apply(z, res, gamma, beta, run_mean, run_var, training, momentum, eps, relu)


# ----------------------------------------------------------------------------------------------
# The train step's loss (trains/attention_scn.py:222-236) on the unpacked (B, T, V) scores
# ----------------------------------------------------------------------------------------------
def _caption_loss_fwd(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, k=0, row_weight=None):
    """The forward launches of csrc/loss.hip; k >= 1: the metrics form, which also returns (hits, preds); row_weight: the
    reward-weighted form."""
    require_cuda(scores, alphas, caps_sorted, dl_dev, row_weight)
    scores = f32c(scores)
    alphas = None if alphas is None else f32c(alphas)
    B, T, V = scores.shape
    P = alphas.shape[2] if alphas is not None else 0
    if caps_sorted.dtype != torch.int64 or caps_sorted.dim() != 2 or caps_sorted.stride(1) != 1 \
            or caps_sorted.shape[0] != B or caps_sorted.shape[1] < T + 1:
        raise RuntimeError("caption_loss: caps_sorted must be int64 (B, >= T+1) with unit column stride")
    if dl_dev.dtype != torch.int32 or dl_dev.numel() != B or not dl_dev.is_contiguous():
        raise RuntimeError("caption_loss: decode lengths must be a contiguous int32 vector of B entries")
    if alphas is not None and tuple(alphas.shape[:2]) != (B, T):
        raise RuntimeError("caption_loss: alphas must be (B, T, P)")
    dev = scores.device
    ws = torch.empty(2 * B * T + B * P + B + 1, device=dev, dtype=torch.float32)
    row_lse, row_loss = ws[:B * T], ws[B * T:2 * B * T]
    sm1, reg_part = ws[2 * B * T:2 * B * T + B * P], ws[2 * B * T + B * P:2 * B * T + B * P + B]
    loss = ws[-1:]
    tgt = C.c_void_p(caps_sorted.data_ptr() + 8)            # targets = caps_sorted[:, 1:]
    args = (stream_of(scores), B, T, V, P, ptr(scores), tgt, caps_sorted.stride(0),
            ptr(dl_dev), int(n_tokens), ptr(alphas), float(alpha_c), ptr(row_lse), ptr(row_loss),
            ptr(sm1) if P else None, ptr(reg_part) if P else None, ptr(loss))
    ctx.save_for_backward(scores, caps_sorted, dl_dev, ws, row_weight)
    ctx.meta = (B, T, V, P, int(n_tokens), float(alpha_c), alphas is not None)
    if row_weight is not None:
        call("scnattn_caption_loss_weighted_fwd", *args[:10], ptr(row_weight), *args[10:])
        return loss.reshape(())
    if not k:
        call("scnattn_caption_loss_fwd", *args)
        return loss.reshape(())
    iws = torch.empty(2 * B * T + 2, device=dev, dtype=torch.int32)     # row_rank [B*T], preds [B][T], hits [2]
    preds, hits = iws[B * T:2 * B * T].view(B, T), iws[2 * B * T:]
    call("scnattn_caption_loss_metrics_fwd", *args, int(k), ptr(iws), ptr(preds), T, ptr(hits))
    return loss.reshape(()), hits, preds


def _caption_loss_bwd(ctx, g):
    """(d scores, d alphas) through scnattn_caption_loss_bwd: the workspaces of either forward form"""
    scores, caps_sorted, dl_dev, ws, row_weight = ctx.saved_tensors
    B, T, V, P, n_tokens, alpha_c, has_alpha = ctx.meta
    g = f32c(g).reshape(1)
    dscores = torch.empty_like(scores) if ctx.needs_input_grad[0] else None
    dalphas = torch.empty((B, T, P), device=scores.device, dtype=torch.float32) \
        if (has_alpha and ctx.needs_input_grad[1]) else None
    if dscores is None:                                       # the kernel pair always produces d scores
        dscores = torch.empty_like(scores)
    row_lse = ws[:B * T]
    sm1 = ws[2 * B * T:2 * B * T + B * P]
    head = (stream_of(scores), B, T, V, P, ptr(scores), C.c_void_p(caps_sorted.data_ptr() + 8), caps_sorted.stride(0),
            ptr(dl_dev), n_tokens)
    tail = (ptr(row_lse), ptr(sm1) if dalphas is not None else None, alpha_c, ptr(g), ptr(dscores), ptr(dalphas))
    if row_weight is not None:
        call("scnattn_caption_loss_weighted_bwd", *head, ptr(row_weight), *tail)
    else:
        call("scnattn_caption_loss_bwd", *head, *tail)
    return (dscores if ctx.needs_input_grad[0] else None), dalphas


class _CaptionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c):
        return _caption_loss_fwd(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c)

    @staticmethod
    def backward(ctx, g):
        return _caption_loss_bwd(ctx, g) + (None, None, None, None)


class _CaptionLossMetrics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, k):
        loss, hits, preds = _caption_loss_fwd(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, k)
        ctx.mark_non_differentiable(hits, preds)
        return loss, hits, preds

    @staticmethod
    def backward(ctx, g, _ghits, _gpreds):
        return _caption_loss_bwd(ctx, g) + (None, None, None, None, None)


class _CaptionLossWeighted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, row_weight):
        return _caption_loss_fwd(ctx, scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, row_weight=row_weight)

    @staticmethod
    def backward(ctx, g):
        return _caption_loss_bwd(ctx, g) + (None, None, None, None, None)


def _loss_lengths(scores, decode_lengths, dl_dev):
    T = scores.shape[1]
    n_tokens = sum(min(int(l), T) for l in decode_lengths)
    if dl_dev is None:
        dl_dev = torch.tensor(list(decode_lengths), dtype=torch.int32, device=scores.device)
    return n_tokens, dl_dev


def caption_loss(scores, caps_sorted, decode_lengths, alphas=None, alpha_c=1.0, dl_dev=None):
    """`CrossEntropyLoss()(pack(scores), pack(caps_sorted[:, 1:])) + alpha_c * ((1 - alphas.sum(1))**2).mean()`
    of trains/attention_scn.py:222-236 without building the packed batch.  scores (B, T, V) and alphas
    (B, T, P) as the decoder returns them, decode_lengths the decoder's list; dl_dev optionally the same
    lengths as an int32 device vector (saves one small host-to-device copy)."""
    n_tokens, dl_dev = _loss_lengths(scores, decode_lengths, dl_dev)
    return _CaptionLoss.apply(scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c)


def caption_loss_weighted(scores, caps_sorted, decode_lengths, row_weight, alphas=None, alpha_c=0.0, dl_dev=None):
    """The reward-weighted loss of self-critical training:
        (1 / n_tokens) * sum_b row_weight[b] * sum_{t < decode_lengths[b]} (logsumexp(scores[b, t]) - scores[b, t, target])
        + alpha_c * ((1 - alphas.sum(1))**2).mean()                      (the regulariser is not weighted)
    row_weight (B,) on the device, fp32: the advantage of each caption, a constant -- it gets no gradient.  The same kernels
    as caption_loss with one product per row, so weights of 1.0 give caption_loss's bits, forward and backward."""
    B = scores.shape[0]
    if row_weight.dim() != 1 or row_weight.numel() != B:
        raise RuntimeError("caption_loss_weighted: row_weight must be a vector of B = %d entries (got %s)"
                           % (B, tuple(row_weight.shape)))
    if row_weight.requires_grad:
        raise RuntimeError("caption_loss_weighted: row_weight is a constant and must not require grad")
    n_tokens, dl_dev = _loss_lengths(scores, decode_lengths, dl_dev)
    return _CaptionLossWeighted.apply(scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, f32c(row_weight))


def caption_loss_metrics(scores, caps_sorted, decode_lengths, alphas=None, alpha_c=1.0, dl_dev=None, k=5):
    """caption_loss with the caption loops' metrics from the same pass over the scores: returns (loss, hits, preds).
    `loss` holds the bits caption_loss gives and differentiates through the same backward entry.  `hits` int32 (2,):
    the number of decoded rows whose target is among the top k, and among the top 1, of its row, elements ordered by
    (value descending, index ascending) -- `accuracy(pack(scores), pack(targets), k)` of utils/metric.py is
    `hits[0].item() * (100.0 / sum(decode_lengths))`.  `preds` int32 (B, T): the arg-max token of every decoded position
    (`torch.max(scores, dim=2)[1]`, the lowest index among equal maxima), 0 where nothing was decoded.  Both stay on
    the device and carry no gradient."""
    if int(k) < 1:
        raise RuntimeError("caption_loss_metrics: k must be >= 1")
    n_tokens, dl_dev = _loss_lengths(scores, decode_lengths, dl_dev)
    return _CaptionLossMetrics.apply(scores, alphas, caps_sorted, dl_dev, n_tokens, alpha_c, int(k))


# ----------------------------------------------------------------------------------------------
def clamp_adam_(p, g, m, v, lr, step, clip, beta1=0.9, beta2=0.999, eps=1e-8, gscale=1.0):
    """Fused clamp(+-clip) + Adam on flat fp32 buffers (utils/optimizer.py:1-11 + torch.optim.Adam)."""
    require_cuda(p, g, m, v)
    call("scnattn_clamp_adam", stream_of(p), p.numel(), ptr(p), ptr(g), ptr(m), ptr(v), lr, beta1, beta2, eps,
         int(step), float(clip if clip is not None else 0.0), gscale)
