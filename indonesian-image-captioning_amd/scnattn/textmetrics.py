"""Caption evaluation on the device: BLEU-1..4, ROUGE-L and CIDEr-D over token ids (csrc/textmetrics.hip through the C ABI).

What the reference's eval_caption.py:135-165 hands to NLGEval after the beam search -- hypotheses and the references of every
test image, special tokens stripped -- scored without leaving the GPU: the sequences are padded int32 tensors, the special
tokens are dropped inside the kernels (a skip list per side), and one call of ``CaptionScorer.score`` downloads a few dozen
numbers.  METEOR (Java + WordNet) is not computed.  Agreement with NLGEval / pycocoevalcap themselves is unconfirmed (neither
is installed here); the definitions are those of include/scnattn.h and DESIGN 5k, and BLEU is pinned to NLTK by
tests/golden/bleu_nltk_1to4.json.

There is no CPU fallback: tensors must live on an MI355X device."""
import ctypes as C
import math

import torch

from utils.metric import bleu_from_totals
from . import _lib

MAX_LEN = _lib.TEXT_MAX_LEN
MAX_REFS = _lib.TEXT_MAX_REFS
CIDER_MAX_TOKEN = _lib.TEXT_CIDER_MAX_TOKEN


def _width(longest):
    if longest > MAX_LEN:
        raise ValueError("scnattn.textmetrics: a sequence of %d tokens exceeds the limit of %d" % (longest, MAX_LEN))
    return max(1, longest)


def pack_captions(seqs, device="cuda"):
    """Hypotheses -> (tokens int32 [N, L], lengths int32 [N]) on the device, one upload.
    `seqs`: a list of token-id lists (ragged), or an integer tensor [N, L] whose rows count in full (what is padding there is
    named in the scorer's skip list).  A tensor already on the device is converted in place, nothing is uploaded."""
    if torch.is_tensor(seqs):
        if seqs.dim() != 2:
            raise ValueError("pack_captions: a tensor of hypotheses is [N, L]")
        N, L = seqs.shape
        _width(L)
        tok = seqs.to(device=device, dtype=torch.int32)
        if L == 0:
            tok = torch.zeros(N, 1, dtype=torch.int32, device=device)
        return tok.contiguous(), torch.full((N,), L, dtype=torch.int32, device=device)
    seqs = [list(s) for s in seqs]
    N = len(seqs)
    L = _width(max((len(s) for s in seqs), default=0))
    flat = [x for s in seqs for x in s + [0] * (L - len(s))]
    host = torch.tensor(flat + [len(s) for s in seqs], dtype=torch.int32)      # tokens, then lengths: one buffer, one upload
    dev = host.to(device)
    return dev[:N * L].view(N, L), dev[N * L:]


def pack_references(refs, device="cuda"):
    """References -> (tokens int32 [N, R, L], lengths int32 [N, R]) on the device, one upload; an image with fewer than R
    references leaves its last slots absent (length -1), and so does a reference given as None, wherever it stands.
    `refs`: a list (images) of lists (references) of token-id lists, or an integer tensor [N, R, L] whose rows count in full."""
    if torch.is_tensor(refs):
        if refs.dim() != 3:
            raise ValueError("pack_references: a tensor of references is [N, R, L]")
        N, R, L = refs.shape
        _width(L)
        if L == 0:
            raise ValueError("pack_references: references of width 0")
        return (refs.to(device=device, dtype=torch.int32).contiguous(),
                torch.full((N, R), L, dtype=torch.int32, device=device))
    refs = [[None if r is None else list(r) for r in per] for per in refs]
    N = len(refs)
    R = max(1, max((len(per) for per in refs), default=1))
    L = _width(max((len(r) for per in refs for r in per if r is not None), default=0))
    if R > MAX_REFS:
        raise ValueError("scnattn.textmetrics: %d references for one image exceed the limit of %d" % (R, MAX_REFS))
    pad, flat, lens = [0] * L, [], []
    for per in refs:
        for r in per + [None] * (R - len(per)):
            flat += pad if r is None else r + pad[len(r):]
            lens.append(-1 if r is None else len(r))
    host = torch.tensor(flat + lens, dtype=torch.int32)                        # tokens, then lengths: one buffer, one upload
    dev = host.to(device)
    return dev[:N * R * L].view(N, R, L), dev[N * R * L:].view(N, R)


def _skip(ids):
    ids = [int(x) for x in ids]
    return (C.c_int32 * max(1, len(ids)))(*ids), len(ids)


def ngram_stats(hyp, hyp_len, ref, ref_len, skip_hyp=(), skip_ref=()):
    """scnattn_text_ngram_stats: int32 [N, 10] -- clipped matches n = 1..4, guesses n = 1..4, hypothesis length, closest
    reference length (include/scnattn.h)."""
    _lib.require_cuda(hyp, hyp_len, ref, ref_len)
    N, Lh = hyp.shape
    _, R, Lr = ref.shape
    stats = torch.empty(N, 10, dtype=torch.int32, device=hyp.device)
    sh, nh = _skip(skip_hyp)
    sr, nr = _skip(skip_ref)
    _lib.call("scnattn_text_ngram_stats", _lib.stream_of(hyp), N, R, _lib.ptr(hyp), Lh, _lib.ptr(hyp_len), _lib.ptr(ref), Lr,
              _lib.ptr(ref_len), sh, nh, sr, nr, _lib.ptr(stats))
    return stats


def nltk_totals(stats):
    """The ten corpus integers of utils.metric.bleu_from_totals from per-image statistics, on the device (int64 [10]):
    matches n = 1..4, denominators n = 1..4 (each hypothesis contributing max(1, guesses)), hypothesis and reference length."""
    s = stats.to(torch.int64)
    return torch.cat([s[:, 0:4].sum(0), s[:, 4:8].clamp_min(1).sum(0), s[:, 8:10].sum(0)])


def bleu_coco(correct, guess, hyp_len, ref_len):
    """[Bleu_1 .. Bleu_4] in the COCO caption-evaluation form, from corpus totals."""
    tiny, small = 1e-15, 1e-9
    ratio = (hyp_len + tiny) / (ref_len + small)
    out, prod = [], 1.0
    for n in range(1, 5):
        prod *= (float(correct[n - 1]) + tiny) / (float(guess[n - 1]) + small)
        b = prod ** (1.0 / n)
        if ratio < 1:
            b *= math.exp(1 - 1 / ratio)
        out.append(b)
    return out


class CaptionScorer:
    """Holds the packed references of a test split and the CIDEr-D document-frequency tables built from them (once, with
    torch.sort / unique_consecutive over the keys of scnattn_text_ref_keys: table building, not the scoring path)."""

    def __init__(self, references, skip_ref=(), device="cuda"):
        if isinstance(references, tuple):
            ref, ref_len = references
            ref = ref.to(device=device, dtype=torch.int32).contiguous()
            ref_len = ref_len.to(device=device, dtype=torch.int32).contiguous()
        else:
            ref, ref_len = pack_references(references, device)
        _lib.require_cuda(ref, ref_len)
        self.ref, self.ref_len, self.skip_ref = ref, ref_len, tuple(int(x) for x in skip_ref)
        self.N, self.R, self.Lr = ref.shape
        if self.N == 0:
            raise ValueError("CaptionScorer: no images")
        if tuple(ref_len.shape) != (self.N, self.R):
            raise ValueError("CaptionScorer: ref_len must be [N, R]")
        self._fit()

    def _fit(self):
        N, R, Lr = self.N, self.R, self.Lr
        dev = self.ref.device
        keys = torch.empty(N, R, Lr, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        seen = torch.zeros(1, dtype=torch.int32, device=dev)
        sr, nr = _skip(self.skip_ref)
        tk, td, off = [], [], [0]
        for n in range(1, 5):
            _lib.call("scnattn_text_ref_keys", _lib.stream_of(keys), n, N, R, _lib.ptr(self.ref), Lr, _lib.ptr(self.ref_len),
                      sr, nr, _lib.ptr(keys), _lib.ptr(flag))
            seen |= flag
            k = keys.reshape(-1)
            uniq, cnt = torch.unique_consecutive(torch.sort(k[k != -1])[0], return_counts=True)
            tk.append(uniq)
            td.append(cnt.to(torch.int32))
            off.append(off[-1] + uniq.numel())
        if int(seen.item()):
            raise ValueError("CaptionScorer: CIDEr-D needs reference token ids in 0..%d" % CIDER_MAX_TOKEN)
        self.table_keys, self.table_df = torch.cat(tk).contiguous(), torch.cat(td).contiguous()
        self.table_off = off
        self._off_c = (C.c_long * 5)(*off)

    def score(self, hypotheses, skip_hyp=(), per_image=False):
        """{'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr', 'bleu4_nltk'} for one hypothesis per image; `hypotheses` as for
        pack_captions, or an already packed (tokens, lengths) pair on the device.  One download.  per_image=True adds the
        device tensors 'stats' int32 [N, 10], 'lcs' int32 [N, R], 'rouge_l' fp64 [N], 'cider' fp64 [N]."""
        dev = self.ref.device
        if isinstance(hypotheses, tuple):
            hyp, hyp_len = hypotheses
            hyp = hyp.to(device=dev, dtype=torch.int32).contiguous()
            hyp_len = hyp_len.to(device=dev, dtype=torch.int32).contiguous()
        else:
            hyp, hyp_len = pack_captions(hypotheses, dev)
        N, Lh = hyp.shape
        if N != self.N or tuple(hyp_len.shape) != (N,):
            raise ValueError("CaptionScorer.score: %d hypotheses for %d images" % (N, self.N))
        R, Lr = self.R, self.Lr
        sh, nh = _skip(skip_hyp)
        sr, nr = _skip(self.skip_ref)
        st = _lib.stream_of(hyp)
        stats = ngram_stats(hyp, hyp_len, self.ref, self.ref_len, skip_hyp, self.skip_ref)
        lcs = torch.empty(N, R, dtype=torch.int32, device=dev)
        rouge = torch.empty(N, dtype=torch.float64, device=dev)
        cider = torch.empty(N, dtype=torch.float64, device=dev)
        means = torch.empty(2, dtype=torch.float64, device=dev)
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call("scnattn_text_lcs", st, N, R, _lib.ptr(hyp), Lh, _lib.ptr(hyp_len), _lib.ptr(self.ref), Lr,
                  _lib.ptr(self.ref_len), sh, nh, sr, nr, _lib.ptr(lcs), _lib.ptr(rouge), C.c_void_p(means.data_ptr()))
        _lib.call("scnattn_text_cider", st, N, R, _lib.ptr(hyp), Lh, _lib.ptr(hyp_len), _lib.ptr(self.ref), Lr,
                  _lib.ptr(self.ref_len), sh, nh, sr, nr, _lib.ptr(self.table_keys), _lib.ptr(self.table_df), self._off_c,
                  self.N, _lib.ptr(cider), C.c_void_p(means.data_ptr() + 8), _lib.ptr(flag))
        s64 = stats.to(torch.int64)
        down = torch.cat([s64.sum(0).double(), s64[:, 4:8].clamp_min(1).sum(0).double(), means, flag.double()]).cpu().tolist()
        if down[16] != 0:
            raise ValueError("CaptionScorer.score: CIDEr-D needs token ids in 0..%d" % CIDER_MAX_TOKEN)
        tot = [int(x) for x in down[:14]]
        out = {"Bleu_%d" % (n + 1): b for n, b in enumerate(bleu_coco(tot[0:4], tot[4:8], tot[8], tot[9]))}
        out["ROUGE_L"], out["CIDEr"] = down[14], down[15]
        out["bleu4_nltk"] = bleu_from_totals(tot[0:4], tot[10:14], tot[8], tot[9])
        if per_image:
            out.update(stats=stats, lcs=lcs, rouge_l=rouge, cider=cider)
        return out

    def score_rows(self, image_index, hyp, hyp_len, skip_hyp=()):
        """Per-row CIDEr-D of any number of captions, each against the references of the image `image_index[row]` names:
        the reward of self-critical training.  hyp int32 [rows, Lh] / hyp_len int32 [rows] packed on the device,
        image_index an integer vector of `rows` entries in [0, N) (device, or host: then it is uploaded).  The document
        frequencies and the document count are the CORPUS's (the fitted tables, self.N), whatever the number of rows, so
        image_index = arange(N) gives the bits of score(per_image=True)['cider'].  Returns (cider fp64 [rows], flag int32
        [1]: non-zero when a token lay outside 0..65534) as device tensors: no download, no synchronisation.  An index
        outside [0, N) is refused when image_index is given on the host; a device index is clamped into range by the
        gather, so a wrong one scores against the wrong image instead of faulting."""
        dev = self.ref.device
        if hyp.dim() != 2 or hyp_len.dim() != 1 or hyp_len.numel() != hyp.shape[0]:
            raise ValueError("CaptionScorer.score_rows: hyp must be [rows, Lh] and hyp_len [rows]")
        rows = hyp.shape[0]
        image_index = torch.as_tensor(image_index)
        if image_index.dim() != 1 or image_index.numel() != rows or image_index.dtype.is_floating_point:
            raise ValueError("CaptionScorer.score_rows: image_index must be an integer vector of %d entries (got %s)"
                             % (rows, tuple(image_index.shape)))
        if not image_index.is_cuda and rows and (int(image_index.min()) < 0 or int(image_index.max()) >= self.N):
            raise ValueError("CaptionScorer.score_rows: image_index outside [0, %d)" % self.N)
        _lib.require_cuda(hyp, hyp_len)
        hyp = hyp.to(device=dev, dtype=torch.int32).contiguous()
        hyp_len = hyp_len.to(device=dev, dtype=torch.int32).contiguous()
        idx = image_index.to(device=dev, dtype=torch.int64).clamp(0, self.N - 1)
        ref, ref_len = self.ref.index_select(0, idx), self.ref_len.index_select(0, idx)
        sh, nh = _skip(skip_hyp)
        sr, nr = _skip(self.skip_ref)
        cider = torch.empty(rows, dtype=torch.float64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if rows:
            _lib.call("scnattn_text_cider", _lib.stream_of(hyp), rows, self.R, _lib.ptr(hyp), hyp.shape[1], _lib.ptr(hyp_len),
                      _lib.ptr(ref), self.Lr, _lib.ptr(ref_len), sh, nh, sr, nr, _lib.ptr(self.table_keys),
                      _lib.ptr(self.table_df), self._off_c, self.N, _lib.ptr(cider), None, _lib.ptr(flag))
        return cider, flag
