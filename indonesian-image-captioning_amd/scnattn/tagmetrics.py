"""Tagger evaluation on the device: tag mAP, per-image ranking AP, precision / recall at k, micro / macro precision, recall
and F1 at thresholds, and the reference's binary_accuracy (csrc/tagmetrics.hip through the C ABI).

The reference judges its tagger by binary_accuracy alone (trains/tagger.py, eval_tagger.py): agreement at 0.5 over all B * S
entries.  About ten of 1000 tags are set per image, so a tagger that answers all zeros scores about 99 %.  ``TagScorer``
accumulates the probabilities of a validation pass batch by batch -- ``update`` is one kernel launch and never synchronises --
and ``result`` downloads one small vector.  Definitions: include/scnattn.h and DESIGN 5t.  In short: average precision in the
tie-invariant counting form (equal to sklearn's average_precision_score per tag and, for rows with 0 < positives < S, to
label_ranking_average_precision_score); an entry is positive iff target >= 0.5; ties at the top-k cut go to the lower index.

Two conventions differ from sklearn's.  An image without a positive is LEFT OUT of every per-image mean and counted in
``n_images_empty`` (label_ranking_average_precision_score counts such a row as 1.0).  A tag without a positive is left out of
``map_tags`` and of the macro means and counted in ``n_tags_empty`` (sklearn gives it 0 with a warning).  Micro-averaged AP
over all n * S entries is not computed.

There is no CPU fallback: tensors must live on an MI355X device."""
import ctypes as C

import torch

from . import _lib

MAX_S, MAX_K, MAX_THRESHOLDS = _lib.TAG_MAX_S, _lib.TAG_MAX_K, _lib.TAG_MAX_THRESHOLDS


class TagScorer:
    """TagScorer(semantic_size, capacity): room for `capacity` images of `semantic_size` tags (5 bytes per entry on the
    device).  `ks`: up to 4 cut-offs for precision / recall at k; `thresholds`: up to 8 decision thresholds."""

    def __init__(self, semantic_size, capacity, ks=(1, 5, 10, 20), thresholds=(0.5,), device="cuda"):
        S, cap = int(semantic_size), int(capacity)
        self.ks = tuple(int(k) for k in ks)
        self.thresholds = tuple(float(x) for x in thresholds)
        if not 1 <= S <= MAX_S:
            raise ValueError("TagScorer: semantic_size outside 1..%d" % MAX_S)
        if not 1 <= cap <= _lib.TAG_MAX_IMAGES:
            raise ValueError("TagScorer: capacity outside 1..%d" % _lib.TAG_MAX_IMAGES)
        if len(self.ks) > MAX_K or any(k < 1 for k in self.ks):
            raise ValueError("TagScorer: at most %d values of k, each >= 1" % MAX_K)
        if len(self.thresholds) > MAX_THRESHOLDS:
            raise ValueError("TagScorer: at most %d thresholds" % MAX_THRESHOLDS)
        self.S, self.capacity = S, cap
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("scnattn.tagmetrics: the HIP path needs an MI355X device; there is no CPU fallback")
        nk, nt = len(self.ks), len(self.thresholds)
        self._ks_c = (C.c_int32 * max(1, nk))(*self.ks)
        self._th_c = (C.c_float * max(1, nt))(*self.thresholds)
        sb, lb = C.c_size_t(), C.c_size_t()
        _lib.call("scnattn_tag_store_size", S, cap, C.byref(sb), C.byref(lb))
        dev = self.device
        self.store_scores = torch.empty(sb.value // 4, dtype=torch.float32, device=dev).view(S, cap)
        self.store_labels = torch.empty(lb.value, dtype=torch.uint8, device=dev).view(S, cap)
        self.row_ap = torch.empty(cap, dtype=torch.float64, device=dev)
        self.row_npos = torch.empty(cap, dtype=torch.int32, device=dev)
        self.row_hits = torch.empty(cap, max(1, nk), dtype=torch.int32, device=dev)
        self.col_ap = torch.empty(S, dtype=torch.float64, device=dev)
        self.col_npos = torch.empty(S, dtype=torch.int32, device=dev)
        self.col_counts = torch.empty(S, max(1, nt), 3, dtype=torch.int32, device=dev)
        self.col_agree = torch.empty(S, dtype=torch.int32, device=dev)
        self.summary = torch.empty(_lib.TAG_SUMMARY_LEN, dtype=torch.float64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.n = 0
        self._result = None

    def reset(self):
        self.n = 0
        self._result = None
        self.flag.zero_()

    def update(self, probs, targets):
        """One batch: probs fp32 [B, S] (rows may be strided), targets fp32 / uint8 / bool [B, S].  One launch on the current
        stream, no synchronisation.  Raises ValueError past the capacity."""
        _lib.require_cuda(probs, targets)
        if probs.dim() != 2 or probs.shape[1] != self.S or tuple(targets.shape) != tuple(probs.shape):
            raise ValueError("TagScorer.update: probs and targets must both be [B, %d]" % self.S)
        B = probs.shape[0]
        if self.n + B > self.capacity:
            raise ValueError("TagScorer.update: %d + %d images exceed the capacity of %d" % (self.n, B, self.capacity))
        if probs.dtype != torch.float32:
            raise ValueError("TagScorer.update: probs must be float32")
        if targets.dtype == torch.bool:
            targets = targets.view(torch.uint8)
        elif targets.dtype not in (torch.float32, torch.uint8):
            raise ValueError("TagScorer.update: targets must be float32, uint8 or bool")
        if B == 0:
            return
        if probs.stride(1) != 1 or probs.stride(0) < self.S:
            probs = probs.contiguous()
        if targets.stride(1) != 1 or targets.stride(0) < self.S:
            targets = targets.contiguous()
        _lib.call("scnattn_tag_rows", _lib.stream_of(probs), B, self.S, _lib.ptr(probs), probs.stride(0), _lib.ptr(targets),
                  int(targets.dtype == torch.uint8), targets.stride(0), self.n, self.capacity, self._ks_c, len(self.ks),
                  _lib.ptr(self.store_scores), _lib.ptr(self.store_labels), _lib.ptr(self.row_ap), _lib.ptr(self.row_npos),
                  _lib.ptr(self.row_hits), _lib.ptr(self.flag))
        self.n += B
        self._result = None

    def result(self):
        """The summary as a dict of floats / ints; one download.  Raises ValueError when a score was not a finite number in
        [0, 1], or when nothing was accumulated."""
        if self._result is not None:
            return dict(self._result)
        if self.n == 0:
            raise ValueError("TagScorer.result: no images")
        st = _lib.stream_of(self.summary)
        nk, nt = len(self.ks), len(self.thresholds)
        _lib.call("scnattn_tag_cols", st, self.S, self.n, self.capacity, _lib.ptr(self.store_scores), _lib.ptr(self.store_labels),
                  self._th_c, nt, _lib.ptr(self.col_ap), _lib.ptr(self.col_npos), _lib.ptr(self.col_counts),
                  _lib.ptr(self.col_agree))
        _lib.call("scnattn_tag_finalize", st, self.S, self.n, self._ks_c, nk, nt, _lib.ptr(self.row_ap), _lib.ptr(self.row_npos),
                  _lib.ptr(self.row_hits), _lib.ptr(self.col_ap), _lib.ptr(self.col_npos), _lib.ptr(self.col_counts),
                  _lib.ptr(self.col_agree), _lib.ptr(self.flag), _lib.ptr(self.summary))
        v = self.summary.cpu().tolist()
        if v[62] != 0:
            raise ValueError("TagScorer.result: tag probabilities must be finite and in [0, 1]")
        out = {"map_tags": v[0], "ap_images": v[1],
               "precision_at": {k: v[2 + q] for q, k in enumerate(self.ks)},
               "recall_at": {k: v[6 + q] for q, k in enumerate(self.ks)}}
        for q, th in enumerate(self.thresholds):
            o = v[10 + 6 * q:16 + 6 * q]
            out["threshold_%g" % th] = {"micro_precision": o[0], "micro_recall": o[1], "micro_f1": o[2],
                                        "macro_precision": o[3], "macro_recall": o[4], "macro_f1": o[5]}
        out.update(binary_accuracy=v[58], n_images=int(v[59]), n_images_empty=int(v[60]), n_tags_empty=int(v[61]))
        self._result = out
        return dict(out)

    def per_image(self):
        """Device tensors over the images accumulated: 'ap' fp64 [n], 'npos' int32 [n], 'hits' int32 [n, len(ks)]."""
        self.result()
        n = self.n
        return {"ap": self.row_ap[:n], "npos": self.row_npos[:n], "hits": self.row_hits[:n, :len(self.ks)]}

    def per_tag(self):
        """Device tensors over the tags: 'ap' fp64 [S], 'npos' int32 [S], and 'tp', 'fp', 'fn' int32 [S, len(thresholds)] --
        e.g. (per_tag()['tp'][:, 0] == 0) & (per_tag()['npos'] > 0) names the tags that are never found."""
        self.result()
        c = self.col_counts[:, :len(self.thresholds)]
        return {"ap": self.col_ap, "npos": self.col_npos, "tp": c[..., 0], "fp": c[..., 1], "fn": c[..., 2]}
