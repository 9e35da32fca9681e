"""Images in, captions out: the batched body of the reference's inference.py:81-160.

Reference, per image: `read_image` (imresize to 256 x 256, transpose, / 255., Normalize), `encoder_tagger(image)`,
`encoder_caption(image)`, `decoder.sample(beam_size, word_map, encoder_out[, tags])`, then the words through the
reversed word map.  Here a batch of decoded images goes through one resize-and-normalise launch
(`data.resize_normalize`), the eval-mode trunks and the batched beam search (`decoder.sample_batch`), all on the device.
With `overlays=True` the records also carry the pictures of `visualize_att` (utils/vizualize.py): per word the
photograph under that word's smoothed attention map, made on the device by `scnattn.viz`.
The modules are taken as given: no checkpoint loading, no file decoding, no CLI, no matplotlib figure.
"""
import numpy as np
import torch

from . import data, viz
from ._lib import require_cuda

_SPECIAL = ("<start>", "<end>", "<pad>")        # utils/token.py; dropped from the sentence (inference.py:156-157)
SCORE_MAX_TOKENS = 51       # the step limit of the device drivers (scnattn.functional.BEAM_MAX_STEPS)


def rerank_order(records, length_penalty=0.0):
    """records of `Captioner.score` (each with "score" and "tokens" = <start> + the scored tokens) -> the same records
    sorted by score / n_tokens**length_penalty, largest first; equal keys keep their input order (a stable sort)."""
    length_penalty = float(length_penalty)
    if length_penalty != length_penalty or length_penalty in (float("inf"), float("-inf")):
        raise ValueError("rerank: length_penalty must be finite (got %r)" % (length_penalty,))
    return sorted(records, key=lambda r: -(r["score"] / float(len(r["tokens"]) - 1) ** length_penalty))


class Captioner:
    """`captioner(images, tag_count=0, overlays=False)` -> one record per image:
        tokens  the best sequence, `<start>` included, as `sample` returns it
        words   the sequence without <start>, <end>, <pad>, through the reversed word map
        alphas  the attention maps of the sequence for the two attention decoders, else None
        tags    with tag_count > 0 and a tagger: (indices, values) of the largest tag scores in the order
                `np.argsort(tags)[-tag_count:]` gives (inference.py:139-140), else None
        overlays  only with overlays=True: uint8 device tensor [len(alphas), 336, 336, 3], per word the photograph
                (Pillow LANCZOS to `overlay_size`) under the word's attention map, expanded by overlay_size / map size and
                smoothed with `overlay_sigma` (`viz.attention_overlays`); None for a decoder without attention
    encoder / tagger: modules mapping the normalised batch [N, 3, OH, OW] to (N, h, w, E) / (N, S); `size` is their
    input size (default: the module's `input_size` attribute, else 256 x 256).  The batch is produced in the layout and
    type a `DeviceBatchLoader` hands the same encoder: channels-last when the encoder asks for it, fp32 values
    (`image_dtype`; the fused stem reads fp32 images in both modes).  `dtype` bf16 runs the trunks under bf16 autocast, as
    `TrainStep` runs them; the decoder stays fp32.  `search_options`: a `models.decoders.SearchOptions` handed to
    `sample_batch` (n-gram blocking, minimum length, banned tokens, length penalty); None: the reference's search.
    `captioner.sample(images, samples=3, top_k=..., top_p=...)`: several sampled captions per image (below);
    `captioner.diverse(images, groups=3, beam_size=2, diversity=0.5)`: several captions per image by diverse beam search."""

    def __init__(self, encoder, decoder, word_map, tagger=None, beam_size=5, dtype=torch.float32,
                 mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, size=None, image_dtype=torch.float32,
                 overlay_size=(336, 336), overlay_sigma=8, overlay_weight=0.8, search_options=None):
        from models.decoders.pure_attention import PureAttention
        from models.decoders.pure_scn import PureSCN
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("Captioner: dtype must be float32 or bfloat16")
        # a DecoderEnsemble states both itself (any member with tags / the member whose maps it returns)
        self.needs_tags = getattr(decoder, "needs_tags", not isinstance(decoder, PureAttention))   # inference.py:73-74 (scn_based_model)
        self.has_alphas = getattr(decoder, "has_alphas", not isinstance(decoder, PureSCN))         # att_based_model
        if self.needs_tags and tagger is None:
            raise ValueError("Captioner: a %s decoder needs a tagger" % type(decoder).__name__)
        for tok in _SPECIAL:
            if tok not in word_map:
                raise ValueError("Captioner: word_map lacks %r" % tok)
        self.encoder, self.decoder, self.tagger = encoder, decoder, tagger
        self.word_map, self.beam_size, self.dtype, self.image_dtype = word_map, int(beam_size), dtype, image_dtype
        self.rev_word_map = {v: k for k, v in word_map.items()}
        self.skip = {word_map[tok] for tok in _SPECIAL}
        if size is None:
            size = getattr(encoder, "input_size", (256, 256))
        self.size = (int(size[0]), int(size[1]))
        self.channels_last = bool(getattr(encoder, "channels_last", False))
        self.overlay_size = (int(overlay_size[0]), int(overlay_size[1]))       # utils/vizualize.py:26, 40-48
        self.overlay_sigma, self.overlay_weight = overlay_sigma, overlay_weight
        self.search_options = search_options        # a models.decoders.SearchOptions for sample_batch, or None
        p = next(decoder.parameters())
        require_cuda(p)
        self.device = p.device
        lut = data.identity_lut(3) if mean is None else data.normalize_lut(mean, std)
        self.lut = torch.from_numpy(lut).to(self.device)

    def images_to_batch(self, images):
        return data.resize_normalize(images, self.lut, size=self.size, dtype=self.image_dtype,
                                     channels_last=self.channels_last)

    def _encode(self, images, want_tags):
        """eval-mode trunks over the resized batch -> (encoder_out fp32, tags fp32 or None); the caller holds the device"""
        for m in (self.encoder, self.decoder, self.tagger):
            if m is not None and any(c.training for c in m.modules()):      # eval() itself walks and writes every module
                m.eval()
        batch = self.images_to_batch(images)
        tags = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.dtype == torch.bfloat16):
            encoder_out = self.encoder(batch)
            if self.tagger is not None and want_tags:
                tags = self.tagger(batch)
        return encoder_out.float(), None if tags is None else tags.float()

    @torch.no_grad()
    def sample(self, images, samples=3, temperature=1.0, top_k=0, top_p=1.0, seed=0, draw=0, greedy_first=False):
        """Several different captions per image by truncated sampling instead of one by search: the trunks and the batch
        path of `__call__`, then ONE `decoder.rollout_batch` (the whole rollout on the device) and one download.
        -> per image a list of `samples` (+ 1 with greedy_first: the arg-max caption first) records
            tokens  <start>, the sampled words, <end> (absent from a caption that was cut off at the step limit)
            words   the same without <start>, <end>, <pad>, through the reversed word map
            logp    the caption's log-probability under the distribution it was drawn from (temperature and filter
                    included)
        top_k / top_p cut the tail of every step's softmax (0 / 1.0: off; `rollout_batch`); (seed, draw) repeats the
        captions and the next `draw` gives fresh ones.  No alphas and no overlays."""
        if not hasattr(self.decoder, "rollout_batch"):
            raise ValueError("Captioner.sample: a %s cannot sample (no rollout_batch)" % type(self.decoder).__name__)
        from models.decoders._common import check_rollout_args
        K = check_rollout_args(samples, temperature, greedy_first, who="Captioner.sample", top_k=top_k, top_p=top_p)
        with torch.cuda.device(self.device):
            encoder_out, tags = self._encode(images, self.needs_tags)
            caps, caplens, sum_logp = self.decoder.rollout_batch(self.word_map, encoder_out, tags, samples=samples, seed=seed,
                                                                 draw=draw, temperature=temperature,
                                                                 greedy_first=greedy_first, top_k=top_k, top_p=top_p)
            # one download: the captions, their lengths and the bits of sum_logp side by side
            host = torch.cat([caps, caplens, sum_logp.view(torch.int32).to(torch.int64).unsqueeze(1)], dim=1).cpu()
        L = caps.shape[1]
        logp = host[:, L + 1].to(torch.int32).view(torch.float32)
        out = []
        for n in range(host.shape[0] // K):
            recs = []
            for r in range(n * K, (n + 1) * K):
                seq = host[r, :int(host[r, L])].tolist()
                recs.append({"tokens": seq, "words": [self.rev_word_map[w] for w in seq if w not in self.skip],
                             "logp": float(logp[r])})
            out.append(recs)
        return out

    @torch.no_grad()
    def diverse(self, images, groups=3, beam_size=2, diversity=0.5):
        """Several different captions per image by DIVERSE beam search instead of sampling: the trunks and the batch path
        of `__call__`, then ONE `decoder.sample_groups` (one search on the device, one download).  `groups` groups of
        `beam_size` beams each (groups x beam_size <= 8); a group pays `diversity` for every word an earlier group picked at
        the same step.  `search_options` are honoured.
        -> per image a list of `groups` records
            group   0 .. groups - 1
            tokens  the group's caption as `__call__` returns it (<start>, the words, <end> unless cut off)
            words   the same without <start>, <end>, <pad>, through the reversed word map
            score   the caption's sum of log-probabilities (nothing of the penalty is in it)
        groups = 1: the one record holds `__call__`'s caption."""
        if not hasattr(self.decoder, "sample_groups"):
            raise ValueError("Captioner.diverse: a %s has no sample_groups" % type(self.decoder).__name__)
        from models.decoders._common import check_groups_args
        check_groups_args(beam_size, groups, diversity, len(self.word_map), who="Captioner.diverse")
        with torch.cuda.device(self.device):
            encoder_out, tags = self._encode(images, self.needs_tags)
            results = self.decoder.sample_groups(beam_size, groups, diversity, self.word_map, encoder_out, tags,
                                                 options=self.search_options, with_scores=True)
        out = []
        for per_image in results:
            recs = []
            for g, (res, score) in enumerate(per_image):
                seq = res[0] if self.has_alphas else res
                recs.append({"group": g, "tokens": seq, "words": [self.rev_word_map[w] for w in seq if w not in self.skip],
                             "score": score})
            out.append(recs)
        return out

    @torch.no_grad()
    def constrained(self, images, words):
        """Captions that must CONTAIN given words (constrained beam search, `decoder.sample_constrained`): the trunks and
        the batch path of `__call__`, then one search on the device with `beam_size` beams.  `words`: one list of strings
        for all images, or one list per image (at most 4 distinct words each, an empty list: no requirement); a word is
        looked up in the word map and a missing one raises ValueError.  `search_options` are honoured.
        -> one record per image
            tokens     the caption as `__call__` returns it
            words      the same without <start>, <end>, <pad>, through the reversed word map
            alphas     the attention maps as `__call__` returns them (None without attention)
            score      the caption's sum of log-probabilities
            missing    the required words absent from the caption (only a caption cut off at the step limit can lack any)
            satisfied  not missing"""
        if not hasattr(self.decoder, "sample_constrained"):
            raise ValueError("Captioner.constrained: a %s has no sample_constrained" % type(self.decoder).__name__)
        images = list(images)
        words = list(words)
        if all(isinstance(w, str) for w in words):
            words = [words] * len(images)
        if len(words) != len(images):
            raise ValueError("Captioner.constrained: %d word lists for %d images" % (len(words), len(images)))
        required = []
        for per_image in words:
            if isinstance(per_image, str):
                raise ValueError("Captioner.constrained: words is one list of strings, or one list of strings per image")
            ids = []
            for w in per_image:
                if w not in self.word_map:
                    raise ValueError("Captioner.constrained: %r is not in the word map" % (w,))
                ids.append(self.word_map[w])
            required.append(ids)
        from models.decoders._common import check_required_args, device_options
        check_required_args(required, len(images), self.word_map, self.beam_size, device_options(self.search_options)[0],
                            who="Captioner.constrained")
        with torch.cuda.device(self.device):
            encoder_out, tags = self._encode(images, self.needs_tags)
            results = self.decoder.sample_constrained(self.beam_size, required, self.word_map, encoder_out, tags,
                                                      options=self.search_options, with_scores=True)
        records = []
        for (res, score), per_image, ids in zip(results, words, required):
            seq, alphas = res if self.has_alphas else (res, None)
            missing = [w for w, i in zip(per_image, ids) if i not in seq]
            records.append({"tokens": seq, "words": [self.rev_word_map[w] for w in seq if w not in self.skip],
                            "alphas": alphas, "score": score, "satisfied": not missing, "missing": missing})
        return records

    def caption_tokens(self, caption):
        """One given caption -> its token ids with <start> in front.  A list of token ids is taken as given (a leading
        <start> is not doubled; nothing is appended: a caption without <end> is scored without one).  A list of WORDS is a
        sentence: words outside the map become <unk>, and <end> is appended unless the sentence already ends with it."""
        caption = list(caption)
        start, end = self.word_map["<start>"], self.word_map["<end>"]
        if caption and all(isinstance(w, str) for w in caption):
            if "<unk>" not in self.word_map and any(w not in self.word_map for w in caption):
                raise ValueError("Captioner.score: a word is outside the word map, which has no <unk>")
            ids = [self.word_map.get(w, self.word_map.get("<unk>")) for w in caption]
            if ids[-1] != end:
                ids.append(end)
        else:
            if any(isinstance(w, (str, bool)) or int(w) != w for w in caption):
                raise ValueError("Captioner.score: a caption is a list of token ids or a list of words")
            ids = [int(w) for w in caption]
        if ids and ids[0] == start:
            ids = ids[1:]
        if not ids:
            raise ValueError("Captioner.score: an empty caption")
        if not all(0 <= w < len(self.word_map) for w in ids):
            raise ValueError("Captioner.score: a token id outside the vocabulary")
        if len(ids) > SCORE_MAX_TOKENS:
            raise ValueError("Captioner.score: a caption of %d tokens (at most %d)" % (len(ids), SCORE_MAX_TOKENS))
        return [start] + ids

    @torch.no_grad()
    def score(self, images, captions, temperature=1.0):
        """How likely does the model find THESE captions for these images: teacher-forced log-probabilities on the device
        (`decoder.score_batch`).  `captions`: per image a list of captions, each a list of token ids or of words
        (`caption_tokens`).  ONE pass of the trunks; the decoder scores 8 captions per image and call, so an image with
        more takes several calls over the same encoder output.  -> per image a list of records, in input order:
            tokens     <start> and the scored tokens
            words      the same without <start>, <end>, <pad>, through the reversed word map
            logp       per scored token its log-probability
            score      their sum, the caption's log-likelihood
            per_token  score / n_tokens
            rank       per scored token how many words the model ranks before it (0: the model's own choice); None under
                       an ensemble of several members"""
        if not hasattr(self.decoder, "score_batch"):
            raise ValueError("Captioner.score: a %s cannot score (no score_batch)" % type(self.decoder).__name__)
        images = list(images)
        captions = [list(c) for c in captions]
        if len(captions) != len(images):
            raise ValueError("Captioner.score: %d caption lists for %d images" % (len(captions), len(images)))
        seqs = [[self.caption_tokens(c) for c in per_image] for per_image in captions]
        N = len(images)
        most = max([len(s) for s in seqs] or [0])
        out = [[] for _ in range(N)]
        if most == 0:
            return out
        L = max(len(s) for per_image in seqs for s in per_image)
        pad = self.word_map["<pad>"]
        with torch.cuda.device(self.device):
            encoder_out, tags = self._encode(images, self.needs_tags)
            for c0 in range(0, most, 8):
                K = min(8, most - c0)
                caps = torch.full((N * K, L), pad, dtype=torch.int64)
                caplens = torch.zeros(N * K, 1, dtype=torch.int64)         # 0: an empty slot
                for n, per_image in enumerate(seqs):
                    for j, s in enumerate(per_image[c0:c0 + K]):
                        caps[n * K + j, :len(s)] = torch.tensor(s)
                        caplens[n * K + j, 0] = len(s)
                res = self.decoder.score_batch(self.word_map, encoder_out, tags, caps.to(self.device),
                                               caplens.to(self.device), per_image=K, temperature=temperature)
                # one download per call: the bits of logp and sum_logp beside the ranks
                rank = res["rank"] if res["rank"] is not None else torch.full_like(res["logp"], -1, dtype=torch.int32)
                host = torch.cat([res["logp"].view(torch.int32), rank, res["sum_logp"].view(torch.int32).unsqueeze(1)],
                                 dim=1).cpu()
                logp, ranks = host[:, :L - 1].view(torch.float32), host[:, L - 1:2 * (L - 1)]
                total = host[:, -1:].contiguous().view(torch.float32)
                for n, per_image in enumerate(seqs):
                    for j, s in enumerate(per_image[c0:c0 + K]):
                        r, nt = n * K + j, len(s) - 1
                        out[n].append({"tokens": s, "words": [self.rev_word_map[w] for w in s if w not in self.skip],
                                       "logp": logp[r, :nt].tolist(), "score": float(total[r, 0]),
                                       "per_token": float(total[r, 0]) / nt,
                                       "rank": None if res["rank"] is None else ranks[r, :nt].tolist()})
        return out

    def rerank(self, images, captions, length_penalty=0.0, temperature=1.0):
        """`score`, then per image the records sorted by score / n_tokens**length_penalty, best first (`rerank_order`:
        the form `SearchOptions.length_penalty` uses; ties keep the input order)."""
        return [rerank_order(recs, length_penalty) for recs in self.score(images, captions, temperature=temperature)]

    @torch.no_grad()
    def __call__(self, images, tag_count=0, overlays=False):
        with torch.cuda.device(self.device):
            encoder_out, tags = self._encode(images, self.needs_tags or tag_count > 0)
            kw = {} if self.search_options is None else {"options": self.search_options}
            if self.needs_tags:
                results = self.decoder.sample_batch(self.beam_size, self.word_map, encoder_out, tags, **kw)
            else:
                results = self.decoder.sample_batch(self.beam_size, self.word_map, encoder_out, **kw)
        tags_host = tags.cpu().numpy() if tags is not None and tag_count > 0 else None
        records = []
        for i, res in enumerate(results):
            seq, alphas = res if self.has_alphas else (res, None)
            rec = {"tokens": seq, "words": [self.rev_word_map[w] for w in seq if w not in self.skip], "alphas": alphas,
                   "tags": None}
            if tags_host is not None:
                t = np.asarray(tags_host[i].flatten().tolist())            # inference.py:139
                idx = np.argsort(t)[-tag_count:]
                rec["tags"] = (idx, t[idx])
            records.append(rec)
        if overlays:
            pictures = [None] * len(records)
            if self.has_alphas:
                hh, ww = np.asarray(records[0]["alphas"]).shape[1:]
                if self.overlay_size[0] % hh or self.overlay_size[0] * ww != self.overlay_size[1] * hh:
                    raise ValueError("Captioner: overlay_size %r is not a multiple of the %d x %d attention maps"
                                     % (self.overlay_size, hh, ww))
                with torch.cuda.device(self.device):
                    pictures = viz.attention_overlays(images, [r["alphas"] for r in records], size=self.overlay_size,
                                                      upscale=self.overlay_size[0] // hh, sigma=self.overlay_sigma,
                                                      weight=self.overlay_weight, device=self.device)
            for rec, pic in zip(records, pictures):
                rec["overlays"] = pic
        return records
