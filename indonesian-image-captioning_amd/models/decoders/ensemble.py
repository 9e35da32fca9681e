"""An ensemble of caption decoders under ONE beam search (csrc/beam_search.cpp: scnattn_ensemble_*).

Published caption scores are normally those of an ensemble of the trained models.  The three decoders read the same
EncoderCaption features and the same tag vector and share one vocabulary, so the search state is one per image, not one
per model: every step runs the decode part of each member, ranks the candidates by the COMBINED distribution and advances
every member's recurrent state by the same parents."""
import torch
from torch import nn

from scnattn import functional as SF
from utils.token import start_token, end_token
from . import _common

COMBINE = ("logprob", "prob")


def _kind(decoder):
    """(use_attention, use_tags) of a member, as the three decoders pass them to the search"""
    from .attention_scn import AttentionSCN
    from .pure_attention import PureAttention
    from .pure_scn import PureSCN
    if isinstance(decoder, PureAttention):
        return True, False
    if isinstance(decoder, PureSCN):
        return False, True
    if isinstance(decoder, AttentionSCN):
        return True, True
    raise ValueError("DecoderEnsemble: %s is not one of AttentionSCN, PureSCN, PureAttention" % type(decoder).__name__)


class DecoderEnsemble(nn.Module):
    """``DecoderEnsemble(decoders, weights=None, combine="logprob", alpha_member=None)``

    decoders      1 to 4 of AttentionSCN / PureSCN / PureAttention with one ``vocab_size``
    weights       one positive number per member (None: equal); normalised to sum 1
    combine       "logprob": candidates are ranked by the weighted mean of the members' log-probabilities (the weighted
                  geometric mean of the probabilities); "prob": by the log of the weighted mean of their probabilities
    alpha_member  index of the member whose attention maps ``sample_batch`` returns (None: the first member with attention)

    ``sample_batch`` returns what a single decoder's ``sample_batch`` returns, so `scnattn.inference.Captioner` and
    `trains.harness.evaluate_captions` take an ensemble wherever they take a decoder.  fp32 only, like the search."""

    def __init__(self, decoders, weights=None, combine="logprob", alpha_member=None):
        super().__init__()
        decoders = list(decoders)
        if not 1 <= len(decoders) <= SF._lib.MAX_ENSEMBLE:
            raise ValueError("DecoderEnsemble: 1 to %d members (got %d)" % (SF._lib.MAX_ENSEMBLE, len(decoders)))
        self.kinds = [_kind(d) for d in decoders]
        if len({d.vocab_size for d in decoders}) != 1:
            raise ValueError("DecoderEnsemble: the members' vocab_size differ: %s" % [d.vocab_size for d in decoders])
        if combine not in COMBINE:
            raise ValueError("DecoderEnsemble: combine must be one of %s (got %r)" % (COMBINE, combine))
        self.member_weights = SF.normalise_member_weights(weights, len(decoders))
        with_att = [i for i, (att, _) in enumerate(self.kinds) if att]
        if alpha_member is None:
            alpha_member = with_att[0] if with_att else None
        elif alpha_member not in with_att:
            raise ValueError("DecoderEnsemble: alpha_member %r is not a member with attention" % (alpha_member,))
        self.decoders = nn.ModuleList(decoders)
        self.combine, self.alpha_member = combine, alpha_member
        self.vocab_size = decoders[0].vocab_size

    @property
    def needs_tags(self):
        return any(tags for _, tags in self.kinds)

    @property
    def has_alphas(self):
        return self.alpha_member is not None

    def sample_groups(self, beam_size, groups, diversity, word_map, encoder_out, tags=None, options=None, return_all=False,
                      with_scores=False):
        """Diverse beam search under the combined distribution (_common.beam_search_grouped): ``groups`` groups of
        ``beam_size`` beams -> per image a list of ``groups`` results, each what ``sample_batch`` returns for an image."""
        return self._search(beam_size, word_map, encoder_out, tags, return_all, options, groups=groups, diversity=diversity,
                            with_scores=with_scores)

    def sample_constrained(self, beam_size, required, word_map, encoder_out, tags=None, options=None, with_scores=False,
                           return_all=False, with_met=False):
        """Constrained beam search under the combined distribution (_common.beam_search_constrained): ``required[n]`` holds
        at most 4 token ids the caption of image n must contain -> per image what ``sample_batch`` returns."""
        if int(beam_size) != beam_size:
            raise ValueError("sample_constrained: beam_size must be an integer (got %r)" % (beam_size,))
        return self._search(int(beam_size), word_map, encoder_out, tags, return_all, options, with_scores=with_scores,
                            required=required, with_met=with_met)

    def sample_batch(self, beam_size, word_map, encoder_out, tags=None, return_all=False, options=None):
        """encoder_out (N, h, w, E), tags (N, S) (may be None when no member uses tags) -> list of N results in the form
        ``_common.beam_search_batched`` returns them: the sequence with the leading <start>, paired with the attention maps
        of ``alpha_member`` (the all-ones first map included) when there is one; the best open beam where nothing
        completed; with ``return_all`` each result paired with the image's completed (sequence, score) list.
        ``options``: a ``SearchOptions`` as a single decoder's ``sample_batch`` takes it (None / all-default: untouched)."""
        return self._search(int(beam_size), word_map, encoder_out, tags, return_all, options)

    def _search(self, beam_size, word_map, encoder_out, tags, return_all, options, groups=None, diversity=0.0,
                with_scores=False, required=None, with_met=False):
        """groups None: sample_batch with beam_size beams; else sample_groups with beam_size beams in each of the groups;
        required (groups None): sample_constrained"""
        V = len(word_map)
        G, lam = 1, 0.0
        if groups is None:
            k = beam_size
            if not 1 <= k <= SF._lib.MAX_BEAM:
                raise ValueError("sample_batch: beam_size must be in [1, %d] (got %d)" % (SF._lib.MAX_BEAM, k))
        else:
            _, G, k, lam = _common.check_groups_args(beam_size, groups, diversity, V)     # k: the total over the groups
        if V != self.vocab_size:
            raise ValueError("sample_batch: the word map has %d words, the members' vocab_size is %d" % (V, self.vocab_size))
        if V < k:
            raise ValueError("sample_batch: vocab_size %d is smaller than beam_size %d" % (V, k))
        if self.needs_tags and tags is None:
            raise ValueError("sample_batch: a member of the ensemble uses tags and none were given")
        start, end = word_map[start_token], word_map[end_token]
        dev_options, alpha = _common.device_options(options)
        if dev_options is not None:
            dev_options.check(V, k, SF.BEAM_MAX_STEPS, end)       # before anything touches the GPU
        pad = word_map.get(_common.padding_token, -1)
        if required is not None:
            required = _common.check_required_args(required, encoder_out.shape[0], word_map, k, dev_options)
        SF._lib.require_cuda(encoder_out, tags)
        N, hh, ww, _ = encoder_out.shape
        dims_list, weights_list, tags_list = [], [], []
        for dec, (use_att, use_tags) in zip(self.decoders, self.kinds):
            dims, weights, enc, tg = _common._search_operands(dec, V, encoder_out, tags if use_tags else None, use_att,
                                                              use_tags)
            dims_list.append(dims)
            weights_list.append(weights)
            tags_list.append(tg)
        res, steps = SF.ensemble_search_run(dims_list, k, weights_list, enc, tags_list, self.member_weights, self.combine,
                                            start, end, self.alpha_member, options=dev_options, groups=G, diversity=lam,
                                            required=required, pad_token=pad)
        out = _common.trace_back(res, steps, N, k, start, end, (hh, ww), self.has_alphas, return_all, length_penalty=alpha,
                                 groups=G, with_scores=with_scores, with_met=with_met)
        return [[x] for x in out] if groups is not None and G == 1 else out

    def score_batch(self, word_map, encoder_out, tags, caps, caplens, per_image, temperature=1.0, want_alpha=False):
        """The log-probabilities of GIVEN captions under the COMBINED distribution: every member's ``score_batch`` (the
        same arguments and refusals, `_common.score_batched`), then ``combine_logp`` on the device -- for every token
        exactly the score the ensemble search accumulates for it.  sum_logp is the fp32 sum of the combined records.
        rank and best are None for more than one member (they would need the combined row); alpha is that of
        ``alpha_member``.  A one-member ensemble returns the decoder's result bit for bit."""
        if len(word_map) != self.vocab_size:
            raise ValueError("score_batch: the word map has %d words, the members' vocab_size is %d"
                             % (len(word_map), self.vocab_size))
        if self.needs_tags and tags is None:
            raise ValueError("score_batch: a member of the ensemble uses tags and none were given")
        res = [dec.score_batch(word_map, encoder_out, tags, caps, caplens, per_image, temperature=temperature,
                               want_alpha=want_alpha and i == self.alpha_member)
               for i, dec in enumerate(self.decoders)]
        if len(res) == 1:
            return res[0]
        logp = combine_logp([r["logp"] for r in res], self.member_weights, COMBINE.index(self.combine))
        return dict(logp=logp, sum_logp=logp.sum(dim=1), n_tokens=res[0]["n_tokens"], rank=None, best=None,
                    alpha=None if self.alpha_member is None else res[self.alpha_member]["alpha"])


def combine_logp(logps, w, mode):
    """The header's ensemble formula taken at ONE word: logps the members' log-probabilities of it (tensors of one
    shape), w their weights -> mode 0 ("logprob"): sum_m w_m l_m, summed in member order; mode 1 ("prob"):
    a + log sum_m w_m exp(l_m - a) with a = max_m l_m.  In the dtype of `logps`, on their device.  A position where every
    member holds -inf gives -inf in both modes."""
    if mode == 0:
        c = w[0] * logps[0]
        for wm, l in zip(w[1:], logps[1:]):
            c = c + wm * l
        return c
    a = logps[0]
    for l in logps[1:]:
        a = torch.maximum(a, l)
    safe = torch.where(torch.isinf(a), torch.zeros_like(a), a)       # a = -inf: exp(l - a) would be NaN
    s = w[0] * torch.exp(logps[0] - safe)
    for wm, l in zip(w[1:], logps[1:]):
        s = s + wm * torch.exp(l - safe)
    return a + torch.log(s)
