"""The options of the batched beam search (include/scnattn.h: scnattn_search_options): no-repeat n-grams, a
minimum length, banned tokens -- applied on the device, inside the selection kernel -- and a length-normalised choice among
the finished beams, applied on the host when the results are read.  The reference's search has none of them; the
semantics are this project's and are stated in the header."""
import math

from utils.token import end_token, unknown_token

MAX_BANNED, MAX_NGRAM = 64, 8      # SCNATTN_MAX_BANNED, SCNATTN_MAX_NGRAM


class SearchOptions:
    """``SearchOptions(min_length=0, no_repeat_ngram=0, banned_tokens=(), length_penalty=0.0)``

    min_length        <end> is not a candidate at the 0-based steps t < min_length: a caption has at least that many words
    no_repeat_ngram   g in [1, 8]: no sequence of g words occurs twice in a caption (0: off)
    banned_tokens     at most 64 distinct token ids that are never candidates (<end> may not be among them)
    length_penalty    alpha: the returned caption is the first maximum, in completion order, of score / L**alpha, L = the
                      number of decoded tokens, <end> included (0: the best raw score, as without options)

    Excluded candidates are left out, nothing is renormalised: scores stay sums of the model's log-probabilities.  Ranges
    are checked here (ValueError); what depends on the vocabulary and the beam size is checked by ``check``."""

    def __init__(self, min_length=0, no_repeat_ngram=0, banned_tokens=(), length_penalty=0.0):
        self.min_length, self.no_repeat_ngram = int(min_length), int(no_repeat_ngram)
        if self.min_length != min_length or self.min_length < 0:
            raise ValueError("SearchOptions: min_length must be a non-negative integer (got %r)" % (min_length,))
        if self.no_repeat_ngram != no_repeat_ngram or not 0 <= self.no_repeat_ngram <= MAX_NGRAM:
            raise ValueError("SearchOptions: no_repeat_ngram must be in [0, %d] (got %r)" % (MAX_NGRAM, no_repeat_ngram))
        banned = tuple(sorted({int(x) for x in banned_tokens}))
        if any(x < 0 for x in banned):
            raise ValueError("SearchOptions: banned token ids must be non-negative (got %r)" % (banned,))
        if len(banned) > MAX_BANNED:
            raise ValueError("SearchOptions: at most %d banned tokens (got %d)" % (MAX_BANNED, len(banned)))
        self.banned_tokens = banned
        self.length_penalty = float(length_penalty)
        if not math.isfinite(self.length_penalty):
            raise ValueError("SearchOptions: length_penalty must be finite (got %r)" % (length_penalty,))

    @classmethod
    def from_words(cls, word_map, ban=(unknown_token,), **kw):
        """the same with the banned tokens given as words of `word_map` (default: <unk>)"""
        missing = [w for w in ban if w not in word_map]
        if missing:
            raise ValueError("SearchOptions.from_words: not in the word map: %r" % (missing,))
        opt = cls(banned_tokens=[word_map[w] for w in ban], **kw)
        if end_token in word_map:
            opt.check_end(word_map[end_token])
        return opt

    @property
    def on_device(self):
        """whether the device search has anything to exclude (otherwise the plain search runs, launch for launch)"""
        return bool(self.min_length or self.no_repeat_ngram or self.banned_tokens)

    def check_end(self, end):
        if end in self.banned_tokens:
            raise ValueError("SearchOptions: <end> (%d) may not be banned" % end)

    def check(self, vocab_size, beam_size, max_steps, end):
        """The refusals that depend on the search: <end> banned, a banned id outside the vocabulary, min_length beyond the
        step limit, and the candidate-count rule -- every live row must still offer beam_size candidates, for which
        vocab_size - banned - 1 - (no_repeat_ngram ? max_steps : 0) >= beam_size is sufficient."""
        self.check_end(end)
        if any(x >= vocab_size for x in self.banned_tokens):
            raise ValueError("SearchOptions: a banned token lies outside the vocabulary of %d words" % vocab_size)
        if self.min_length > max_steps - 1:
            raise ValueError("SearchOptions: min_length %d exceeds max_steps - 1 = %d" % (self.min_length, max_steps - 1))
        left = vocab_size - len(self.banned_tokens) - 1 - (max_steps if self.no_repeat_ngram >= 1 else 0)
        if left < beam_size:
            raise ValueError("SearchOptions: the options may leave a beam fewer than beam_size candidates: vocab_size %d - "
                             "%d banned - 1%s = %d < beam_size %d" % (
                                 vocab_size, len(self.banned_tokens),
                                 " - max_steps %d" % max_steps if self.no_repeat_ngram >= 1 else "", left, beam_size))

    def __repr__(self):
        return "SearchOptions(min_length=%d, no_repeat_ngram=%d, banned_tokens=%r, length_penalty=%r)" % (
            self.min_length, self.no_repeat_ngram, self.banned_tokens, self.length_penalty)
