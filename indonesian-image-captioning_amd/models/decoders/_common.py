"""Logic shared by the three caption decoders (the reference repeats it in each file):
length sort + permutation (attention_scn.py:115-131), the dropout mask that sits between h and fc
(:154), and beam search (:160-296)."""
import torch
import torch.nn.functional as F

from scnattn import functional as SF
from utils.token import start_token, end_token, padding_token


def sort_by_length(encoder_out, encoded_captions, caption_lengths, sort_ind=None, caplens_host=None):
    """Flatten pixels, sort rows by caption length (descending) and permute images + captions.
    Tags are deliberately NOT touched (the reference indexes the un-permuted tags, :152).
    Returns enc (B,P,E), caps (B,L), decode_lengths (list[int]), sort_ind.
    `caplens_host`: the same caption lengths as a CPU tensor, when the caller has them there anyway (a loader reads
    them from a JSON file): the Python list the loop bounds come from is then computed on the host and the forward
    pass has NO device synchronisation at all -- the host keeps running ahead of the GPU across the encoder / decoder
    boundary.  Without it: one sync, exactly where the reference has its `.tolist()` (:131)."""
    B, E = encoder_out.size(0), encoder_out.size(-1)
    enc = encoder_out.reshape(B, -1, E)
    lens = caption_lengths.squeeze(1)
    sort_given = sort_ind is not None
    if not sort_given:
        lens, sort_ind = lens.sort(dim=0, descending=True, stable=True)
    else:
        lens = lens[sort_ind]
    if caplens_host is not None and not sort_given:
        lh, ph = caplens_host.reshape(-1).cpu().sort(dim=0, descending=True, stable=True)    # same stable order as on the device
        decode_lengths, perm = (lh - 1).tolist(), ph.tolist()
    else:
        # the one host sync of the forward pass, as in the reference (`.tolist()`, :131); the permutation rides
        # along so that a batch that is already in order (fixed-length captions, or a loader that sorts) skips
        # the 51 MB gather of encoder_out and, when the encoder is fine-tuned, its scatter in the backward pass
        host = torch.stack([lens - 1, sort_ind]).tolist()
        decode_lengths, perm = host
    if perm != list(range(B)):
        enc = enc[sort_ind]
        encoded_captions = encoded_captions[sort_ind]
    return enc, encoded_captions, decode_lengths, (lens - 1).to(torch.int32), sort_ind


USE_PREPOOL = True     # set False to force the dense (B, P, E) path even when the encoder attached its source map


def attached_prepool(encoder_out):
    """The un-pooled trunk output (B, h, w, E) that `EncoderCaption.forward` attaches to the pooled tensor it
    returns, if `encoder_out` is still that very tensor, unmodified (same object, same version counter)."""
    if not USE_PREPOOL or encoder_out is None:
        return None
    tag = getattr(encoder_out, "_scn_prepool", None)
    if tag is None:
        return None
    pre, version = tag
    if version != encoder_out._version or pre.shape[0] != encoder_out.shape[0] or pre.shape[-1] != encoder_out.shape[-1]:
        return None
    return pre


def resolve_prepool(encoder_out, prepool, pool_size, attention_dim=None, who="forward"):
    """-> (tensor to sort/permute, PoolTaps or None).  The trunk map (B, h, w, E) is used instead of the pooled
    encoder_out when it was given (or attached by EncoderCaption), lives on the GPU, has vector-friendly widths
    and the pooling is an up-sampling one (windows of at most 2x2); otherwise the dense path is taken."""
    pre = prepool if prepool is not None else attached_prepool(encoder_out)
    pool = None
    if pre is not None and pre.is_cuda and pre.dim() == 4 and pre.shape[-1] % 4 == 0 \
            and (attention_dim is None or attention_dim % 4 == 0):
        out_hw = tuple(encoder_out.shape[1:3]) if encoder_out is not None else (pool_size, pool_size)
        try:
            pool = SF.pool_taps(pre.shape[1], pre.shape[2], out_hw[0], out_hw[1], pre.device)
        except ValueError:
            pool = None
    if pool is None and encoder_out is None:
        raise RuntimeError("%s: encoder_out is None and no usable prepool map was given" % who)
    return (pre if pool is not None else encoder_out), pool


def active_rows(decode_lengths):
    return [sum(l > t for l in decode_lengths) for t in range(max(decode_lengths))]


def make_drop_mask(module, B, T, D, device):
    """Pre-scaled Bernoulli mask for fc(dropout(h)) or None (eval mode / p == 0).  A test can pin the
    mask by setting ``module.drop_mask_override`` (B,T,D)."""
    override = getattr(module, "drop_mask_override", None)
    if override is not None:
        return override.to(device=device, dtype=torch.float32)
    p = module.dropout.p
    if not module.training or p <= 0.0:
        return None
    keep = 1.0 - p
    return torch.empty((B, T, D), device=device, dtype=torch.float32).bernoulli_(keep).div_(keep)


def beam_search(decoder, beam_size, word_map, encoder_out, tag_out, use_attention, use_tags, return_all=False):
    """Beam search shared by AttentionSCN / PureSCN / PureAttention ``sample`` (reference
    attention_scn.py:160-296, pure_scn.py:142-249, pure_attention.py:153-281).  Identical control flow,
    with the unrolled-index split done by FLOOR division (the reference's ``/`` breaks on torch >= 1.5).
    ``return_all`` (tests): also return every completed (sequence, score) pair in completion order."""
    k = beam_size
    vocab_size = len(word_map)
    dev = encoder_out.device
    enc_image_size = encoder_out.size(1)
    encoder_dim = encoder_out.size(3)
    encoder_out = encoder_out.reshape(1, -1, encoder_dim)
    num_pixels = encoder_out.size(1)
    encoder_out = encoder_out.expand(k, num_pixels, encoder_dim).contiguous()
    tags = tag_out.expand(k, tag_out.size(1)).contiguous() if use_tags else None

    k_prev_words = torch.full((k, 1), word_map[start_token], dtype=torch.long, device=dev)
    seqs = k_prev_words
    top_k_scores = torch.zeros(k, 1, device=dev)
    seqs_alpha = torch.ones(k, 1, enc_image_size, enc_image_size, device=dev)
    complete_seqs, complete_seqs_alpha, complete_seqs_scores = [], [], []
    step = 1
    h, c = decoder.init_hidden_state(encoder_out)
    while True:
        embeddings = decoder.embedding(k_prev_words).squeeze(1)
        if use_attention:
            awe, alpha = decoder.attention(encoder_out, h)
            alpha = alpha.view(-1, enc_image_size, enc_image_size)
            gate = torch.sigmoid(SF.linear(h, decoder.f_beta.weight, decoder.f_beta.bias))
            step_in = torch.cat([embeddings, gate * awe], dim=1)
        else:
            alpha = None
            step_in = embeddings
        if use_tags:
            h, c = decoder.decode_step(step_in, tags, (h, c))
        else:
            h, c = decoder.decode_step(step_in, (h, c))
        scores = F.log_softmax(SF.linear(h, decoder.fc.weight, decoder.fc.bias), dim=1)
        scores = top_k_scores.expand_as(scores) + scores
        if step == 1:
            top_k_scores, top_k_words = scores[0].topk(k, 0, True, True)
        else:
            top_k_scores, top_k_words = scores.view(-1).topk(k, 0, True, True)
        prev_word_inds = torch.div(top_k_words, vocab_size, rounding_mode='floor')
        next_word_inds = top_k_words % vocab_size
        seqs = torch.cat([seqs[prev_word_inds], next_word_inds.unsqueeze(1)], dim=1)
        if use_attention:
            seqs_alpha = torch.cat([seqs_alpha[prev_word_inds], alpha[prev_word_inds].unsqueeze(1)], dim=1)
        nxt = next_word_inds.tolist()
        incomplete_inds = [i for i, w in enumerate(nxt) if w != word_map[end_token]]
        complete_inds = sorted(set(range(len(nxt))) - set(incomplete_inds))
        if complete_inds:
            complete_seqs.extend(seqs[complete_inds].tolist())
            if use_attention:
                complete_seqs_alpha.extend(seqs_alpha[complete_inds].tolist())
            complete_seqs_scores.extend(top_k_scores[complete_inds].tolist())
        k -= len(complete_inds)
        if k == 0:
            break
        seqs = seqs[incomplete_inds]
        if use_attention:
            seqs_alpha = seqs_alpha[incomplete_inds]
        keep = prev_word_inds[incomplete_inds]
        h, c = h[keep], c[keep]
        encoder_out = encoder_out[keep]
        if use_tags:
            tags = tags[keep]
        top_k_scores = top_k_scores[incomplete_inds].unsqueeze(1)
        k_prev_words = next_word_inds[incomplete_inds].unsqueeze(1)
        if step > 50:
            break
        step += 1
    if not complete_seqs_scores:  # nothing reached <end> within 50 steps: fall back to the best open beam
        complete_seqs = seqs.tolist()
        complete_seqs_scores = top_k_scores.view(-1).tolist()
        if use_attention:
            complete_seqs_alpha = seqs_alpha.tolist()
    i = complete_seqs_scores.index(max(complete_seqs_scores))
    seq = complete_seqs[i]
    out = (seq, complete_seqs_alpha[i]) if use_attention else seq
    if return_all:
        return out, list(zip(complete_seqs, complete_seqs_scores))
    return out


def _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags):
    """(dims, weights, enc (N, P, E), tags (N, S)) as the device drivers of the search and of the rollout take them"""
    N, hh, ww, E = encoder_out.shape
    P = hh * ww
    enc = encoder_out.reshape(N, P, E)
    D = decoder.decoder_dim
    if use_tags:
        from models.decoders.attention_scn import _collect_weights
        weights, Fd, S = _collect_weights(decoder), decoder.factored_dim, decoder.semantic_dim
    else:       # PureAttention: the LSTM cell through its SCN view, one constant "tag" (pure_attention.py)
        weights, Fd, S = decoder._scn_view_of_lstm(), D, 1
        tag_out = torch.ones(N, 1, device=enc.device)
    dims = (N, P, E, decoder.attention_dim if use_attention else 0, D, Fd, decoder.embed_dim, S, V, SF.BEAM_MAX_STEPS,
            SF.BEAM_MAX_STEPS, int(use_attention))
    return dims, weights, enc, tag_out


def device_options(options):
    """(what the device search gets, length_penalty): None for the device when there is nothing to exclude -- ``None`` or
    an all-default object takes the plain search, launch for launch"""
    if options is None:
        return None, 0.0
    return (options if options.on_device else None), options.length_penalty


def beam_search_batched(decoder, beam_size, word_map, encoder_out, tag_out, use_attention, use_tags, return_all=False,
                        options=None):
    """``beam_search`` for N images at once, the search itself on the device (csrc/beam_search.cpp): encoder_out
    (N, h, w, E), tag_out (N, S).  Returns a list of N results, each what ``beam_search`` returns for that image --
    the leading <start>, the all-ones first alpha map and this build's fallback to the best open beam included; with
    ``return_all`` each result is paired with the image's completed (sequence, score) list in completion order (by
    step, within a step by rank).
    K = beam_size slots per image; a step takes the top candidates of score + log_softmax ordered by (value
    descending, flat index beam * vocab_size + word ascending): among EQUAL values the lower flat index wins, where the
    reference leaves the choice to ``topk``.  Per step only token / parent / alpha records are kept; the sequences
    that are returned are read off the parent chain here.  1 <= beam_size <= 8 <= vocab_size; fp32 only.
    ``options``: a ``models.decoders.SearchOptions`` (n-gram blocking, minimum length, banned tokens inside the
    selection kernel, a length penalty in ``trace_back``); None or an all-default object: the search above, untouched."""
    from scnattn import _lib
    k = beam_size
    if not 1 <= k <= _lib.MAX_BEAM:
        raise ValueError("sample_batch: beam_size must be in [1, %d] (got %d)" % (_lib.MAX_BEAM, k))
    V = len(word_map)
    if V < k:
        raise ValueError("sample_batch: vocab_size %d is smaller than beam_size %d" % (V, k))
    start, end = word_map[start_token], word_map[end_token]
    dev_options, alpha = device_options(options)
    if dev_options is not None:
        dev_options.check(V, k, SF.BEAM_MAX_STEPS, end)       # before anything touches the GPU
    _lib.require_cuda(encoder_out, tag_out)
    N, hh, ww, E = encoder_out.shape
    dims, weights, enc, tag_out = _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags)
    res, steps = SF.beam_search_run(dims, k, weights, enc, tag_out, start, end, options=dev_options)
    return trace_back(res, steps, N, k, start, end, (hh, ww), use_attention, return_all, length_penalty=alpha)


def check_groups_args(beam_size, groups, diversity, V, who="sample_groups"):
    """The host-side refusals of a diverse search, before anything touches the GPU -> (beams per group, groups, total K,
    penalty): beam_size (PER GROUP) and groups integers >= 1 with beam_size * groups in [1, 8] and <= vocab_size, a finite
    penalty >= 0"""
    import math
    from scnattn import _lib
    if int(beam_size) != beam_size or int(groups) != groups or beam_size < 1 or groups < 1:
        raise ValueError("%s: beam_size and groups must be integers >= 1 (got %r, %r)" % (who, beam_size, groups))
    kg, G = int(beam_size), int(groups)
    K = kg * G
    if K > _lib.MAX_BEAM:
        raise ValueError("%s: beam_size x groups = %d beams per image exceeds %d" % (who, K, _lib.MAX_BEAM))
    if V < K:
        raise ValueError("%s: vocab_size %d is smaller than beam_size x groups = %d" % (who, V, K))
    lam = float(diversity)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("%s: the diversity penalty must be finite and not negative (got %r)" % (who, diversity))
    return kg, G, K, lam


def beam_search_grouped(decoder, beam_size, groups, diversity, word_map, encoder_out, tag_out, use_attention, use_tags,
                        return_all=False, options=None, with_scores=False):
    """DIVERSE beam search (include/scnattn.h; Vijayakumar et al. 2016) for N images on the device: ``groups`` groups of
    ``beam_size`` beams each, beam_size * groups <= 8.  Every group searches like ``beam_search_batched`` with beam_size
    beams, but at each step a candidate pays ``diversity`` for every pick of an earlier group with the same word at that
    step; returned scores are raw sums of log-probabilities.  Returns, per image, a list of ``groups`` results, each in
    the form ``beam_search_batched`` returns for an image (``return_all`` / ``options`` as there; the length penalty
    chooses per group).  groups == 1 is ``beam_search_batched`` bit for bit, whatever the penalty."""
    V = len(word_map)
    kg, G, K, lam = check_groups_args(beam_size, groups, diversity, V)
    start, end = word_map[start_token], word_map[end_token]
    dev_options, alpha = device_options(options)
    if dev_options is not None:
        dev_options.check(V, K, SF.BEAM_MAX_STEPS, end)       # the candidate-count rule takes the total K
    from scnattn import _lib
    _lib.require_cuda(encoder_out, tag_out)
    N, hh, ww, E = encoder_out.shape
    dims, weights, enc, tag_out = _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags)
    res, steps = SF.beam_search_run(dims, K, weights, enc, tag_out, start, end, options=dev_options, groups=G, diversity=lam)
    out = trace_back(res, steps, N, K, start, end, (hh, ww), use_attention, return_all, length_penalty=alpha, groups=G,
                     with_scores=with_scores)
    return out if G > 1 else [[x] for x in out]


def check_required_args(required, N, word_map, beam_size, options=None, who="sample_constrained"):
    """The host-side refusals of a constrained search, before anything touches the GPU (ValueError) -> the lists as lists
    of ints: one sequence per image, at most 4 distinct token ids of the vocabulary each, none of them <start>, <end>,
    <pad> or banned by ``options``; beam_size in [1, 8]; the candidate-count rule with 4 more words"""
    if isinstance(required, (str, bytes)) or not hasattr(required, "__len__"):
        raise ValueError("%s: required must hold one sequence of token ids per image" % who)
    lists = []
    for r in required:
        if isinstance(r, torch.Tensor):
            r = r.tolist()
        if isinstance(r, (str, bytes)) or not hasattr(r, "__iter__"):
            raise ValueError("%s: required must hold one sequence of token ids per image (got %r)" % (who, r))
        lists.append(list(r))
    try:
        SF.required_table(lists, N, len(word_map), beam_size, SF.BEAM_MAX_STEPS, word_map[start_token], word_map[end_token],
                          word_map.get(padding_token, -1), options)
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e)) from None
    return [[int(w) for w in r] for r in lists]


def beam_search_constrained(decoder, beam_size, required, word_map, encoder_out, tag_out, use_attention, use_tags,
                            return_all=False, options=None, with_scores=False, with_met=False):
    """CONSTRAINED beam search (include/scnattn.h; Anderson et al. 2017, Post & Vilar 2018) for N images on the device:
    ``required[n]`` holds at most 4 token ids the caption of image n must contain.  The beams of an image are kept in banks
    by the number of required words they have met and every step fills the banks round-robin; <end> is a candidate only for
    a beam that has met them all, so every completed caption satisfies its list.  Returns per image what
    ``beam_search_batched`` returns (``return_all`` / ``options`` as there); ``with_scores``: (result, raw score);
    ``with_met``: (result, raw score, bitmask of the required words the returned caption contains) -- the mask is
    incomplete only when nothing completed within the step limit.  Empty lists: ``beam_search_batched`` bit for bit."""
    from scnattn import _lib
    k = beam_size
    if int(k) != k or not 1 <= k <= _lib.MAX_BEAM:
        raise ValueError("sample_constrained: beam_size must be an integer in [1, %d] (got %r)" % (_lib.MAX_BEAM, k))
    k = int(k)
    V = len(word_map)
    if V < k:
        raise ValueError("sample_constrained: vocab_size %d is smaller than beam_size %d" % (V, k))
    start, end = word_map[start_token], word_map[end_token]
    dev_options, alpha = device_options(options)
    if dev_options is not None:
        dev_options.check(V, k, SF.BEAM_MAX_STEPS, end)       # before anything touches the GPU
    lists = check_required_args(required, encoder_out.shape[0], word_map, k, dev_options)
    _lib.require_cuda(encoder_out, tag_out)
    N, hh, ww, E = encoder_out.shape
    dims, weights, enc, tag_out = _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags)
    res, steps = SF.beam_search_run(dims, k, weights, enc, tag_out, start, end, options=dev_options, required=lists,
                                    pad_token=word_map.get(padding_token, -1))
    return trace_back(res, steps, N, k, start, end, (hh, ww), use_attention, return_all, length_penalty=alpha,
                      with_scores=with_scores, with_met=with_met)


def pick_best(done_scores, lengths, length_penalty):
    """index of the first maximum of score / L**alpha over the beams, in the order given (Python floats)"""
    norm = [s / float(L) ** length_penalty for s, L in zip(done_scores, lengths)]
    return norm.index(max(norm))


def trace_back(res, steps, N, k, start, end, map_hw, use_attention, return_all=False, length_penalty=0.0, groups=1,
               with_scores=False, with_met=False):
    """The results of a device search (SF.beam_search_run / SF.ensemble_search_run) -> the list of N results that
    ``beam_search_batched`` documents: the parent chains read off the token / parent records, the all-ones first alpha map
    (``use_attention``: the search kept maps), the fallback to the best open beam.
    ``length_penalty`` alpha != 0: the returned caption is the first maximum, in completion order (the open beams: slot
    order), of score / L**alpha with L = len(sequence) - 1, the decoded tokens with <end>; the (sequence, score) lists of
    ``return_all`` keep raw scores.  alpha == 0: the device's best_idx decides, as without options.
    ``groups`` > 1 (a diverse search; k is the TOTAL over the groups): the per-group records are read -- group g of image n
    keeps its completions at n*k + g*kg .., its open beams in slots g*kg .., its counters at n*groups + g -- and the result
    of an image is the list of its ``groups`` results, each in the form above.  ``with_scores``: each result is paired
    with the raw score of the caption it returns.
    A CONSTRAINED search (res["met"] is not None; include/scnattn.h): every completed beam has met all the image's required
    words; the fallback takes the open beams with the largest popcount(met) and chooses among THOSE as above (the higher
    score, then the lower slot; with alpha != 0 the length-normalised score) -- with no required words that is the fallback
    above.  ``with_met``: each result becomes (result, score, met_mask), met_mask the bitmask (bit c: the image's c-th
    required word) of what the returned caption contains."""
    hh, ww = map_hw
    kg = k // groups
    met = res["met"].tolist() if res.get("met") is not None else None
    full = [sum(1 << c for c, w in enumerate(row) if w >= 0) for row in res["required"].tolist()] if met is not None else None
    token, parent = res["token"].tolist(), res["parent"].tolist()
    alpha = res["alpha"]
    ones = torch.ones(1, hh, ww)

    def chain(n, t, slot):
        """sequence (and alpha rows) of the beam that sits in `slot` of image n after step t (0-based; -1: <start>)"""
        words, rows = [], []
        while t >= 0:
            r = n * k + slot
            words.append(token[t][r])
            slot = parent[t][r]
            rows.append((t, n * k + slot))
            t -= 1
        words.append(start)
        return words[::-1], rows[::-1]

    def alphas_of(rows):
        if not use_attention:
            return None
        maps = [ones] + [alpha[t, r].view(1, hh, ww) for t, r in rows]
        return torch.cat(maps).tolist()

    def group(n, g):
        """the result of group g of image n: its slots are g*kg .. g*kg + kg - 1 of the image"""
        sg, s0 = n * groups + g, g * kg
        done = []       # (sequence, alpha rows, score) in completion order
        for ci in range(int(res["ncomp"][sg])):
            r = n * k + s0 + ci
            t, src = int(res["comp_step"][r]), int(res["comp_parent"][r])
            words, rows = chain(n, t - 1, src)
            done.append((words + [end], rows + [(t, n * k + src)], float(res["comp_score"][r])))
        pool = None     # the beams the choice is among (indices into done); None: all of them
        masks = None
        if done:
            i = int(res["best_idx"][sg])
        else:           # nothing reached <end> within the step limit: the best open beam (rank order: slot 0)
            for s in range(s0, s0 + int(res["nsrc"][sg])):
                words, rows = chain(n, steps - 1, s)
                done.append((words, rows, float(res["scores"][n * k + s])))
            pool = list(range(len(done)))
            if met is not None:     # a constrained search: first the beams that met the most required words
                masks = [met[n * k + s0 + q] for q in pool]
                most = max(bin(m).count("1") for m in masks)
                pool = [q for q in pool if bin(masks[q]).count("1") == most]
            scores = [done[q][2] for q in pool]
            i = pool[scores.index(max(scores))]
        if length_penalty != 0.0:
            among = pool if pool is not None else list(range(len(done)))
            i = among[pick_best([done[q][2] for q in among], [len(done[q][0]) - 1 for q in among], length_penalty)]
        seq, rows, score = done[i]
        one = (seq, alphas_of(rows)) if use_attention else seq
        one = (one, [(s, sc) for s, _, sc in done]) if return_all else one
        if with_met:
            return one, score, (0 if met is None else masks[i] if masks is not None else full[n])
        return (one, score) if with_scores else one

    # The results are nested lists of plain numbers (an attention map per word: some 10 000 floats and 800 lists per
    # caption) and hold no reference cycles; the collector, woken by every few hundred new lists to walk all of them again,
    # made up most of this function's time once an image returns several captions.  It rests while they are built.
    import gc
    resting = gc.isenabled()
    gc.disable()
    try:
        if groups == 1:
            return [group(n, 0) for n in range(N)]
        return [[group(n, g) for g in range(groups)] for n in range(N)]
    finally:
        if resting:
            gc.enable()


def check_rollout_args(samples, temperature, greedy_first=False, who="rollout_batch", top_k=0, top_p=1.0):
    """The host-side refusals of a rollout: K = samples (+ 1 with greedy_first) slots per image in [1, 8], temperature > 0,
    and the sample filter's: top_k an integer >= 0 (0: off), top_p in (0, 1] (1: off), NaN refused"""
    from scnattn import _lib
    samples = int(samples)
    K = samples + (1 if greedy_first else 0)
    if samples < 1 or K > _lib.MAX_BEAM:
        raise ValueError("%s: %d slots per image (samples%s) outside [1, %d]"
                         % (who, K, " + the greedy slot" if greedy_first else "", _lib.MAX_BEAM))
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError("%s: temperature must be positive and finite (got %r)" % (who, temperature))
    SF.sample_filter_struct(top_k, top_p, who)
    return K


def rollout_batched(decoder, word_map, encoder_out, tag_out, use_attention, use_tags, samples=1, seed=0, draw=0,
                    temperature=1.0, greedy_first=False, top_k=0, top_p=1.0):
    """Sampled captions for N images, the whole rollout on the device (csrc/rollout.hip, SF.rollout_run): encoder_out
    (N, h, w, E), tag_out (N, S).  K = samples (+ 1 with greedy_first: slot 0 of every image is then the arg-max caption)
    slots per image, rows R = N*K ordered n*K + j.  Every token is a draw from softmax(logits / temperature); the noise
    is a pure function of (seed, draw, row, step, word), so the same (seed, draw) repeats the captions and the next
    `draw` gives fresh ones.  No dropout, like the search; fp32 only.
    top_k / top_p: truncated sampling (SF.rollout_run) -- every token is drawn from the top_k most likely words and / or
    the nucleus holding top_p of the mass, and sum_logp is the log-likelihood under that truncated, renormalised
    distribution.  The defaults (0, 1.0) are the full softmax and the plain kernels.
    Returns (caps (R, L) int64, caplens (R, 1) int64, sum_logp (R,)) ON THE DEVICE, in the form ``decoder.forward`` takes
    captions: caps = <start>, tokens ..., <end>, <pad> ...; caplens counts <start> and <end>, so decode_lengths =
    caplens - 1 is the number of sampled tokens and sum_logp their log-likelihood at this temperature.  A row that
    produced no <end> within the step limit is CUT OFF there: its caption is <start> and all `steps` tokens without an
    <end>, caplens = steps + 1 (decode_lengths = steps).  L = steps + 1."""
    K = check_rollout_args(samples, temperature, greedy_first, top_k=top_k, top_p=top_p)
    from scnattn import _lib
    _lib.require_cuda(encoder_out, tag_out)
    V = len(word_map)
    dims, weights, enc, tag_out = _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags)
    start, end, pad = word_map[start_token], word_map[end_token], word_map[padding_token]
    res, steps = SF.rollout_run(dims, K, weights, enc, tag_out, start, end, seed, draw, inv_temp=1.0 / float(temperature),
                                greedy_first=greedy_first, top_k=top_k, top_p=top_p)
    length = res["length"].to(torch.int64)
    n_tok = torch.where(length > 0, length, torch.full_like(length, steps))      # a cut-off row keeps every step
    R = length.numel()
    pos = torch.arange(steps, device=length.device).unsqueeze(0)
    caps = torch.full((R, steps + 1), pad, dtype=torch.int64, device=length.device)
    caps[:, 0] = start
    caps[:, 1:] = torch.where(pos < n_tok.unsqueeze(1), res["tokens"].to(torch.int64), caps[:, 1:])
    return caps, (n_tok + 1).unsqueeze(1), res["sum_logp"].clone()


SCORE_MAX_PER_IMAGE = 8       # captions of one image in one call: the K of the driver (scnattn._lib.MAX_BEAM)


def check_score_args(word_map, n_images, caps, caplens, per_image, temperature=1.0, who="score_batch"):
    """The refusals of ``score_batched`` (ValueError), on whatever device the captions live: per_image in [1, 8], caps
    (n_images * per_image, L) with caplens one per row, a positive finite temperature; then, on the data, caplens - 1 <= 51,
    <start> in front of every non-empty row, and every scored token inside the vocabulary.  The data checks are three
    flags computed where the captions are and read with ONE download (one synchronisation when that is the GPU).
    -> (per_image, ntok (R,) int64 on the captions' device)"""
    import operator
    try:
        per_image = operator.index(per_image)
    except TypeError:
        raise ValueError("%s: per_image must be an integer in [1, %d] (got %r)" % (who, SCORE_MAX_PER_IMAGE, per_image)) from None
    if not 1 <= per_image <= SCORE_MAX_PER_IMAGE:
        raise ValueError("%s: per_image must be in [1, %d] (got %d)" % (who, SCORE_MAX_PER_IMAGE, per_image))
    temperature = float(temperature)
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError("%s: temperature must be positive and finite (got %r)" % (who, temperature))
    R = n_images * per_image
    if caps.dim() != 2 or caps.shape[0] != R or caps.shape[1] < 1 or caplens.numel() != R:
        raise ValueError("%s: %d images x %d captions need caps (%d, L) and caplens (%d, 1) (got %s and %s)"
                         % (who, n_images, per_image, R, R, tuple(caps.shape), tuple(caplens.shape)))
    if caps.dtype.is_floating_point or caplens.dtype.is_floating_point:
        raise ValueError("%s: caps and caplens must be integer tensors" % who)
    V, L = len(word_map), caps.shape[1]
    ntok = (caplens.reshape(-1).to(torch.int64) - 1).clamp_min(0)
    tgt = caps[:, 1:].to(torch.int64)
    given = torch.arange(L - 1, device=caps.device).unsqueeze(0) < ntok.unsqueeze(1)
    too_long = (ntok > min(SF.BEAM_MAX_STEPS, L - 1)).any()
    no_start = ((caps[:, 0] != word_map[start_token]) & (ntok > 0)).any()
    outside = (((tgt < 0) | (tgt >= V)) & given).any()
    too_long, no_start, outside = torch.stack([too_long, no_start, outside]).tolist()
    if too_long:
        raise ValueError("%s: a caption has more than %d tokens after <start> (caplens - 1), or more than caps holds"
                         % (who, SF.BEAM_MAX_STEPS))
    if no_start:
        raise ValueError("%s: a non-empty caption does not begin with <start>" % who)
    if outside:
        raise ValueError("%s: a caption holds a token outside the vocabulary of %d words" % (who, V))
    return per_image, ntok


def score_batched(decoder, word_map, encoder_out, tag_out, use_attention, use_tags, caps, caplens, per_image,
                  temperature=1.0, want_alpha=False):
    """The log-probabilities of GIVEN captions, teacher-forced on the device (csrc/rollout.hip: rollout_score,
    SF.score_run): encoder_out (N, h, w, E), tag_out (N, S); caps (N*per_image, L) and caplens (N*per_image, 1) in the form
    ``forward`` takes and ``rollout_batch`` returns them, row n*per_image + j belonging to image n.  The scored tokens are
    caps[:, 1:caplens] (ntok = caplens - 1 of them); <end> is a token like any other, so a caption without one is scored
    as given.  caplens <= 1 marks an EMPTY slot (ragged input: fewer than per_image captions for an image); its records are
    zeros.  The per_image captions of an image share the image-side set-up, and no (rows, T, V) scores exist anywhere.
    No dropout, like the search; fp32 only.
    The arguments are checked before anything touches the GPU (check_score_args; ValueError); the checks that need the
    captions' values cost ONE synchronisation when the captions are on the device.
    Returns a dict ON THE DEVICE:
        logp (R, L-1)        log softmax(logits / temperature) at every given token, 0.0 beyond ntok
        sum_logp (R,)        their fp32 sum: the caption's log-likelihood
        n_tokens (R,) int32  ntok
        rank (R, L-1) int32  how many words the model ranks before the given one (0: it is the model's own word)
        best (R, L-1) int32  the model's own word at that position, given the caption so far
        alpha (R, L-1, P)    with want_alpha and attention: the attention maps of the given caption; else None"""
    from scnattn import _lib
    N = encoder_out.shape[0]
    per_image, ntok = check_score_args(word_map, N, caps, caplens, per_image, temperature)
    _lib.require_cuda(encoder_out, tag_out, caps, caplens)
    V = len(word_map)
    dims, weights, enc, tag_out = _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags)
    R, L = caps.shape
    T = SF.BEAM_MAX_STEPS
    targets = torch.zeros(R, T, dtype=torch.int32, device=caps.device)
    n = min(L - 1, T)
    targets[:, :n] = caps[:, 1:1 + n]
    res, steps = SF.score_run(dims, per_image, weights, enc, tag_out, word_map[start_token], targets, ntok.to(torch.int32),
                              inv_temp=1.0 / float(temperature), want_alpha=want_alpha)

    def padded(x):          # (R, steps, ...) -> (R, L - 1, ...), zeros beyond the longest caption
        out = torch.zeros((R, L - 1) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
        out[:, :steps] = x
        return out

    alpha = res["alpha"]
    return dict(logp=padded(res["logp"]), sum_logp=res["sum_logp"].clone(), n_tokens=res["ntok"].clone(),
                rank=padded(res["rank"]), best=padded(res["best"]),
                alpha=None if alpha is None else padded(alpha.transpose(0, 1)))


def check_mix_args(word_map, n_images, caps, caplens, per_image, prob, temperature=1.0, who="mix_batch"):
    """The refusals of ``mix_batched`` (ValueError): those of check_score_args, plus prob in [0, 1] (NaN refused).
    -> (per_image, nmix (R,) int64 on the captions' device, prob as the fp32 number the kernel compares with)"""
    prob = SF.mix_prob(prob, who)
    per_image, ntok = check_score_args(word_map, n_images, caps, caplens, per_image, temperature, who)
    return per_image, (ntok - 1).clamp_min(0), prob


def mix_batched(decoder, word_map, encoder_out, tag_out, use_attention, use_tags, caps, caplens, prob, per_image=1, seed=0,
                draw=0, temperature=1.0, greedy=False):
    """SCHEDULED SAMPLING (Bengio et al. 2015): the decoder's INPUT words for a teacher-forced pass, a share `prob` of them
    the model's own samples, mixed on the device (csrc/rollout.hip: rollout_pick_mixed, SF.mix_run).  encoder_out
    (N, h, w, E), tag_out (N, S); caps (N*per_image, L) and caplens (N*per_image, 1) in the form ``forward`` takes, row
    n*per_image + j belonging to image n.  ``forward`` embeds the positions 0 .. caplens - 2, so only the inputs at the
    positions 1 .. caplens - 2 can be replaced (nmix = max(caplens - 2, 0) of them); the last gold word is never an input
    and is never touched, and the TARGETS of the loss stay the caller's caps.  The word at position t + 1 is replaced when
    the coin of (seed, draw, row, t) falls below prob, by a draw from softmax(logits / temperature) after the mixed inputs
    0 .. t -- rollout_batch's pick with its noise -- or, with greedy, by the arg-max.  <end> is a word like any other.  No
    dropout, like the rollout; fp32 only.  The arguments are checked before anything touches the GPU (check_mix_args).
    Returns a dict ON THE DEVICE:
        inputs (R, L) int64       <start>, the mixed words, then caps unchanged from position caplens - 1 on
        replaced (R, L) bool      where inputs holds a sample
        sample (R, L-1) int32     the sample taken at step t (for position t + 1), -1 where none was
        logp (R, L-1)             its log-probability at this temperature, 0.0 elsewhere
        sum_logp (R,)             the fp32 sum of the row's logp
        n_replaced (R,) int32     how many inputs of the row were replaced"""
    from scnattn import _lib
    N = encoder_out.shape[0]
    per_image, nmix, prob = check_mix_args(word_map, N, caps, caplens, per_image, prob, temperature)
    _lib.require_cuda(encoder_out, tag_out, caps, caplens)
    V = len(word_map)
    dims, weights, enc, tag_out = _search_operands(decoder, V, encoder_out, tag_out, use_attention, use_tags)
    R, L = caps.shape
    T = SF.BEAM_MAX_STEPS
    gold = torch.zeros(R, T, dtype=torch.int32, device=caps.device)
    n = min(L - 1, T)
    gold[:, :n] = caps[:, 1:1 + n]
    res, steps = SF.mix_run(dims, per_image, weights, enc, tag_out, word_map[start_token], gold, nmix.to(torch.int32), prob,
                            seed, draw, inv_temp=1.0 / float(temperature), greedy=greedy)
    rep = res["replaced"] != 0
    inputs = caps.to(torch.int64).clone()
    inputs[:, 1:1 + steps] = torch.where(rep, res["tokens"].to(torch.int64), inputs[:, 1:1 + steps])
    replaced = torch.zeros(R, L, dtype=torch.bool, device=caps.device)
    replaced[:, 1:1 + steps] = rep
    sample = torch.full((R, L - 1), -1, dtype=torch.int32, device=caps.device)
    sample[:, :steps] = torch.where(rep, res["sample"], sample[:, :steps])
    logp = torch.zeros(R, L - 1, dtype=torch.float32, device=caps.device)
    logp[:, :steps] = res["logp"]
    return dict(inputs=inputs, replaced=replaced, sample=sample, logp=logp, sum_logp=res["sum_logp"].clone(),
                n_replaced=rep.sum(dim=1, dtype=torch.int32))


def score_matrix(decoder, word_map, encoder_out, tags, caps, caplens, temperature=1.0):
    """Every one of Q captions against every one of N images -> (N, Q) log-likelihoods on the device (image-caption
    retrieval; recall@k stays with the caller).  caps (Q, L), caplens (Q, 1).  A loop of ``score_batch`` calls, 8 captions
    at a time, every image scoring the same 8."""
    N, Q = encoder_out.shape[0], caps.shape[0]
    if caps.dim() != 2 or caplens.numel() != Q:
        raise ValueError("score_matrix: caps must be (Q, L) and caplens (Q, 1) (got %s and %s)"
                         % (tuple(caps.shape), tuple(caplens.shape)))
    caplens = caplens.reshape(Q, 1)
    out = []
    for q0 in range(0, Q, SCORE_MAX_PER_IMAGE):
        k = min(SCORE_MAX_PER_IMAGE, Q - q0)
        res = decoder.score_batch(word_map, encoder_out, tags, caps[q0:q0 + k].repeat(N, 1), caplens[q0:q0 + k].repeat(N, 1),
                                  per_image=k, temperature=temperature)
        out.append(res["sum_logp"].view(N, k))
    return torch.cat(out, dim=1) if out else torch.zeros(N, 0, device=encoder_out.device)
