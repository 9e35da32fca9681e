"""Synthetic-data training harness: the body of the reference's train step
(trains/attention_scn.py:204-258, and the pure_scn / pure_attention siblings) with real flags instead
of module-level globals; defaults equal the reference's constants (:25-61).

One call of ``TrainStep.step()`` =
    encoder fwd -> decoder fwd -> CrossEntropy over packed tokens + alpha_c * doubly-stochastic term
    -> zero_grad -> backward (+ bucketed RCCL all-reduce when world > 1) -> clamp +-5 -> Adam.
Data loading and the ``.item()`` metric syncs of the reference are outside the step.
Tags are a synthetic input (the tagger encoder is a "next" row of SURVEY.md 8f).

``TaggerTrainStep`` / ``validate_tagger`` are the fourth mode, trains/tagger.py:132-250: EncoderTagger under nn.BCELoss,
the same clamp and Adam, binary accuracy as the metric."""
import os

import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence

from models.decoders.attention_scn import AttentionSCN
from models.decoders.pure_scn import PureSCN
from models.decoders.pure_attention import PureAttention
from models.encoders.caption import EncoderCaption
from models.encoders.tagger import EncoderTagger
from scnattn import functional as SF
from scnattn.dp import GradReducer, broadcast_parameters
from utils.optimizer import FusedClampAdam

DEFAULTS = dict(emb_dim=512, attention_dim=512, decoder_dim=512, factored_dim=512, semantic_dim=1000,
                dropout=0.5, batch_size=32, encoder_lr=1e-4, decoder_lr=4e-4, grad_clip=5.0, alpha_c=1.0,
                vocab_size=10000, max_len=50, image_size=256)


def synthetic_batch(batch_size, vocab_size, max_len, image_size, semantic_dim, device, seed, ragged=False):
    """Seeded synthetic inputs of SURVEY.md 8d: images ~ N(0,1); captions <start> + words + <end>
    padded with 0 to max_len+2 (word-map convention: pad=0, words 1.., unk, start=V-2, end=V-1)."""
    g = torch.Generator().manual_seed(seed)
    L = max_len + 2
    imgs = torch.randn(batch_size, 3, image_size, image_size, generator=g)
    tags = torch.rand(batch_size, semantic_dim, generator=g)
    caps = torch.zeros(batch_size, L, dtype=torch.long)
    lens = torch.full((batch_size,), L, dtype=torch.long)
    if ragged:
        lens = torch.randint(7, L + 1, (batch_size,), generator=g)
    for b in range(batch_size):
        n = int(lens[b])
        caps[b, 0] = vocab_size - 2
        caps[b, 1:n - 1] = torch.randint(1, vocab_size - 3, (n - 2,), generator=g)
        caps[b, n - 1] = vocab_size - 1
    return imgs.to(device), tags.to(device), caps.to(device), lens.unsqueeze(1).to(device)


def build_decoder(kind, cfg):
    extra = {"encoder_dim": cfg["encoder_dim"]} if "encoder_dim" in cfg else {}      # default: the trunk's 2048 channels
    if kind == "attention_scn":
        return AttentionSCN(cfg["attention_dim"], cfg["emb_dim"], cfg["decoder_dim"], cfg["factored_dim"],
                            cfg["semantic_dim"], cfg["vocab_size"], dropout=cfg["dropout"], **extra)
    if kind == "pure_scn":
        return PureSCN(cfg["emb_dim"], cfg["decoder_dim"], cfg["factored_dim"], cfg["semantic_dim"],
                       cfg["vocab_size"], dropout=cfg["dropout"], **extra)
    if kind == "pure_attention":
        return PureAttention(cfg["attention_dim"], cfg["emb_dim"], cfg["decoder_dim"], cfg["vocab_size"],
                             dropout=cfg["dropout"], **extra)
    raise ValueError("Error model type not found!")


_DIAG_SLEEP_CYCLES = int(os.environ.get("SCNATTN_DIAG_BWD_HEADSTART_CYCLES", "0"))


class TrainStep:
    def __init__(self, kind="attention_scn", fine_tune_encoder=True, device="cuda", seed=1234, encoder=True,
                 bucket_mb=32, graph_encoder=False, tagger=False, force_reduce=False, encoder_dtype="f32",
                 decoder_dtype="f32", tagger_overlap=True,
                 fused_loss=True, pooled_attention=True, metrics=False, scheduled_sampling=0.0, ss_temperature=1.0,
                 ss_greedy=False, ss_seed=None, word_map=None, **overrides):
        self.cfg = dict(DEFAULTS)
        self.cfg.update(overrides)
        self.kind = kind
        # scheduled sampling (Bengio et al. 2015): with probability `scheduled_sampling` an input word of the decoder is the
        # model's own sample (decoder.mix_batch, at ss_temperature; ss_greedy: its arg-max) instead of the gold word; the
        # targets stay the gold words.  0.0: the step below does not touch any of it.  The coin and the noise are keyed by
        # (ss_seed, the number of steps so far); `last_mix` keeps inputs / replaced / n_replaced of the last mixed step on
        # the device.  word_map: where <start> sits (default: synthetic_batch's convention).
        from models.decoders._common import check_rollout_args
        check_rollout_args(1, ss_temperature, who="TrainStep")
        self.ss_temperature, self.ss_greedy = float(ss_temperature), bool(ss_greedy)
        self.ss_seed = int(seed if ss_seed is None else ss_seed)
        self.set_sampling_prob(scheduled_sampling)
        self.word_map = word_map if word_map is not None else SyntheticWordMap(self.cfg["vocab_size"])
        self.steps_done = 0
        self.last_mix = None
        self.fused_loss = fused_loss
        # metrics=True: the loss pass also counts the step's top-5 / top-1 hits (trains/attention_scn.py:255-257) and leaves
        # them in `last_metrics` on the device; the loss, its gradient and the update keep their bits.  topk_percent() syncs.
        if metrics and not fused_loss:
            raise ValueError("TrainStep: metrics=True rides in the fused loss pass (fused_loss=True)")
        self.metrics = metrics
        self.last_metrics = None     # (loss.detach(), hits int32 (2,) = [top-5 hits, top-1 hits], n_tokens)
        self.pooled_attention = pooled_attention   # attention on the trunk's 8x8 map instead of its 14x14 pooling
        # "bf16": the ResNet trunk runs under bf16 autocast (MIOpen bf16 MFMA convolutions, bf16 feature maps
        # through the fused BatchNorm kernels, fp32 master weights/statistics); the decoder stays fp32.
        # This is BASELINE config 5's mixed-precision flavour, NOT the headline fp32 metric.
        self.encoder_bf16 = encoder_dtype == "bf16"
        # decoder "bf16": the operands the recurrence streams every step (recurrent weights, att1, the trunk map) are
        # read as bf16 copies made once per call (include/scnattn.h, option "decoder_bf16"); fp32 accumulate, fp32
        # softmax / LSTM state / master weights / gradients.  A process-wide option of the library.
        self.tagger_overlap = tagger_overlap
        self.decoder_bf16 = decoder_dtype in ("bf16", "bf16mfma")
        if torch.device(device).type == "cuda":      # "bf16mfma": also round the activation rows of the per-step products
            SF.set_option("decoder_bf16", {"bf16": 1, "bf16mfma": 2}.get(decoder_dtype, 0))   # and use the bf16 MFMA
        self.device = torch.device(device)
        torch.manual_seed(seed)  # same seed on every rank => identical initial weights
        self.decoder = build_decoder(kind, self.cfg).to(self.device)
        self.encoder = None
        self.encoder_optimizer = None
        if encoder:
            # Measured on MI355X (tools/miopen_probe.py, ResNet-152 fwd+bwd, B=32 fp32): channels-last with
            # MIOpen's find API (cudnn.benchmark) under FAST find mode = 40 ms/step after a one-off ~55 s of
            # kernel compilation; NCHW immediate mode = 50 ms; channels-last immediate mode = 320 ms.
            torch.backends.cudnn.benchmark = True
            self.encoder = EncoderCaption(channels_last=True).to(self.device)
            self.encoder.fine_tune(fine_tune_encoder)
            if fine_tune_encoder:
                self.encoder_optimizer = FusedClampAdam(
                    filter(lambda p: p.requires_grad, self.encoder.parameters()), lr=self.cfg["encoder_lr"],
                    grad_clip=self.cfg["grad_clip"])
        # the reference's real step also runs a frozen tagger ResNet-152 in train() mode to produce the tags
        # (trains/attention_scn.py:79-81, 194, 214); the benchmark feeds synthetic tags unless tagger=True
        self.tagger = None
        if tagger:
            self.tagger = EncoderTagger(semantic_size=self.cfg["semantic_dim"], channels_last=True).to(self.device)
            self.tagger.fine_tune(False)
            self.tagger.train()
        self.decoder_optimizer = FusedClampAdam(filter(lambda p: p.requires_grad, self.decoder.parameters()),
                                                lr=self.cfg["decoder_lr"], grad_clip=self.cfg["grad_clip"])
        self.criterion = nn.CrossEntropyLoss().to(self.device)
        self.reducers = [GradReducer(self.decoder_optimizer.flat, max(bucket_mb << 20, 4096))]
        broadcast_parameters(self.decoder_optimizer.flat)
        if self.encoder_optimizer is not None:
            self.reducers.append(GradReducer(self.encoder_optimizer.flat, max(bucket_mb << 20, 4096)))
            broadcast_parameters(self.encoder_optimizer.flat)
        if force_reduce:          # diagnostics: exercise hooks + collectives with a single rank
            for r in self.reducers:
                r.enabled = True
        self.encoder_events = None   # bench.py: a list -> every step appends (fwd start, fwd end, bwd start, bwd end) HIP events
        self.decoder.train()
        self.graphed = False         # make_graphed_callables patches the module's forward in place: no extra keywords then
        self.encoder_call = self.encoder
        if self.encoder is not None:
            self.encoder.train()   # reference quirk Q3: BN uses batch statistics even when frozen
            if graph_encoder and self.device.type == "cuda":
                # Optional: capture the encoder's forward and backward as two HIP graphs (static shapes).
                # Measured on MI355X / ROCm 7.2: graph replay of the ~2000-node encoder is SLOWER than eager
                # launches (51.5 vs 45.2 ms per step), so it is off by default.
                cfg = self.cfg
                sample = torch.randn(cfg["batch_size"], 3, cfg["image_size"], cfg["image_size"], device=self.device)
                self.encoder_call = torch.cuda.make_graphed_callables(self.encoder, (sample,), num_warmup_iters=3)
                self.graphed = True

    def loss_fn(self, scores, caps_sorted, decode_lengths, alphas, dl_dev=None):
        """trains/attention_scn.py:222-236.  On the GPU: one fused forward/backward pair on the unpacked
        scores (csrc/loss.hip); `fused_loss=False` keeps the reference's op sequence (tests compare the two)."""
        if self.metrics:
            loss, hits, _ = SF.caption_loss_metrics(scores, caps_sorted, decode_lengths, alphas, self.cfg["alpha_c"], dl_dev, k=5)
            self.last_metrics = (loss.detach(), hits, sum(decode_lengths))
            return loss
        if self.fused_loss and scores.is_cuda:
            return SF.caption_loss(scores, caps_sorted, decode_lengths, alphas, self.cfg["alpha_c"], dl_dev)
        targets = caps_sorted[:, 1:]
        scores = pack_padded_sequence(scores, decode_lengths, batch_first=True).data
        targets = pack_padded_sequence(targets, decode_lengths, batch_first=True).data
        loss = self.criterion(scores, targets)
        if alphas is not None:
            loss = loss + self.cfg["alpha_c"] * ((1. - alphas.sum(dim=1)) ** 2).mean()
        return loss

    def set_sampling_prob(self, p):
        """the share of input words replaced by the model's own samples from the next step on (scheduled_sampling_prob
        gives the usual staircase); 0.0 is the plain teacher-forced step"""
        self.sampling_prob = SF.mix_prob(p, "TrainStep.set_sampling_prob")

    def step(self, imgs, tags, caps, caplens, encoder_out=None, prepool=None, drop_in=False, caplens_host=None):
        """`drop_in=True` is the reference's literal call sequence (trains/attention_scn.py:213-216):
        `encoder_out = encoder(imgs)` materialises the (B,14,14,2048) map, `decoder(encoder_out, ...)` receives only
        that tensor (and finds the trunk map EncoderCaption attached to it).  The default hands the trunk map over
        explicitly and skips the pooling kernel and its 51 MB write.  `caplens_host`: the caption lengths as a CPU tensor
        when the caller has them on the host anyway (a loader does): the decoder then needs no device synchronisation
        to learn its loop bounds (models/decoders/_common.py::sort_by_length); ignored for `drop_in`."""
        mixing = self.sampling_prob > 0.0
        if mixing and self.encoder is None and encoder_out is None:
            raise ValueError("TrainStep.step: scheduled sampling mixes on the dense encoder_out; a prepool map alone is not "
                             "enough (hand encoder_out over: the map attached to it is still used by forward)")
        tag_event = None
        if self.tagger is not None and self.tagger_overlap and imgs.is_cuda and self.encoder is not None:
            # The frozen tagger's forward pass shares nothing with the caption encoder's: it runs on the side stream
            # (scnattn/conv.py: a stream probed to be concurrent with this one) beside it; the decoder is the first
            # consumer of the tags and waits for them by event.
            from scnattn import conv as _conv
            main = torch.cuda.current_stream(imgs.device)
            side = _conv._side(imgs.device)
            side.fork(main, imgs)
            with torch.cuda.stream(side.stream), torch.no_grad(), \
                    torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.encoder_bf16):
                tags = self.tagger(imgs).float()
            tag_event = torch.cuda.Event()
            tag_event.record(side.stream)
        ev = None
        if self.encoder_events is not None and self.encoder is not None and imgs.is_cuda:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.encoder_bf16):
            if self.encoder is not None:
                if self.pooled_attention and not self.graphed and not drop_in and not mixing:
                    prepool = self.encoder(imgs, pooled=False)     # the decoder works on the 8x8 source map
                    encoder_out = None
                else:
                    encoder_out = self.encoder_call(imgs)
        if ev is not None:
            ev[1].record()
            feat = prepool if prepool is not None else encoder_out
            if feat.requires_grad:       # fires when the decoder's backward pass hands d(feature map) to the encoder's
                feat.register_hook(lambda g_, e=ev[2]: (e.record(), None)[1])
        if self.tagger is not None and tag_event is None:       # in line, after the caption encoder (no overlap)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.encoder_bf16):
                tags = self.tagger(imgs)
        if self.tagger is not None and tag_event is None:
            tags = tags.float()
        if tag_event is not None:
            torch.cuda.current_stream(imgs.device).wait_event(tag_event)
            tags.record_stream(torch.cuda.current_stream(imgs.device))
        inputs, pool_size = caps, self.encoder.enc_image_size if self.encoder is not None else 14
        if mixing:
            # the SCST step's feature route: the mix runs on the dense map, forward on the pre-pool map attached to it
            from models.decoders._common import attached_prepool
            with torch.no_grad():
                mix = self.decoder.mix_batch(self.word_map, encoder_out.detach(), tags, caps, caplens, self.sampling_prob,
                                             seed=self.ss_seed, draw=self.steps_done, temperature=self.ss_temperature,
                                             greedy=self.ss_greedy)
            inputs = mix["inputs"]
            self.last_mix = dict(inputs=inputs, replaced=mix["replaced"], n_replaced=mix["n_replaced"])
            prepool = attached_prepool(encoder_out)
            if self.encoder is None:
                pool_size = encoder_out.shape[1]
            if prepool is not None:
                encoder_out = None
        if self.kind == "attention_scn":
            scores, caps_sorted, decode_lengths, alphas, sort_ind = self.decoder(
                encoder_out, tags, inputs, caplens, prepool=prepool, pool_size=pool_size,
                caplens_host=None if drop_in else caplens_host)
        elif self.kind == "pure_scn":
            scores, caps_sorted, decode_lengths, sort_ind = self.decoder(
                encoder_out, tags, inputs, caplens, prepool=prepool, pool_size=pool_size,
                caplens_host=None if drop_in else caplens_host)
            alphas = None
        else:
            scores, caps_sorted, decode_lengths, alphas, sort_ind = self.decoder(
                encoder_out, inputs, caplens, prepool=prepool, pool_size=pool_size,
                caplens_host=None if drop_in else caplens_host)
        if mixing:      # the decoder read the mixed words; the loss (and the metrics) are taken against the gold ones
            assert torch.equal(caps_sorted, inputs[sort_ind]), "forward did not return the captions it was given"
            caps_sorted = caps[sort_ind]
        self.steps_done += 1
        dl_dev = (caplens.reshape(-1)[sort_ind] - 1).to(torch.int32) if self.fused_loss else None
        loss = self.loss_fn(scores, caps_sorted, decode_lengths, alphas, dl_dev)
        self.decoder_optimizer.zero_grad()
        if self.encoder_optimizer is not None:
            self.encoder_optimizer.zero_grad()
        for r in self.reducers:
            r.reset()
        if _DIAG_SLEEP_CYCLES:      # diagnostics (tools/README.md): keep the GPU busy so that the host enqueues backward() ahead of it
            torch.cuda._sleep(_DIAG_SLEEP_CYCLES)
        loss.backward()
        if ev is not None:
            from scnattn import conv as _conv
            _conv.join_side_streams()       # the encoder's weight gradients on the side stream belong to its backward pass
            ev[3].record()
            self.encoder_events.append(ev)
        scale = 1.0
        for r in self.reducers:
            scale = r.finish()
        self.decoder_optimizer.step(scale)
        if self.encoder_optimizer is not None:
            self.encoder_optimizer.step(scale)
        return loss

    def topk_percent(self):
        """The last step's top-5 accuracy in percent (metrics=True), the reference's `accuracy(scores, targets, 5)`;
        the one place that waits for the device."""
        if self.last_metrics is None:
            raise RuntimeError("TrainStep.topk_percent: no step has run with metrics=True")
        return topk_percent(self.last_metrics[1], self.last_metrics[2])


def scheduled_sampling_prob(epoch, start=0, every=5, increase=0.05, max_prob=0.25):
    """The usual staircase of the replacement probability (a host function): 0 before epoch `start`, then `increase` more
    every `every` epochs, capped at max_prob: min(max_prob, increase * ((epoch - start) // every + 1))."""
    if every < 1:
        raise ValueError("scheduled_sampling_prob: every must be at least 1 (got %r)" % (every,))
    if epoch < start:
        return 0.0
    return min(float(max_prob), increase * ((epoch - start) // every + 1))


class SyntheticWordMap:
    """The word map of synthetic_batch without its V entries: <pad> = 0, <unk> = V-3, <start> = V-2, <end> = V-1"""

    def __init__(self, vocab_size):
        self.ids = {"<pad>": 0, "<unk>": vocab_size - 3, "<start>": vocab_size - 2, "<end>": vocab_size - 1}
        self.vocab_size = vocab_size

    def __len__(self):
        return self.vocab_size

    def __getitem__(self, word):
        return self.ids[word]


class SCSTTrainStep(TrainStep):
    """Self-critical sequence training (Rennie et al. 2017) on the TrainStep's models and optimizers: the decoder is
    rewarded with the CIDEr-D of the captions it samples itself.  One ``step(imgs, tags, image_index)`` =
        encoder fwd (and the tagger's tags, when there is a tagger)
        -> under no_grad one rollout of K = samples (+ 1 with baseline="greedy": slot 0 is the arg-max caption) captions
           per image on the device (decoder.rollout_batch), at `temperature`
        -> rewards = scorer.score_rows(image of each row, the captions)          CIDEr-D against that image's references
        -> advantage = reward - baseline:  "greedy": the reward of the image's arg-max caption;
                                           "mean":   the mean reward of the image's OTHER samples (samples >= 2)
        -> the teacher-forced decoder.forward on the sampled rows (encoder rows repeated per sample; the attached
           pre-pool map when there is one), SF.caption_loss_weighted with row_weight = advantage (fp32, a constant)
        -> backward, clamp + Adam as in TrainStep.
    The rollout runs WITHOUT dropout, as the search does; the teacher-forced pass runs in whatever mode the decoder
    module is in (train() after construction: dropout as configured), so its log-likelihood is not bit for bit the
    rollout's.  Every step draws fresh noise: the rollout's `draw` is the number of steps taken so far, `rollout_seed`
    (default: `seed`) stays.  The arg-max rows get no gradient (their advantage is 0 by construction) and are left out of
    the teacher-forced pass.  `last` keeps what the step did, on the device: caps / caplens / advantage / reward of the
    trained rows (n*samples + s), reward_all (N, K), mean_reward / mean_baseline / mean_advantage over the trained rows
    as 0-dim tensors, flag (a token outside CIDEr-D's range).  Nothing of it is downloaded; the step waits for the device
    only in the rollout's counter polls and where decoder.forward learns its loop bounds (the caption lengths)."""

    def __init__(self, scorer=None, samples=5, baseline="greedy", temperature=1.0, word_map=None, rollout_seed=None,
                 seed=1234, **kw):
        if baseline not in ("greedy", "mean"):
            raise ValueError("SCSTTrainStep: baseline must be 'greedy' or 'mean' (got %r)" % (baseline,))
        if baseline == "mean" and int(samples) < 2:
            raise ValueError("SCSTTrainStep: baseline='mean' is the mean of an image's other samples and needs samples >= 2")
        from models.decoders._common import check_rollout_args
        self.K = check_rollout_args(samples, temperature, baseline == "greedy", who="SCSTTrainStep")
        if scorer is None or not hasattr(scorer, "score_rows"):
            raise ValueError("SCSTTrainStep: scorer must be a CaptionScorer (score_rows gives the rewards)")
        if kw.get("metrics"):
            raise ValueError("SCSTTrainStep: metrics=True belongs to the cross-entropy step")
        if kw.get("scheduled_sampling"):
            raise ValueError("SCSTTrainStep: scheduled_sampling belongs to the cross-entropy step (this one already trains on "
                             "its own samples)")
        super().__init__(seed=seed, **kw)
        self.scorer, self.samples, self.baseline, self.temperature = scorer, int(samples), baseline, float(temperature)
        self.word_map = word_map if word_map is not None else SyntheticWordMap(self.cfg["vocab_size"])
        if len(self.word_map) != self.cfg["vocab_size"]:
            raise ValueError("SCSTTrainStep: word_map has %d entries, vocab_size is %d" % (len(self.word_map), self.cfg["vocab_size"]))
        self.rollout_seed = int(seed if rollout_seed is None else rollout_seed)
        self.draw = 0
        self.last = None

    def step(self, imgs, tags, image_index, encoder_out=None):
        """imgs (N, 3, H, W) (ignored without an encoder: then encoder_out (N, h, w, E) is given), tags (N, S) (replaced
        by the tagger's when there is one), image_index (N,): the scorer's image behind each batch row."""
        N = imgs.shape[0] if encoder_out is None else encoder_out.shape[0]
        image_index = torch.as_tensor(image_index)
        if image_index.dim() != 1 or image_index.numel() != N:
            raise ValueError("SCSTTrainStep.step: image_index must name one image per batch row (%d), got %s"
                             % (N, tuple(image_index.shape)))
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.encoder_bf16):
            if self.encoder is not None:
                encoder_out = self.encoder_call(imgs)
            if self.tagger is not None:
                with torch.no_grad():
                    tags = self.tagger(imgs)
        if encoder_out is None:
            raise RuntimeError("SCSTTrainStep.step: no encoder and no encoder_out")
        if self.tagger is not None:
            tags = tags.float()
        S, K, greedy = self.samples, self.K, self.baseline == "greedy"
        from models.decoders._common import attached_prepool
        from utils.token import start_token, end_token, padding_token
        pre = attached_prepool(encoder_out)
        with torch.no_grad():
            caps, caplens, _ = self.decoder.rollout_batch(self.word_map, encoder_out.detach(), tags, samples=S,
                                                          seed=self.rollout_seed, draw=self.draw,
                                                          temperature=self.temperature, greedy_first=greedy)
            self.draw += 1
            dev = caps.device
            rows_image = image_index.to(dev).repeat_interleave(K)
            skip = tuple(self.word_map[w] for w in (start_token, end_token, padding_token))
            reward, flag = self.scorer.score_rows(rows_image, caps[:, 1:].to(torch.int32),
                                                  (caplens.reshape(-1) - 1).to(torch.int32), skip_hyp=skip)
            reward_all = reward.view(N, K)
            sampled = reward_all[:, 1:] if greedy else reward_all
            if greedy:
                base = reward_all[:, :1].expand(N, S)
            else:
                base = (sampled.sum(dim=1, keepdim=True) - sampled) / (S - 1)
            advantage = (sampled - base).reshape(-1)
            keep = torch.arange(N * K, device=dev).view(N, K)[:, K - S:].reshape(-1)      # the sampled rows n*K + j
            caps_s, caplens_s = caps[keep], caplens[keep]
        rep = lambda x: None if x is None else x.repeat_interleave(S, dim=0)      # noqa: E731
        enc_rep, pre_rep = (None, rep(pre)) if pre is not None else (rep(encoder_out), None)
        pool = self.encoder.enc_image_size if self.encoder is not None else encoder_out.shape[1]
        if self.kind == "attention_scn":
            scores, caps_sorted, decode_lengths, alphas, sort_ind = self.decoder(enc_rep, rep(tags), caps_s, caplens_s,
                                                                                 prepool=pre_rep, pool_size=pool)
        elif self.kind == "pure_scn":
            scores, caps_sorted, decode_lengths, sort_ind = self.decoder(enc_rep, rep(tags), caps_s, caplens_s,
                                                                         prepool=pre_rep, pool_size=pool)
            alphas = None
        else:
            scores, caps_sorted, decode_lengths, alphas, sort_ind = self.decoder(enc_rep, caps_s, caplens_s, prepool=pre_rep,
                                                                                 pool_size=pool)
        dl_dev = (caplens_s.reshape(-1)[sort_ind] - 1).to(torch.int32)
        weight = advantage[sort_ind].to(torch.float32)
        loss = SF.caption_loss_weighted(scores, caps_sorted, decode_lengths, weight, alphas, self.cfg["alpha_c"], dl_dev)
        self.last = dict(caps=caps_s, caplens=caplens_s, advantage=advantage, reward=sampled.reshape(-1),
                         reward_all=reward_all, mean_reward=sampled.mean(), mean_baseline=base.mean(),
                         mean_advantage=advantage.mean(), flag=flag, loss=loss.detach())
        self.decoder_optimizer.zero_grad()
        if self.encoder_optimizer is not None:
            self.encoder_optimizer.zero_grad()
        for r in self.reducers:
            r.reset()
        loss.backward()
        scale = 1.0
        for r in self.reducers:
            scale = r.finish()
        self.decoder_optimizer.step(scale)
        if self.encoder_optimizer is not None:
            self.encoder_optimizer.step(scale)
        return loss


def topk_percent(hits, n_tokens):
    """utils/metric.py::accuracy from the hit count of SF.caption_loss_metrics: `correct_total.item() * (100.0 / batch_size)`"""
    return float(int(hits[0])) * (100.0 / n_tokens)


def validate(batches, encoder, encoder_tagger, decoder, criterion, word_map, alpha_c=1.0, fused=False, device_bleu=False):
    """The reference's validate() (trains/attention_scn.py:274-385): eval-mode forward under no_grad,
    loss / top-5 accuracy bookkeeping, references and arg-max hypotheses, corpus BLEU-4.
    `batches` yields (imgs, caps, caplens, allcaps) already on the device; `encoder_tagger` may be a
    callable returning tags or None when the batch tuple carries tags in place of images for it.
    `fused=True`: loss, top-5 and hypotheses from one pass over the scores (_validate_fused), any of the three decoders;
    with `device_bleu=True` as well, BLEU's n-gram counting runs on the device too and only ten integers per pass come down
    for it (the same BLEU-4, bit for bit)."""
    if device_bleu and not fused:
        raise ValueError("validate: device_bleu=True needs fused=True")
    if fused:
        return _validate_fused(batches, encoder, encoder_tagger, decoder, word_map, alpha_c, device_bleu)
    from utils.metric import AverageMeter, accuracy, corpus_bleu
    decoder.eval()
    encoder.eval()
    if hasattr(encoder_tagger, "eval"):
        encoder_tagger.eval()
    losses, top5accs = AverageMeter(), AverageMeter()
    references, hypotheses = [], []
    skip = {word_map['<start>'], word_map['<pad>']}
    with torch.no_grad():
        for imgs, caps, caplens, allcaps in batches:
            encoder_out = encoder(imgs)
            tags = encoder_tagger(imgs)
            scores, caps_sorted, decode_lengths, alphas, sort_ind = decoder(encoder_out, tags, caps, caplens)
            targets = caps_sorted[:, 1:]
            scores_copy = scores.clone()
            scores_p = pack_padded_sequence(scores, decode_lengths, batch_first=True).data
            targets_p = pack_padded_sequence(targets, decode_lengths, batch_first=True).data
            loss = criterion(scores_p, targets_p) + alpha_c * ((1. - alphas.sum(dim=1)) ** 2).mean()
            losses.update(loss.item(), sum(decode_lengths))
            top5accs.update(accuracy(scores_p, targets_p, 5), sum(decode_lengths))
            allcaps = allcaps[sort_ind]
            for j in range(allcaps.shape[0]):
                references.append([[w for w in c if w not in skip] for c in allcaps[j].tolist()])
            preds = torch.max(scores_copy, dim=2)[1].tolist()
            hypotheses.extend(p[:decode_lengths[j]] for j, p in enumerate(preds))
    assert len(references) == len(hypotheses)
    return corpus_bleu(references, hypotheses), losses.avg, top5accs.avg


def _validate_fused(batches, encoder, encoder_tagger, decoder, word_map, alpha_c, device_bleu=False):
    """validate() on SF.caption_loss_metrics: per batch the decoder's forward and one loss pass that also yields the top-5
    hit count and the arg-max tokens; no clone, no packed copies, no topk, no synchronisation of its own.  What a batch
    leaves stays on the device -- loss bits, hits and preds in one int32 vector, allcaps[sort_ind] -- and comes down in two
    copies after the last batch; the AverageMeter arithmetic is then replayed in the reference's order, so the averages are
    formed as the eager path forms them.  The decoder's kind decides its call, as in TrainStep.step().
    device_bleu=True: preds and allcaps[sort_ind] are not downloaded at all.  Per batch scnattn.textmetrics.ngram_stats counts
    the clipped matches on them (hypothesis length = decode_lengths, references without <start>/<pad>), the ten corpus
    integers of utils.metric.bleu_from_totals accumulate on the device, and the one download holds them, the loss bits and the
    hit counts; corpus_bleu ends in that same bleu_from_totals on the same integers."""
    from utils.metric import AverageMeter, bleu_from_totals, corpus_bleu
    from scnattn import textmetrics as TM
    decoder.eval()
    encoder.eval()
    if hasattr(encoder_tagger, "eval"):
        encoder_tagger.eval()
    skip = {word_map['<start>'], word_map['<pad>']}
    words, caps_dev, shapes = [], [], []
    totals = None
    with torch.no_grad():
        for imgs, caps, caplens, allcaps in batches:
            encoder_out = encoder(imgs)
            alphas = None
            if isinstance(decoder, PureAttention):
                scores, caps_sorted, decode_lengths, alphas, sort_ind = decoder(encoder_out, caps, caplens)
            elif isinstance(decoder, PureSCN):
                scores, caps_sorted, decode_lengths, sort_ind = decoder(encoder_out, encoder_tagger(imgs), caps, caplens)
            else:
                scores, caps_sorted, decode_lengths, alphas, sort_ind = decoder(encoder_out, encoder_tagger(imgs), caps, caplens)
            dl_dev = (caplens.reshape(-1)[sort_ind] - 1).to(torch.int32)
            loss, hits, preds = SF.caption_loss_metrics(scores, caps_sorted, decode_lengths, alphas, alpha_c, dl_dev, k=5)
            allcaps = allcaps[sort_ind]
            if device_bleu:
                refs = allcaps.to(torch.int32).contiguous()
                ref_len = torch.full(refs.shape[:2], refs.shape[2], dtype=torch.int32, device=refs.device)
                stats = TM.ngram_stats(preds.contiguous(), dl_dev.contiguous(), refs, ref_len, (), sorted(skip))
                batch_totals = TM.nltk_totals(stats)
                totals = batch_totals if totals is None else totals + batch_totals
                words.append(torch.cat([loss.reshape(1).view(torch.int32), hits]))
                shapes.append(list(decode_lengths))
                continue
            words.append(torch.cat([loss.reshape(1).view(torch.int32), hits, preds.reshape(-1)]))
            caps_dev.append(allcaps.reshape(-1))
            shapes.append((tuple(preds.shape), tuple(allcaps.shape), list(decode_lengths)))
    losses, top5accs = AverageMeter(), AverageMeter()
    if device_bleu:
        if not shapes:
            return corpus_bleu([], []), losses.avg, top5accs.avg
        # ten int64 as twenty int32 words behind the per-batch (loss bits, hits, hits1): one copy
        words = torch.cat(words + [totals.view(torch.int32)]).cpu()
        for i, decode_lengths in enumerate(shapes):
            n = sum(decode_lengths)
            losses.update(words[3 * i:3 * i + 1].view(torch.float32).item(), n)
            top5accs.update(topk_percent(words[3 * i + 1:3 * i + 3], n), n)
        tot = words[3 * len(shapes):].clone().view(torch.int64).tolist()
        return bleu_from_totals(tot[0:4], tot[4:8], tot[8], tot[9]), losses.avg, top5accs.avg
    references, hypotheses = [], []
    if shapes:
        words, caps_host = torch.cat(words).cpu(), torch.cat(caps_dev).cpu()
    w = c = 0
    for (B, T), cshape, decode_lengths in shapes:
        n = sum(decode_lengths)
        losses.update(words[w:w + 1].view(torch.float32).item(), n)
        top5accs.update(topk_percent(words[w + 1:w + 3], n), n)
        preds = words[w + 3:w + 3 + B * T].view(B, T).tolist()
        w += 3 + B * T
        ncap = cshape[0] * cshape[1] * cshape[2]
        allcaps = caps_host[c:c + ncap].view(cshape)
        c += ncap
        for j in range(cshape[0]):
            references.append([[x for x in cap if x not in skip] for cap in allcaps[j].tolist()])
        hypotheses.extend(p[:decode_lengths[j]] for j, p in enumerate(preds))
    assert len(references) == len(hypotheses)
    return corpus_bleu(references, hypotheses), losses.avg, top5accs.avg


def evaluate_captions(batches, encoder, encoder_tagger, decoder, word_map, beam_size=5, search_options=None):
    """The reference's eval_caption.py:95-165, batched: per batch (imgs, allcaps) on the device both trunks in eval mode, the
    batched beam search (sample_batch), then BLEU-1..4, ROUGE-L and CIDEr-D of the whole split from ONE
    scnattn.textmetrics.CaptionScorer.score with <start>, <end> and <pad> dropped on both sides inside the kernels -- what the
    reference strips in Python before it hands words to NLGEval.  The references never leave the device; each batch uploads
    its hypotheses once.  Returns the scorer's dict (NLGEval's key names, plus 'bleu4_nltk'; no METEOR); writing the JSON files
    of the reference is the caller's business.  `search_options`: a models.decoders.SearchOptions handed to sample_batch
    (None: the reference's search)."""
    import torch.nn.functional as F
    from scnattn import textmetrics as TM
    kw = {} if search_options is None else {"options": search_options}
    decoder.eval()
    encoder.eval()
    if hasattr(encoder_tagger, "eval"):
        encoder_tagger.eval()
    special = sorted({word_map['<start>'], word_map['<end>'], word_map['<pad>']})
    hyps, hyp_lens, refs, ref_lens = [], [], [], []
    with torch.no_grad():
        for imgs, allcaps in batches:
            encoder_out = encoder(imgs)
            if isinstance(decoder, PureAttention) or not getattr(decoder, "needs_tags", True):     # or an ensemble of them
                results = decoder.sample_batch(beam_size, word_map, encoder_out, **kw)
            else:
                results = decoder.sample_batch(beam_size, word_map, encoder_out, encoder_tagger(imgs), **kw)
            seqs = [r[0] if isinstance(r, tuple) else r for r in results]
            tok, n = TM.pack_captions(seqs, allcaps.device)
            hyps.append(tok)
            hyp_lens.append(n)
            ref, n = TM.pack_references(allcaps, allcaps.device)
            refs.append(ref)
            ref_lens.append(n)
    if not hyps:
        raise ValueError("evaluate_captions: no batches")
    Lh, Lr = max(t.shape[1] for t in hyps), max(t.shape[2] for t in refs)
    hyp = torch.cat([F.pad(t, (0, Lh - t.shape[1])) for t in hyps])
    ref = torch.cat([F.pad(t, (0, Lr - t.shape[2])) for t in refs])
    scorer = TM.CaptionScorer((ref, torch.cat(ref_lens)), skip_ref=special, device=ref.device)
    return scorer.score((hyp, torch.cat(hyp_lens)), skip_hyp=special)


def evaluate_likelihood(encoder, decoder, loader, word_map, tagger=None):
    """How likely does the model find the split's own references: corpus perplexity and teacher-forced accuracy from
    `decoder.score_batch` (the whole scoring on the device).  `loader` yields (imgs, allcaps) or (imgs, allcaps, allcaplens):
    allcaps (N, per_image, L) int holds ALL references of every image (5 in the reference's data), each <start>, the words,
    <end>, <pad> ...; allcaplens (N, per_image) counts <start> and <end> (absent: up to and including the first <end>, else
    every token before the padding); a length <= 1 marks a missing reference.  More than 8 references per image are scored
    8 at a time over the same encoder output.  ONE download per batch: the bits of logp beside rank and n_tokens.
    Returns dict:
        perplexity   exp(-sum logp / sum n_tokens), summed in fp64 from the fp32 logp records
        top1, top5   percent of the reference tokens that the model ranks first / among its first five (rank < 1, < 5)
        mean_rank    the mean of rank over the reference tokens (0: every token was the model's own choice)
        n_tokens, n_captions, sum_logp   the totals behind them
    top1, top5 and mean_rank are None under an ensemble of several members, whose score_batch has no rank."""
    import math
    decoder.eval()
    encoder.eval()
    if hasattr(tagger, "eval"):
        tagger.eval()
    needs_tags = not isinstance(decoder, PureAttention) and getattr(decoder, "needs_tags", True)
    if needs_tags and tagger is None:
        raise ValueError("evaluate_likelihood: a %s decoder needs a tagger" % type(decoder).__name__)
    end, pad = word_map['<end>'], word_map['<pad>']
    total_lp, n_tok, n_cap, top1, top5, rank_sum, ranked = 0.0, 0, 0, 0, 0, 0, True
    with torch.no_grad():
        for batch in loader:
            imgs, allcaps = batch[0], batch[1]
            N, Q, L = allcaps.shape
            if len(batch) > 2:
                lens = batch[2].reshape(N, Q).to(torch.int64)
            else:
                is_end = allcaps == end
                first_end = torch.where(is_end.any(2), is_end.to(torch.int64).argmax(2) + 1, (allcaps != pad).sum(2))
                lens = first_end
            encoder_out = encoder(imgs)
            tags = tagger(imgs) if needs_tags else None
            parts = []
            for q0 in range(0, Q, 8):
                k = min(8, Q - q0)
                res = decoder.score_batch(word_map, encoder_out, tags, allcaps[:, q0:q0 + k].reshape(N * k, L),
                                          lens[:, q0:q0 + k].reshape(N * k, 1), per_image=k)
                ranked = ranked and res["rank"] is not None
                rank = res["rank"] if res["rank"] is not None else torch.zeros_like(res["logp"], dtype=torch.int32)
                parts.append(torch.cat([res["logp"].view(torch.int32), rank, res["n_tokens"].unsqueeze(1)], dim=1))
            host = torch.cat(parts).cpu()                   # the one download of the batch
            nt = host[:, -1].to(torch.int64)
            given = torch.arange(L - 1).unsqueeze(0) < nt.unsqueeze(1)
            logp, rank = host[:, :L - 1].view(torch.float32), host[:, L - 1:2 * (L - 1)]
            total_lp += float(logp.double()[given].sum())
            n_tok += int(nt.sum())
            n_cap += int((nt > 0).sum())
            top1 += int((rank[given] < 1).sum())
            top5 += int((rank[given] < 5).sum())
            rank_sum += int(rank[given].to(torch.int64).sum())
    if n_tok == 0:
        raise ValueError("evaluate_likelihood: no reference tokens")
    return {"perplexity": math.exp(-total_lp / n_tok), "top1": 100.0 * top1 / n_tok if ranked else None,
            "top5": 100.0 * top5 / n_tok if ranked else None, "mean_rank": rank_sum / n_tok if ranked else None,
            "n_tokens": n_tok, "n_captions": n_cap, "sum_logp": total_lp}


TAGGER_DEFAULTS = dict(semantic_size=1000, dropout=0.15, batch_size=32, encoder_lr=1e-4, grad_clip=5.0, image_size=256)


class TaggerTrainStep:
    """The body of the reference's tagger loop (trains/tagger.py:153-173) with its constants (:24-46) as defaults.

    One call of ``step(imgs, tags)`` =
        trunk fwd -> pool, dropout mask, Linear, Sigmoid, BCELoss and agreement count (EncoderTagger.tag_loss)
        -> zero_grad -> backward (+ bucketed all-reduce when world > 1) -> clamp +-5 -> Adam
    and returns (loss, agree) on the device: `loss.item()` and `agree / tags.numel() * 100` (binary_accuracy) are the
    caller's syncs, as in TrainStep.  `encoder`: an EncoderTagger to train instead of a fresh one (a checkpoint's).
    `loss`: a scnattn.functional.TagLoss in the place of BCELoss (positive weights, focal, asymmetric: the answers to rare
    tags); None is the reference's loss, bit for bit.  `prior_bias_from`: an [N, S] target matrix whose tag frequencies
    initialise linear.bias (scnattn.functional.prior_bias) -- for an untrained head; it overwrites the bias of `encoder`."""

    def __init__(self, fine_tune_encoder=False, device="cuda", seed=1234, encoder_dtype="f32", bucket_mb=32,
                 force_reduce=False, encoder=None, loss=None, prior_bias_from=None, **overrides):
        unknown = set(overrides) - set(TAGGER_DEFAULTS)
        if unknown:
            raise TypeError("TaggerTrainStep: unknown setting(s) %s" % ", ".join(sorted(unknown)))
        self.cfg = dict(TAGGER_DEFAULTS)
        self.cfg.update(overrides)
        self.device = torch.device(device)
        self.encoder_bf16 = encoder_dtype == "bf16"       # the trunk under bf16 autocast; head, loss and master weights fp32
        self.fine_tune_encoder = fine_tune_encoder
        torch.manual_seed(seed)  # same seed on every rank => identical initial weights
        if encoder is None:
            encoder = EncoderTagger(semantic_size=self.cfg["semantic_size"], dropout=self.cfg["dropout"], channels_last=True)
        self.encoder = encoder.to(self.device)
        self.encoder.fine_tune(fine_tune_encoder)
        if loss is not None and not isinstance(loss, SF.TagLoss):
            raise TypeError("TaggerTrainStep: loss must be a scnattn.functional.TagLoss or None")
        self.loss = loss
        if prior_bias_from is not None:
            with torch.no_grad():
                self.encoder.linear.bias.copy_(SF.prior_bias(prior_bias_from).to(self.device))
        self.optimizer = FusedClampAdam(filter(lambda p: p.requires_grad, self.encoder.parameters()),
                                        lr=self.cfg["encoder_lr"], grad_clip=self.cfg["grad_clip"])
        self.reducers = [GradReducer(self.optimizer.flat, max(bucket_mb << 20, 4096))]
        broadcast_parameters(self.optimizer.flat)
        if force_reduce:          # diagnostics: exercise hooks + collectives with a single rank
            for r in self.reducers:
                r.enabled = True
        self.encoder.train()
        self.probs = None         # the last step's tag probabilities (what the reference calls `scores`)

    def step(self, imgs, tags):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.encoder_bf16):
            self.probs, loss, agree = self.encoder.tag_loss(imgs, tags, loss=self.loss)
        self.optimizer.zero_grad()
        for r in self.reducers:
            r.reset()
        loss.backward()
        if self.fine_tune_encoder:
            from scnattn import conv as _conv
            _conv.join_side_streams()       # the trunk's weight gradients on the side stream belong to its backward pass
        scale = 1.0
        for r in self.reducers:
            scale = r.finish()
        self.optimizer.step(scale)
        return loss, agree


def validate_tagger(batches, encoder, losses=None, scorer=None, loss=None):
    """The reference's tagger validate() (trains/tagger.py:195-250): eval mode, no_grad, one unweighted `update(val)` per
    batch for loss and accuracy (= agree / (B * S) * 100, binary_accuracy); returns the accuracy meter.  `batches` yields
    (imgs, tags) on the device; `losses`: an AverageMeter that receives the per-batch losses.  `scorer`: a
    scnattn.tagmetrics.TagScorer that receives every batch's probabilities and tags (one launch each, no synchronisation);
    its result() then holds tag mAP, precision / recall at k and per-tag F1 of the pass.  `loss`: the TagLoss the tagger is
    trained under, so that `losses` reports the validation loss of that loss; the accuracy does not depend on it."""
    from utils.metric import AverageMeter
    encoder.eval()
    losses = AverageMeter() if losses is None else losses
    accs = AverageMeter()
    with torch.no_grad():
        for imgs, tags in batches:
            probs, batch_loss, agree = encoder.tag_loss(imgs, tags, loss=loss)
            if scorer is not None:
                scorer.update(probs, tags)
            losses.update(batch_loss.item())
            accs.update(agree.item() / tags.numel() * 100.0)
    return accs


def evaluate_tagger(batches, encoder, ks=(1, 5, 10, 20), thresholds=(0.5,), capacity=None):
    """The reference's eval_tagger.py at any batch size, with the measures binary_accuracy cannot give: eval mode, no_grad,
    `encoder(imgs)` of every batch into a TagScorer, one download at the end.  `batches` yields (imgs, tags) on the device.
    `capacity`: the number of images (e.g. len(dataset)), so that a loader can be streamed; without it `batches` is made a
    list first and counted.  Returns TagScorer.result()."""
    from scnattn.tagmetrics import TagScorer
    if capacity is None:
        batches = list(batches)
        capacity = sum(int(tags.shape[0]) for _, tags in batches)
    encoder.eval()
    scorer = None
    with torch.no_grad():
        for imgs, tags in batches:
            if scorer is None:
                scorer = TagScorer(encoder.semantic_size, capacity, ks=ks, thresholds=thresholds, device=tags.device)
            scorer.update(encoder(imgs), tags)
    if scorer is None:
        raise ValueError("evaluate_tagger: no batches")
    return scorer.result()
