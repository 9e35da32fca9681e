"""Self-critical training on the device: what a rollout and a whole SCST step cost.

    python tools/scst_bench.py [--images 32] [--repeats 7] [--out profiles/scst_bench.txt]

One process, AttentionSCN at the train step's widths (P=196, E=2048, A=D=F=M=512, S=1000, V=10000) with random weights (one
seed), the logits sharpened and the <end> bias raised as in tools/beam_bench.py.  At temperature 1 nearly every sampled row
still runs to the step limit with these weights (the lines report mean_length / longest), so the rollout figures are those of
full-length captions: the most a rollout can cost.
After one warm-up pass each measurement is the median of `--repeats` passes, each bracketed by device events (the rollouts
synchronise inside, so the events see host time too).  One JSON line per measurement:

  rollout        rollout_batch on `--images` images with 1, 5 and 6 slots (6 = 5 samples + the arg-max slot), captions/s
  search         sample_batch with beam 1 and 5 on the same images: the search this build had before the rollout
  module_loop    the same sampling done with the module path: one decode step of the nn.Module per time step over all
                 rows, torch.multinomial for the pick, the open-row test on the host (one .tolist() per step), 5 slots
  scst_step      SCSTTrainStep.step (5 samples, greedy baseline) against TrainStep.step on the same decoder, decoder only
                 (the encoder output is an input: the encoder costs the same in both), B = `--images`

Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "indonesian-image-captioning_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def word_map(V):
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    for i in range(1, V - 3):
        wm["w%d" % i] = i
    return wm


def timed(run, repeats):
    import torch
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def module_loop(m, wm, enc, tags, K, max_steps=51):
    """K samples per image through the module's own step, torch.multinomial per step, the stop test on the host"""
    import torch
    from scnattn import functional as SF
    N, hh, ww, E = enc.shape
    e = enc.reshape(N, hh * ww, E).repeat_interleave(K, 0)
    tg = tags.repeat_interleave(K, 0)
    R = N * K
    h, c = m.init_hidden_state(e)
    prev = torch.full((R,), wm["<start>"], dtype=torch.long, device=enc.device)
    open_ = torch.ones(R, dtype=torch.bool, device=enc.device)
    out = []
    for _ in range(max_steps):
        emb = m.embedding(prev)
        awe, _ = m.attention(e, h)
        gate = torch.sigmoid(SF.linear(h, m.f_beta.weight, m.f_beta.bias))
        h, c = m.decode_step(torch.cat([emb, gate * awe], dim=1), tg, (h, c))
        logits = SF.linear(h, m.fc.weight, m.fc.bias)
        prev = torch.multinomial(torch.softmax(logits, dim=1), 1).squeeze(1)
        out.append(prev)
        open_ &= prev != wm["<end>"]
        if not any(open_.tolist()):
            break
    return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sharpen", type=float, default=10.0)
    ap.add_argument("--end-bias", type=float, default=2.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    from trains.harness import SCSTTrainStep, TrainStep, synthetic_batch
    from scnattn import textmetrics as TM
    assert torch.cuda.is_available(), "scst_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    V, E, S, N = args.vocab, 2048, 1000, args.images
    wm = word_map(V)
    g = torch.Generator().manual_seed(args.seed)
    refs = [[[V - 2] + torch.randint(1, V - 3, (int(torch.randint(8, 20, (1,), generator=g)),), generator=g).tolist() + [V - 1]
             for _ in range(5)] for _ in range(N)]
    scorer = TM.CaptionScorer(refs, skip_ref=(V - 2, V - 1, 0), device=dev)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def sharpen(m):
        with torch.no_grad():
            m.fc.weight.mul_(args.sharpen)
            m.fc.bias[V - 1] += args.end_bias

    ts = SCSTTrainStep(scorer=scorer, samples=5, baseline="greedy", word_map=wm, device=dev, encoder=False, seed=args.seed,
                       vocab_size=V, dropout=0.0)
    sharpen(ts.decoder)
    m = ts.decoder
    enc = torch.rand(N, 14, 14, E, generator=g).to(dev)
    tags = torch.rand(N, S, generator=g).to(dev)
    draw = [0]
    for K, greedy in ((1, False), (5, False), (6, True)):
        def run():
            draw[0] += 1
            with torch.no_grad():
                return m.rollout_batch(wm, enc, tags, samples=K - int(greedy), seed=args.seed, draw=draw[0], greedy_first=greedy)
        med, lo, hi = timed(run, args.repeats)
        lens = (run()[1].reshape(-1) - 1).tolist()
        emit(what="rollout", images=N, slots=K, greedy_first=greedy, median_ms=round(med, 3), min_ms=round(lo, 3),
             max_ms=round(hi, 3), captions_per_s=round(N * K * 1e3 / med, 1), images_per_s=round(N * 1e3 / med, 1),
             mean_length=round(sum(lens) / len(lens), 1), longest=max(lens))
    m.eval()
    for beam in (1, 5):
        def run():
            with torch.no_grad():
                return m.sample_batch(beam, wm, enc, tags)
        med, lo, hi = timed(run, args.repeats)
        emit(what="search", images=N, beam=beam, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
             images_per_s=round(N * 1e3 / med, 1), steps_longest=max(len(r[0]) for r in run()) - 1)

    def run():
        with torch.no_grad():
            return module_loop(m, wm, enc, tags, 5)
    med, lo, hi = timed(run, args.repeats)
    emit(what="module_loop", images=N, slots=5, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
         captions_per_s=round(N * 5 * 1e3 / med, 1), steps=int(run().shape[1]))
    m.train()
    index = torch.arange(N)
    med, lo, hi = timed(lambda: ts.step(None, tags, index, encoder_out=enc), args.repeats)
    emit(what="scst_step", images=N, samples=5, baseline="greedy", median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
         teacher_forced_rows=N * 5, mean_reward=round(float(ts.last["mean_reward"]), 4))
    ce = TrainStep(device=dev, encoder=False, seed=args.seed, vocab_size=V, dropout=0.0)
    _, _, caps, caplens = synthetic_batch(N, V, 50, 8, S, dev, 3, ragged=True)
    med, lo, hi = timed(lambda: ce.step(None, tags, caps, caplens, encoder_out=enc), args.repeats)
    emit(what="cross_entropy_step", images=N, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3))
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/scst_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
