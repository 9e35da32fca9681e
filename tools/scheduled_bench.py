"""Scheduled sampling on the device: what the mix pass and a mixed cross-entropy step cost.

    python tools/scheduled_bench.py [--images 32] [--repeats 9] [--parent-tree DIR] [--rounds 3]
                                    [--out profiles/scheduled_bench.txt]

AttentionSCN at the train step's widths (P=196, E=2048, A=D=F=M=512, S=1000, V=10000) with random weights (one seed), the logits
sharpened as in tools/scst_bench.py and the <end> bias LOWERED, so that no sampled row ends early: a rollout then runs all
51 steps, the most it can cost, next to the 50 steps of the mix pass over 51-word captions (<start>, 50 words, <end>:
decode_lengths 51, of which the inputs 1 .. 50 can be replaced).  Times are therefore also given per step.
After one warm-up pass each measurement is the median of `--repeats` passes, each bracketed by device events (the drivers
synchronise inside, so the events see host time too).  One JSON line per measurement:

  mix            decoder.mix_batch at p = 0.25 and p = 1.0 (every pass another draw)
  rollout        decoder.rollout_batch(samples=1) on the same rows, in this process
  rollout_child  the same measurement in a fresh process per run, alternating between THIS tree and `--parent-tree` (a checkout
                 of the parent commit with its library built), `--rounds` runs each: the runs of one tree give the
                 run-to-run spread (the larger of the two trees' max - min), against which the difference between the
                 trees' means is read
  ce_step        TrainStep.step, decoder only (the encoder output is an input), at scheduled_sampling 0, 0.25 and 1.0
  module_mix     the same mixing through the module path: one decode step of the nn.Module per word over all rows,
                 torch.multinomial for the sample, torch.where against a host-side coin tensor for the mix (p = 0.25)

Not measured here: other batch sizes, captions of mixed lengths (the pass costs its longest row), the encoder in the step.
Not part of bench.py."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def use_tree(root):
    for p in (os.path.join(root, "indonesian-image-captioning_amd"), root):
        if p not in sys.path:
            sys.path.insert(0, p)


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
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def module_mix(m, wm, enc, tags, caps, nmix, prob, gen):
    """the module path: per word one nn.Module step, torch.multinomial, torch.where"""
    import torch
    from scnattn import functional as SF
    N, hh, ww, E = enc.shape
    e = enc.reshape(N, hh * ww, E)
    h, c = m.init_hidden_state(e)
    prev = caps[:, 0]
    inputs = caps.clone()
    for s in range(int(nmix.max())):
        emb = m.embedding(prev)
        awe, _ = m.attention(e, h)
        gate = torch.sigmoid(SF.linear(h, m.f_beta.weight, m.f_beta.bias))
        h, c = m.decode_step(torch.cat([emb, gate * awe], dim=1), tags, (h, c))
        logits = SF.linear(h, m.fc.weight, m.fc.bias)
        sample = torch.multinomial(torch.softmax(logits, dim=1), 1).squeeze(1)
        coin = (torch.rand(N, generator=gen, device=enc.device) < prob) & (s < nmix)
        prev = torch.where(coin, sample, caps[:, s + 1])
        inputs[:, s + 1] = prev
    return inputs


def setup(args):
    import torch
    from trains.harness import TrainStep, synthetic_batch
    dev = torch.device("cuda:0")
    V, E, S, N = args.vocab, 2048, 1000, args.images
    ts = TrainStep(device=dev, encoder=False, seed=args.seed, vocab_size=V, dropout=0.0)
    with torch.no_grad():
        ts.decoder.fc.weight.mul_(args.sharpen)
        ts.decoder.fc.bias[V - 1] -= args.end_bias
    g = torch.Generator().manual_seed(args.seed)
    enc = torch.rand(N, 14, 14, E, generator=g).to(dev)
    tags = torch.rand(N, S, generator=g).to(dev)
    _, _, caps, caplens = synthetic_batch(N, V, 50, 8, S, dev, 3)
    return ts, dev, word_map(V), enc, tags, caps, caplens


def rollout_entry(args, m, wm, enc, tags):
    import torch
    draw = [0]

    def run():
        draw[0] += 1
        with torch.no_grad():
            return m.rollout_batch(wm, enc, tags, samples=1, seed=args.seed, draw=draw[0])
    r = timed(run, args.repeats)
    lens = (run()[1].reshape(-1) - 1).tolist()
    steps = max(lens)
    return dict(images=enc.shape[0], steps=steps, shortest=min(lens), ms_per_step=round(r["median_ms"] / steps, 4), **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sharpen", type=float, default=10.0)
    ap.add_argument("--end-bias", type=float, default=1000.0)
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3, help="runs per tree of the this-tree / parent-tree comparison")
    ap.add_argument("--rollout-only", metavar="TREE", help="(child) measure rollout_batch with the package of TREE, print one line")
    ap.add_argument("--out")
    args = ap.parse_args()
    use_tree(os.path.abspath(args.rollout_only) if args.rollout_only else HERE)
    import torch
    assert torch.cuda.is_available(), "scheduled_bench needs an MI355X: there is nothing to measure on a CPU"
    ts, dev, wm, enc, tags, caps, caplens = setup(args)
    m = ts.decoder
    if args.rollout_only:
        import scnattn
        assert os.path.abspath(scnattn.__file__).startswith(os.path.abspath(args.rollout_only) + os.sep), scnattn.__file__
        print(json.dumps(dict(what="rollout_child", **rollout_entry(args, m, wm, enc, tags))), flush=True)
        return
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    N = enc.shape[0]
    nmix = (caplens.reshape(-1) - 2).clamp_min(0)
    steps = int(nmix.max())
    draw = [0]
    for prob in (0.25, 1.0):
        def run():
            draw[0] += 1
            with torch.no_grad():
                return m.mix_batch(wm, enc, tags, caps, caplens, prob, seed=args.seed, draw=draw[0])
        r = timed(run, args.repeats)
        emit(what="mix", images=N, prob=prob, steps=steps, replaced=int(run()["n_replaced"].sum()), of=int(nmix.sum()),
             ms_per_step=round(r["median_ms"] / steps, 4), **r)
    emit(what="rollout", **rollout_entry(args, m, wm, enc, tags))
    if args.parent_tree:
        child = [sys.executable, os.path.abspath(__file__), "--images", str(args.images), "--repeats", str(args.repeats),
                 "--vocab", str(args.vocab), "--seed", str(args.seed), "--sharpen", str(args.sharpen), "--end-bias",
                 str(args.end_bias), "--rollout-only"]
        got = {"this": [], "parent": []}
        pair = (("this", HERE), ("parent", args.parent_tree))
        for tree, root in [x for i in range(max(args.rounds, 2)) for x in pair[::1 if i % 2 == 0 else -1]]:
            out = subprocess.run(child + [root], check=True, capture_output=True, text=True, timeout=300).stdout
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            got[tree].append(rec["median_ms"])
            emit(tree=tree, **rec)
        spread = max(max(x) - min(x) for x in got.values())
        moved = abs(statistics.mean(got["this"]) - statistics.mean(got["parent"]))
        emit(what="rollout_this_vs_parent", this_ms=got["this"], parent_ms=got["parent"], run_to_run_spread_ms=round(spread, 3),
             difference_of_means_ms=round(moved, 3), within_spread=bool(moved <= spread))
    for prob in (0.0, 0.25, 1.0):
        ts.set_sampling_prob(prob)
        r = timed(lambda: ts.step(None, tags, caps, caplens, encoder_out=enc), args.repeats)
        emit(what="ce_step", images=N, scheduled_sampling=prob, **r)
    gen = torch.Generator(device=dev).manual_seed(args.seed)

    def run():
        with torch.no_grad():
            return module_mix(m, wm, enc, tags, caps, nmix, 0.25, gen)
    r = timed(run, args.repeats)
    emit(what="module_mix", images=N, prob=0.25, steps=steps, ms_per_step=round(r["median_ms"] / steps, 4), **r)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/scheduled_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
