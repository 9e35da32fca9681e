"""Truncated sampling on the device: what a top-k / nucleus rollout costs beside the plain rollout and the search.

    python tools/sampling_bench.py [--images 32] [--slots 5] [--repeats 7] [--out profiles/sampling_bench.txt]
    python tools/sampling_bench.py --plain-only [--package OTHER/indonesian-image-captioning_amd]

One process, AttentionSCN at the train step's widths (P=196, E=2048, A=D=F=M=512, S=1000, V=10000) with random weights (one
seed), the logits sharpened and the <end> bias raised as in tools/scst_bench.py, 32 images x 5 slots.  After one warm-up pass
each measurement is the median of `--repeats` passes, each bracketed by device events (the rollouts synchronise inside, so the
events see host time too).  One JSON line per measurement:

  rollout        rollout_batch with the filter off, top_k=50, top_p=0.9 and both: ms per batch, steps run, ms per step,
                 mean_length / longest of the captions (a filter shortens captions, so compare per step)
  search         sample_batch with beam 5 on the same images: the search the filtered rollout is the cheap alternative to
  module_loop    the same truncated sampling done with the module path, the "before": one decode step of the nn.Module per
                 time step over all rows, torch.sort + cumulative sum + torch.multinomial for the pick (top_k=50, top_p=0.9),
                 the open-row test on the host

--plain-only measures the filter-off rollout alone and needs nothing this tool's commit added, so --package can point it at
the package directory of another checkout (built there): alternate the two for an A/B of the plain path.

Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def module_loop(m, wm, enc, tags, K, top_k, top_p, max_steps=51):
    """K truncated samples per image through the module's own step: sort, cut, multinomial per step, the stop test on the host"""
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
        prob, idx = torch.sort(torch.softmax(logits, dim=1), dim=1, descending=True)
        before = torch.cumsum(prob, dim=1) - prob                   # the mass in front of each word: keep while it is < top_p
        keep = before < top_p
        keep[:, top_k:] = False
        prob = torch.where(keep, prob, torch.zeros_like(prob))
        prev = idx.gather(1, torch.multinomial(prob, 1)).squeeze(1)
        out.append(prev)
        open_ &= prev != wm["<end>"]
        if not any(open_.tolist()):
            break
    return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sharpen", type=float, default=10.0)
    ap.add_argument("--end-bias", type=float, default=2.0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--package", default=os.path.join(ROOT, "indonesian-image-captioning_amd"))
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    from models.decoders.attention_scn import AttentionSCN
    assert torch.cuda.is_available(), "sampling_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    V, E, S, N, K = args.vocab, 2048, 1000, args.images, args.slots
    wm = word_map(V)
    torch.manual_seed(args.seed)
    m = AttentionSCN(512, 512, 512, 512, S, V, encoder_dim=E, dropout=0.0).to(dev).eval()
    with torch.no_grad():
        m.fc.weight.mul_(args.sharpen)
        m.fc.bias[V - 1] += args.end_bias
    g = torch.Generator().manual_seed(args.seed)
    enc = torch.rand(N, 14, 14, E, generator=g).to(dev)
    tags = torch.rand(N, S, generator=g).to(dev)
    lines = []

    def emit(**kw):
        if args.label:
            kw["label"] = args.label
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    draw = [0]
    filters = [("off", {})] if args.plain_only else [("off", {}), ("top_k=50", {"top_k": 50}), ("top_p=0.9", {"top_p": 0.9}),
                                                     ("top_k=50,top_p=0.9", {"top_k": 50, "top_p": 0.9})]
    for name, kw in filters:
        def run():
            draw[0] += 1
            with torch.no_grad():
                return m.rollout_batch(wm, enc, tags, samples=K, seed=args.seed, draw=draw[0], **kw)
        med, lo, hi = timed(run, args.repeats)
        caps, caplens, _ = run()            # one more pass, to describe the captions
        lens = (caplens.reshape(-1) - 1).tolist()
        emit(what="rollout", filter=name, images=N, slots=K, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
             captions_per_s=round(N * K * 1e3 / med, 1), steps_last_pass=caps.shape[1] - 1,
             mean_length=round(sum(lens) / len(lens), 1), longest=max(lens))
        # per step: one more pass, timed alone with its own step count (the draws differ from pass to pass, and so do the steps)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per = []
        for _ in range(args.repeats):
            draw[0] += 1
            a.record()
            with torch.no_grad():
                caps = m.rollout_batch(wm, enc, tags, samples=K, seed=args.seed, draw=draw[0], **kw)[0]
            b.record()
            torch.cuda.synchronize()
            per.append(a.elapsed_time(b) / (caps.shape[1] - 1))
        emit(what="rollout_per_step", filter=name, median_ms_per_step=round(statistics.median(per), 4),
             min_ms_per_step=round(min(per), 4), max_ms_per_step=round(max(per), 4))
    if not args.plain_only:
        def run():
            with torch.no_grad():
                return m.sample_batch(5, wm, enc, tags)
        med, lo, hi = timed(run, args.repeats)
        steps = max(len(r[0]) for r in run()) - 1
        emit(what="search", images=N, beam=5, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
             images_per_s=round(N * 1e3 / med, 1), steps_longest=steps)

        def run():
            with torch.no_grad():
                return module_loop(m, wm, enc, tags, K, 50, 0.9)
        med, lo, hi = timed(run, args.repeats)
        steps = int(run().shape[1])
        emit(what="module_loop", filter="top_k=50,top_p=0.9", images=N, slots=K, median_ms=round(med, 3), min_ms=round(lo, 3),
             max_ms=round(hi, 3), captions_per_s=round(N * K * 1e3 / med, 1), steps_last_pass=steps,
             ms_per_step_last_pass=round(med / steps, 4))
    if args.out:
        with open(args.out, "a" if args.plain_only else "w") as f:
            f.write("tools/sampling_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
