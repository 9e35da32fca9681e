"""Scoring given captions on the device: what score_batch costs beside the module path and beside a rollout of the same rows.

    python tools/scoring_bench.py [--images 32] [--slots 5] [--repeats 7] [--out profiles/scoring_bench.txt]
    python tools/scoring_bench.py --parent-only [--package OTHER/indonesian-image-captioning_amd] [--label parent-r1]

One process, AttentionSCN at the train step's widths (P=196, E=2048, A=D=F=M=512, S=1000, V=10000) with random weights (one
seed), the logits sharpened as in tools/sampling_bench.py, 32 images x 5 captions of 51 random tokens each (no <end>: every
step of every row is scored).  After one warm-up pass each measurement is the median of `--repeats` passes, each bracketed by
device events (the drivers synchronise inside, so the events see host time too).  One JSON line per measurement:

  score_batch    decoder.score_batch on the device and the download of its records (logp, rank, best, sum_logp): ms per
                 batch, ms per step, captions per second
  module_path    the same 160 captions through decoder.forward + log_softmax + gather, the "before": every caption repeats
                 the image-side set-up and (rows, T, V) scores are materialised (their size is reported)
  rollout        a plain rollout_batch of the same 160 rows, for orientation: the step chain is the same but for the pick
  search         sample_batch with beam 5 on the same images

--parent-only measures the rollout and the search alone and needs nothing this tool's commit added, so --package can point it
at the package directory of another checkout (built there): alternate the two for an A/B of the existing paths.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--slots", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=51)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sharpen", type=float, default=10.0)
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--package", default=os.path.join(ROOT, "indonesian-image-captioning_amd"))
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    from models.decoders.attention_scn import AttentionSCN
    assert torch.cuda.is_available(), "scoring_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    V, E, S, N, K, T = args.vocab, 2048, 1000, args.images, args.slots, args.tokens
    wm = word_map(V)
    torch.manual_seed(args.seed)
    m = AttentionSCN(512, 512, 512, 512, S, V, encoder_dim=E, dropout=0.0).to(dev).eval()
    with torch.no_grad():
        m.fc.weight.mul_(args.sharpen)      # no <end> bias: the rollout below runs all 51 steps, as the scoring does
    g = torch.Generator().manual_seed(args.seed)
    enc = torch.rand(N, 14, 14, E, generator=g).to(dev)
    tags = torch.rand(N, S, generator=g).to(dev)
    R = N * K
    caps = torch.cat([torch.full((R, 1), wm["<start>"]), torch.randint(1, V - 3, (R, T), generator=g)], dim=1).to(dev)
    caplens = torch.full((R, 1), T + 1, dtype=torch.long, device=dev)
    lines = []

    def emit(**kw):
        if args.label:
            kw["label"] = args.label
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    if not args.parent_only:
        def run():
            with torch.no_grad():
                out = m.score_batch(wm, enc, tags, caps, caplens, per_image=K)
            return torch.cat([out["logp"].view(torch.int32), out["rank"], out["best"],
                              out["sum_logp"].view(torch.int32).unsqueeze(1)], dim=1).cpu()
        med, lo, hi = timed(run, args.repeats)
        emit(what="score_batch", images=N, per_image=K, tokens=T, median_ms=round(med, 3), min_ms=round(lo, 3),
             max_ms=round(hi, 3), ms_per_step=round(med / T, 4), captions_per_s=round(R * 1e3 / med, 1))
        device_lp = run()[:, :T].view(torch.float32)

        enc_rows, tag_rows = enc.repeat_interleave(K, 0), tags.repeat_interleave(K, 0)      # what the module path must be fed

        def run():
            with torch.no_grad():
                scores, caps_sorted, lens, _, sort_ind = m(enc_rows, tag_rows, caps, caplens)
                lp = torch.log_softmax(scores, dim=2).gather(2, caps_sorted[:, 1:].unsqueeze(2)).squeeze(2)
                return lp, sort_ind, scores
        med, lo, hi = timed(run, args.repeats)
        lp, sort_ind, scores = run()
        back = torch.empty_like(lp)
        back[sort_ind] = lp
        worst = float((back.cpu() - device_lp).abs().max())
        emit(what="module_path", images=N, per_image=K, tokens=T, median_ms=round(med, 3), min_ms=round(lo, 3),
             max_ms=round(hi, 3), ms_per_step=round(med / T, 4), captions_per_s=round(R * 1e3 / med, 1),
             scores_MB=round(scores.numel() * 4 / 1e6, 1), worst_abs_diff_of_logp=worst)
        del lp, scores, back

    draw = [0]

    def run():
        draw[0] += 1
        with torch.no_grad():
            return m.rollout_batch(wm, enc, tags, samples=K, seed=args.seed, draw=draw[0])
    med, lo, hi = timed(run, args.repeats)
    steps = run()[0].shape[1] - 1
    emit(what="rollout", filter="off", images=N, slots=K, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
         steps_last_pass=steps, ms_per_step=round(med / steps, 4), captions_per_s=round(R * 1e3 / med, 1))

    def run():
        with torch.no_grad():
            return m.sample_batch(5, wm, enc, tags)
    med, lo, hi = timed(run, args.repeats)
    emit(what="search", images=N, beam=5, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
         images_per_s=round(N * 1e3 / med, 1), steps_longest=max(len(r[0]) for r in run()) - 1)
    if args.out:
        with open(args.out, "a" if args.parent_only else "w") as f:
            f.write("tools/scoring_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
