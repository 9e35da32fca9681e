"""The caption metrics in the loss pass (csrc/loss.hip, scnattn.functional.caption_loss_metrics) at B = 32, T = 51, V = 10 000,
P = 196 with ragged lengths: three sides in ONE process, interleaved, each repetition of each side between two device events
after a warm-up:

    (a) caption_loss forward             -- the pass as it was
    (b) caption_loss_metrics forward     -- the same pass with target ranks, arg-max tokens and the top-5 / top-1 counts
    (c) the eager metric ops (b) replaces in validate(): scores.clone(), two pack_padded_sequence, accuracy(.., 5),
        torch.max(dim=2)                 -- without their .item() / .tolist() synchronisations

Four score tensors (65 MB each) take turns, so no side finds its input in a cache.  Printed: median and range per side, the
two expectations -- (b) within 10 % of (a)'s median, or within (a)'s own range when that is larger, and (b) < (a) + (c) -- and
the host time of one validate() batch (AttentionSCN at the BASELINE widths, encoder and tagger replaced by their outputs),
fused against eager, wall clock around a device synchronise.  Needs an MI355X: without one it fails.

    python tools/caption_metrics_bench.py [--reps 9] [--warmup 3] [--out profiles/caption_metrics_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indonesian-image-captioning_amd"))
sys.path.insert(0, ROOT)

B, T, V, P = 32, 51, 10000, 196
NBUF = 4


def _fmt(name, ms):
    return "%-44s median %8.3f ms  [%8.3f .. %8.3f]" % (name, statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("caption_metrics_bench: needs an MI355X; there is nothing to measure without one")
    from torch.nn.utils.rnn import pack_padded_sequence
    from scnattn import functional as SF
    from utils.metric import accuracy
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    lens = sorted(torch.randint(7, T + 1, (B,), generator=g).tolist(), reverse=True)
    lens[0] = T
    caps = torch.randint(1, V - 3, (B, T + 1), generator=g)
    lift = torch.zeros(B, T, V).scatter_(2, caps[:, 1:].unsqueeze(2), 9.0)      # the target three sigma up: a top-5 worth counting
    scores = [(3 * torch.randn(B, T, V, generator=g) + lift).to(dev) for _ in range(NBUF)]
    caps = caps.to(dev)
    alphas = torch.softmax(torch.randn(B, T, P, generator=g), dim=2).to(dev)
    dl_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    targets = caps[:, 1:]

    def side_a(s):
        return SF.caption_loss(s, caps, lens, alphas, 1.0, dl_dev)

    def side_b(s):
        return SF.caption_loss_metrics(s, caps, lens, alphas, 1.0, dl_dev, k=5)

    def side_c(s):
        copy = s.clone()
        sp = pack_padded_sequence(s, lens, batch_first=True).data
        tp = pack_padded_sequence(targets, lens, batch_first=True).data
        _, ind = sp.topk(5, 1, True, True)                      # utils.metric.accuracy without its .item()
        correct = ind.eq(tp.view(-1, 1).expand_as(ind)).view(-1).float().sum()
        return correct, torch.max(copy, dim=2)[1]

    sides = (("a", side_a), ("b", side_b), ("c", side_c))
    ms = {k: [] for k, _ in sides}
    with torch.no_grad():
        for i in range(args.warmup + args.reps):
            for name, fn in sides:
                s = scores[i % NBUF]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(s)
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        # the three sides agree on what they compute
        la, (lb, hits, preds), (correct, amax) = side_a(scores[0]), side_b(scores[0]), side_c(scores[0])
        n = sum(lens)
        assert torch.equal(la, lb), "caption_loss and caption_loss_metrics disagree on the loss bits"
        top5 = (float(int(hits[0])) * (100.0 / n), accuracy(pack_padded_sequence(scores[0], lens, batch_first=True).data,
                                                            pack_padded_sequence(targets, lens, batch_first=True).data, 5))
        same_preds = all(torch.equal(preds[b_, :l].long(), amax[b_, :l]) for b_, l in enumerate(lens))
    a, b, c = (statistics.median(ms[k]) for k in "abc")
    spread = max(ms["a"]) - min(ms["a"])
    within = b <= 1.10 * a or b - a <= spread
    below = b < a + c
    mb = 4.0 * n * V / 1e6
    lines = ["caption_metrics_bench: B = %d, T = %d, V = %d, P = %d, %d decoded rows (%.1f MB of scores read per pass), %d score "
             "tensors in rotation, %d repetitions after %d warm-up rounds, sides interleaved in one process, device events"
             % (B, T, V, P, n, mb, NBUF, args.reps, args.warmup),
             _fmt("(a) caption_loss forward", ms["a"]),
             _fmt("(b) caption_loss_metrics forward", ms["b"]),
             _fmt("(c) eager clone + 2 packs + top-5 + max(dim=2)", ms["c"]),
             "(b) - (a) = %+.3f ms (%+.1f %% of (a)); (a)'s range %.3f ms: (b) within 10 %% of (a) or within (a)'s range: %s"
             % (b - a, 100.0 * (b - a) / a, spread, "met" if within else "NOT met"),
             "(b) %.3f ms < (a) + (c) = %.3f ms: %s" % (b, a + c, "met" if below else "NOT met"),
             "same loss bits from (a) and (b); top-5 %.4f %% from (b), %.4f %% from accuracy(); arg-max tokens of (b) and "
             "torch.max %s (random fp32 rows of %d can hold equal values, where topk follows no index rule)"
             % (top5[0], top5[1], "equal" if same_preds else "differ", V)]
    lines += validate_host_time(dev, args)
    for ln in lines:
        print(ln, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if (within and below) else 1


def validate_host_time(dev, args):
    """one validate() batch, fused against eager: wall clock from the call to its return (both end in downloads)"""
    import torch
    from models.decoders.attention_scn import AttentionSCN
    from trains.harness import validate, synthetic_batch
    torch.manual_seed(2)
    dec = AttentionSCN(512, 512, 512, 512, 1000, V).to(dev)
    _, tags, caps, caplens = synthetic_batch(B, V, T - 1, 8, 1000, dev, 3, ragged=True)
    enc = torch.rand(B, 14, 14, 2048, device=dev)
    allcaps = torch.stack([caps] * 5, dim=1)
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    encoder = type("E", (), {"eval": lambda s: None, "__call__": lambda s, x: enc})()
    crit = torch.nn.CrossEntropyLoss().to(dev)
    ms, res = {True: [], False: []}, {}
    for i in range(2 + 5):
        for fused in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[fused] = validate([(None, caps, caplens, allcaps)], encoder, lambda x: tags, dec, crit, wm, fused=fused)
            torch.cuda.synchronize()
            if i >= 2:
                ms[fused].append(1e3 * (time.perf_counter() - t0))
    same = res[True][0] == res[False][0] and res[True][2] == res[False][2]
    return [_fmt("validate() batch, eager (decoder included)", ms[False]), _fmt("validate() batch, fused (decoder included)", ms[True]),
            "validate(): BLEU-4 and top-5 of the two paths %s; loss eager %.6f fused %.6f"
            % ("equal" if same else "DIFFER", res[False][1], res[True][1])]


if __name__ == "__main__":
    sys.exit(main())
