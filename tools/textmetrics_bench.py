"""Caption text metrics on the device (csrc/textmetrics.hip, scnattn.textmetrics) against the same metrics in pure Python.

Synthetic corpora of 1000 and 5000 images x 5 references, sentence lengths 8..22, V = 10 000, noisy copies of random base
sentences (tests/textmetrics_refs.py::make_case, the generator of oracle/gen_bleu_golden.py).  Per corpus, wall clock around a
device synchronise, a warm-up and then repetitions, median and range:

    CaptionScorer(...)        from Python lists (packing and one upload included) and from packed device tensors
    scorer.score(...)         from Python lists and from packed device tensors (both end in the one download)
    host, one thread          the pure-Python restatements of tests/textmetrics_refs.py: n-gram statistics + both BLEU tails,
                              ROUGE-L, CIDEr-D; and utils.metric.corpus_bleu, the BLEU-4 validate() runs today

and the values of the two sides next to each other.  Then validate(fused=True) with and without device_bleu on the workload
of tools/caption_metrics_bench.py (AttentionSCN at the BASELINE widths, B = 32, T = 51, V = 10 000, five references, encoder and
tagger replaced by their outputs), one batch per pass and eight, the two sides interleaved.  Needs an MI355X.

    python tools/textmetrics_bench.py [--reps 9] [--warmup 2] [--host-reps 3] [--out profiles/textmetrics_bench.txt]"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indonesian-image-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

B, T, V = 32, 51, 10000


def _fmt(name, ms):
    return "%-58s median %10.3f ms  [%10.3f .. %10.3f]  n = %d" % (name, statistics.median(ms), min(ms), max(ms), len(ms))


def _timed(fn, warmup, reps, sync):
    out, ms = None, []
    for i in range(warmup + reps):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    return out, ms


def corpus_side(n_img, dev, args):
    import torch
    import textmetrics_refs as R
    from scnattn import textmetrics as TM
    from utils.metric import corpus_bleu
    refs, hyps = R.make_case(random.Random(n_img), n_img, V, 5, 8, 22, 0.25)
    sync = torch.cuda.synchronize
    lines = ["-- %d images x 5 references, lengths 8..22, V = %d" % (n_img, V)]
    scorer, ms = _timed(lambda: TM.CaptionScorer(refs, device=dev), args.warmup, args.reps, sync)
    lines.append(_fmt("CaptionScorer from lists (pack, upload, 4 tables)", ms))
    packed_r = TM.pack_references(refs, dev)
    _, ms = _timed(lambda: TM.CaptionScorer(packed_r, device=dev), args.warmup, args.reps, sync)
    lines.append(_fmt("CaptionScorer from packed device tensors", ms))
    dev_scores, ms = _timed(lambda: scorer.score(hyps), args.warmup, args.reps, sync)
    lines.append(_fmt("score() from lists (pack, upload, 3 kernels, download)", ms))
    packed_h = TM.pack_captions(hyps, dev)
    _, ms = _timed(lambda: scorer.score(packed_h), args.warmup, args.reps, sync)
    lines.append(_fmt("score() from packed device tensors", ms))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev = []
    for i in range(args.warmup + args.reps):
        e0.record()
        scorer.score(packed_h)
        e1.record()
        e1.synchronize()
        if i >= args.warmup:
            ev.append(e0.elapsed_time(e1))
    lines.append(_fmt("score() from packed tensors, device events", ev))

    nothing = lambda: None
    (tot, den), ms_b = _timed(lambda: R.corpus_totals(hyps, refs), 1, args.host_reps, nothing)
    lines.append(_fmt("host: n-gram statistics n = 1..4 (dicts of tuples)", ms_b))
    rouge, ms_r = _timed(lambda: R.mean([R.rouge_l(h, r)[1] for h, r in zip(hyps, refs)]), 1, args.host_reps, nothing)
    lines.append(_fmt("host: ROUGE-L (LCS table per pair)", ms_r))
    cider, ms_c = _timed(lambda: R.mean(R.cider_scores(hyps, refs)), 1, args.host_reps, nothing)
    lines.append(_fmt("host: CIDEr-D (df + tf-idf vectors)", ms_c))
    b4, ms_n = _timed(lambda: corpus_bleu(refs, hyps), 1, args.host_reps, nothing)
    lines.append(_fmt("host: utils.metric.corpus_bleu (BLEU-4 only)", ms_n))
    host_all = statistics.median(ms_b) + statistics.median(ms_r) + statistics.median(ms_c)
    host = {"Bleu_%d" % (n + 1): b for n, b in enumerate(R.bleu_coco_tail(tot[0:4], tot[4:8], tot[8], tot[9]))}
    host.update(ROUGE_L=rouge, CIDEr=cider, bleu4_nltk=R.bleu_nltk_tail(tot[0:4], den, tot[8], tot[9]))
    lines.append("host, the three metrics together (sum of the medians): %.1f ms" % host_all)
    worst = max(abs(dev_scores[k] - host[k]) / max(1.0, abs(host[k])) for k in host)
    lines.append("values  device: " + "  ".join("%s %.6f" % (k, dev_scores[k]) for k in sorted(host)))
    lines.append("values  host:   " + "  ".join("%s %.6f" % (k, host[k]) for k in sorted(host)))
    lines.append("largest |device - host| / max(1, |host|) over the seven values: %.3g; corpus_bleu %.6f" % (worst, b4))
    return lines


def validate_side(dev, args):
    """validate(fused=True) passes, device_bleu off / on, interleaved; wall clock from the call to its return"""
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
    lines = ["-- validate(fused=True): AttentionSCN 512/512/512/512/1000, B = %d, T = %d, V = %d, 5 references per image" % (B, T, V)]
    for nb in (1, 8):
        batches = [(None, caps, caplens, allcaps)] * nb
        ms, res = {False: [], True: []}, {}
        for i in range(args.warmup + args.reps):
            for flag in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[flag] = validate(batches, encoder, lambda x: tags, dec, None, wm, fused=True, device_bleu=flag)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ms[flag].append(1e3 * (time.perf_counter() - t0))
        lines.append(_fmt("%d batch(es), device_bleu=False (decoder included)" % nb, ms[False]))
        lines.append(_fmt("%d batch(es), device_bleu=True  (decoder included)" % nb, ms[True]))
        a, b = statistics.median(ms[False]), statistics.median(ms[True])
        spread = max(max(ms[k]) - min(ms[k]) for k in ms)
        lines.append("    device_bleu=True - False = %+.3f ms (%+.1f %%); largest range of the two sides %.3f ms; the three "
                     "returned values %s" % (b - a, 100.0 * (b - a) / a, spread,
                                             "bit-equal" if res[False] == res[True] else "DIFFER"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("textmetrics_bench: needs an MI355X; there is nothing to measure without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    lines = ["textmetrics_bench: %d repetitions after %d warm-up rounds on the device sides, %d after 1 on the host sides; wall "
             "clock around a device synchronise unless stated; host sides on one thread" % (args.reps, args.warmup, args.host_reps)]
    for n_img in (1000, 5000):
        lines += corpus_side(n_img, dev, args)
    lines += validate_side(dev, args)
    for ln in lines:
        print(ln, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
