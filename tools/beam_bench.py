"""Caption generation throughput: sample_batch() on a batch of images against sample() looped over the same images.

    python tools/beam_bench.py [--images 32] [--beam 5] [--repeats 7] [--out profiles/NAME.txt]

Both sides get the same random weights (one seed) at the train step's widths (P=196, E=2048, A=D=F=M=512, S=1000,
V=10000), with the <end> bias raised so that searches end at mixed lengths.  Each side runs in a FRESH process
(`--side batched|loop`, started from here): a warm-up pass over the whole batch, then `--repeats` timed passes, each
bracketed by device events around the whole batch (the searches synchronise inside, so the events see host time too);
the median is reported.  Prints one JSON line per side and one for the ratio.  Not part of bench.py.

    python tools/beam_bench.py --side batched --end-bias -30 [--no-repeat-ngram 3 --ban-unk] [--min-length N]

One side alone; with --end-bias -30 nothing completes and every search runs all 51 steps, which makes the plain search
and the search with options comparable per step.

    python tools/beam_bench.py --side batched --end-bias -30 --beam 2 --groups 3 --diversity 0.5

The diverse search: `--groups` groups of `--beam` beams each, to be set beside the plain search at the same
total (`--beam 6`).

    python tools/beam_bench.py --side batched --end-bias -30 --require C [--launches]

The constrained search: every image requires C words (0 <= C <= min(4, beam - 1)) chosen by a fixed rule from
its own plain result -- the plain search's picks of step 0 at ranks 1 .. C (rank 0 is the word the plain caption starts
with), special tokens left out -- so they are reachable.  `--require 0` runs the constrained calls with empty lists.
`--launches` also reports the device kernels per step of the search the side runs: the kernels of a search cut off after
51 steps minus those of one cut off after 11, over 40 (torch.profiler; null when the trace is unavailable).
`--search-only` times the search on the device with the download of its records (SF.beam_search_run) and leaves out the
host's trace-back, which builds the attention maps as nested lists and is most of the spread of the end-to-end figure."""
import argparse
import json
import os
import statistics
import subprocess
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


def side(args):
    import torch
    from models.decoders.attention_scn import AttentionSCN
    assert torch.cuda.is_available(), "beam_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    V, E, S = args.vocab, 2048, 1000
    m = AttentionSCN(512, 512, 512, 512, S, V, encoder_dim=E, dropout=0.0)
    with torch.no_grad():
        m.fc.weight.mul_(args.sharpen)              # random-init logits are nearly uniform: sharpen them ...
        m.fc.bias[V - 1] += args.end_bias           # ... and raise <end> so that beams complete at different steps
    m = m.to(dev).eval()
    enc = torch.rand(args.images, 14, 14, E).to(dev)
    tags = torch.rand(args.images, S).to(dev)
    wm = word_map(V)
    kw = {}
    if args.no_repeat_ngram or args.min_length or args.ban_unk:
        from models.decoders import SearchOptions
        kw["options"] = SearchOptions(min_length=args.min_length, no_repeat_ngram=args.no_repeat_ngram,
                                      banned_tokens=(wm["<unk>"],) if args.ban_unk else ())

    req = None
    if args.require is not None:
        from models.decoders import _common
        from scnattn import functional as SF
        if not 0 <= args.require <= min(4, args.beam - 1):
            raise SystemExit("--require must be in [0, min(4, beam - 1)]")
        ops = _common._search_operands(m, V, enc, tags, True, True)
        res, _ = SF.beam_search_run(ops[0], args.beam, *ops[1:], wm["<start>"], wm["<end>"])
        never = {wm["<pad>"], wm["<unk>"], wm["<start>"], wm["<end>"]}
        first = res["token"][0].view(args.images, args.beam).tolist()      # step 0: the plain search's picks in rank order
        req = [[w for w in row[1:] if w not in never][:args.require] for row in first]

    if args.search_only:
        from models.decoders import _common
        from scnattn import functional as SF
        s_ops = _common._search_operands(m, V, enc, tags, True, True)
        s_kw = dict(options=_common.device_options(kw.get("options"))[0])
        if args.groups:
            s_kw.update(groups=args.groups, diversity=args.diversity)
        if req is not None:
            s_kw.update(required=req, pad_token=wm["<pad>"])

    def run():
        with torch.no_grad():
            if args.search_only:        # the records of step 0 stand for the captions in the digest
                res, _ = SF.beam_search_run(s_ops[0], args.beam * (args.groups or 1), *s_ops[1:], wm["<start>"], wm["<end>"],
                                            **s_kw)
                return res["token"].t().tolist()[:args.images]
            if args.side == "batched" and req is not None:
                return [r[0] for r in m.sample_constrained(args.beam, req, wm, enc, tags, **kw)]
            if args.side == "batched" and args.groups:     # the first group's caption stands for the image
                return [r[0][0] for r in m.sample_groups(args.beam, args.groups, args.diversity, wm, enc, tags, **kw)]
            if args.side == "batched":
                return [r[0] for r in m.sample_batch(args.beam, wm, enc, tags, **kw)]
            return [m.sample(args.beam, wm, enc[i:i + 1], tags[i:i + 1])[0] for i in range(args.images)]

    seqs = run()                                    # warm-up: code objects, allocator, workspaces
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    lens = [len(s) for s in seqs]
    met = None if req is None or args.search_only else sum(all(w in s for w in r) for s, r in zip(seqs, req))
    per_step = launches_per_step(m, args, wm, enc, tags, req, kw.get("options")) if args.launches else None
    print(json.dumps({"side": args.side, "images": args.images, "beam": args.beam, "groups": args.groups,
                      "diversity": args.diversity, "require": args.require, "search_only": args.search_only,
                      "captions_with_all_words": met,
                      "kernels_per_step": per_step, "median_ms": round(med, 3),
                      "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "captions_per_s": round(args.images * 1e3 / med, 2),
                      "options": repr(kw.get("options")), "ms_per_step_of_longest": round(med / (max(lens) - 1), 4),
                      "steps_longest": max(lens) - 1, "lengths": sorted(lens), "digest": hash(tuple(map(tuple, seqs))) & 0xffffffff}))


def launches_per_step(m, args, wm, enc, tags, req, options):
    """device kernels per step of the search this side runs (SF.beam_search_run; copies and fills are not kernels): the
    count of a search of 51 steps minus that of 11 steps, over 40; None when the profiler cannot attach"""
    import torch
    from models.decoders import _common
    from scnattn import functional as SF
    ops = _common._search_operands(m, len(wm), enc, tags, True, True)
    extra = dict(options=_common.device_options(options)[0])
    if args.groups:
        extra.update(groups=args.groups, diversity=args.diversity)
    if req is not None:
        extra.update(required=req, pad_token=wm["<pad>"])
    beam = args.beam * (args.groups or 1)

    def kernels(steps):
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _, ran = SF.beam_search_run(ops[0], beam, *ops[1:], wm["<start>"], wm["<end>"], max_steps=steps, **extra)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return sum(1 for x in names if not x.lower().startswith(("memcpy", "memset", "copy", "fill"))), ran

    try:
        kernels(11)
        (a, ra), (b, rb) = kernels(11), kernels(51)
        return round((b - a) / (rb - ra), 3) if rb > ra else None
    except Exception as e:  # noqa: BLE001 -- a profiler that cannot attach is reported, not fatal
        print("profiler unavailable: %s" % e, file=sys.stderr, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sharpen", type=float, default=10.0)
    ap.add_argument("--end-bias", type=float, default=2.0)
    ap.add_argument("--no-repeat-ngram", type=int, default=0)      # search options (batched side only)
    ap.add_argument("--min-length", type=int, default=0)
    ap.add_argument("--ban-unk", action="store_true")
    ap.add_argument("--groups", type=int, default=0)               # diverse search (batched side only):
    ap.add_argument("--diversity", type=float, default=0.5)        # --groups groups of --beam beams; 0: the plain search
    ap.add_argument("--require", type=int, default=None)           # constrained search (batched side only)
    ap.add_argument("--launches", action="store_true")             # also count the device kernels per step
    ap.add_argument("--search-only", action="store_true")          # time SF.beam_search_run, not the host's trace-back
    ap.add_argument("--side", choices=["batched", "loop"])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.side:
        side(args)
        return
    lines = []
    for s in ("batched", "loop"):
        cmd = [sys.executable, os.path.abspath(__file__), "--side", s] + [a for a in sys.argv[1:]]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    a, b = (json.loads(x) for x in lines)
    lines.append(json.dumps({"batched_over_loop": round(a["captions_per_s"] / b["captions_per_s"], 3),
                             "same_captions": a["digest"] == b["digest"]}))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/beam_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
