"""Tagger train step (trains/tagger.py:153-173): `TaggerTrainStep` (fused head, csrc/taghead.hip) against the module path it
replaces (EncoderTagger.forward + nn.BCELoss + backward + the same FusedClampAdam), B = 32, 3 x 256 x 256, S = 1000, in four
configurations: trunk frozen (the reference's default) / fine-tuned, fp32 / bf16 trunk.

Every measurement runs in a fresh child process (subprocess, its own timeout); the two sides alternate, `--rounds` children
each.  A child warms up, then brackets each of `--steps` (>= 7) steps with device events.  Printed per side: the median and
the range of all its steps.  Acceptance: the fused median is not above the module path's median by more than the module
path's own range in this run.

    python tools/tagger_bench.py [--steps 9] [--warmup 3] [--rounds 2] [--out profiles/tagger_step_bench.txt]
    python tools/tagger_bench.py --head 20      # 20 forward + backward passes of the head alone on fp32, then bf16 maps
                                                # (B = 32, 8 x 8 x 2048, 16 maps in rotation: 268 MB, beyond the caches), for
                                                # `rocprofv3 --kernel-trace --stats -- python tools/tagger_bench.py --head 20`:
                                                # the head's launches and the kernel time of tag_pool_fwd; bytes / that time is
                                                # its achieved bandwidth (16.8 MB read in fp32, 8.4 MB in bf16, + 0.5 MB)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indonesian-image-captioning_amd"))
sys.path.insert(0, ROOT)

B, S, IMG = 32, 1000, 256
CONFIGS = (("frozen", "f32"), ("frozen", "bf16"), ("finetune", "f32"), ("finetune", "bf16"))


def child(args):
    """one side of one configuration: prints `RESULT {...}` with the per-step milliseconds"""
    import torch
    from torch import nn
    from models.encoders.tagger import EncoderTagger
    from trains.harness import TaggerTrainStep
    from utils.optimizer import FusedClampAdam
    dev = torch.device("cuda:0")
    fine_tune, bf16 = args.trunk == "finetune", args.dtype == "bf16"
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(B, 3, IMG, IMG, generator=g).to(dev)
    tags = (torch.rand(B, S, generator=g) >= 0.9).float().to(dev)
    if args.child == "fused":
        ts = TaggerTrainStep(fine_tune_encoder=fine_tune, device=dev, encoder_dtype=args.dtype, semantic_size=S)

        def step():
            return ts.step(imgs, tags)[0]
    else:
        torch.manual_seed(1234)
        m = EncoderTagger(semantic_size=S, dropout=0.15, channels_last=True).to(dev)
        m.fine_tune(fine_tune)
        opt = FusedClampAdam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-4, grad_clip=5.0)
        crit = nn.BCELoss().to(dev)
        m.train()

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                scores = m(imgs)
            loss = crit(scores, tags)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    print("RESULT " + json.dumps(dict(side=args.child, trunk=args.trunk, dtype=args.dtype, ms=ms, loss=float(loss))), flush=True)


def head(args):
    import torch
    from scnattn import functional as SF
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    W = (torch.randn(S, 2048, generator=g) * 0.02).to(dev).requires_grad_(True)
    b = torch.zeros(S, device=dev, requires_grad=True)
    t = (torch.rand(B, S, generator=g) >= 0.9).float().to(dev)
    ks = ((torch.rand(B, 2048, generator=g) >= 0.15).float() / 0.85).to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        maps = [torch.randn(B, 2048, 8, 8, device=dev).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                for _ in range(16)]
        for i in range(args.head):
            W.grad = b.grad = maps[i % 16].grad = None       # no accumulation kernels in the trace
            _, loss, _ = SF.tag_head_loss(maps[i % 16], ks, W, b, t)
            loss.backward()
        torch.cuda.synchronize()
        print("head: %d forward + backward passes on %s maps, loss %.5f" % (args.head, dtype, float(loss)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("fused", "module"), default=None)
    ap.add_argument("--trunk", choices=("frozen", "finetune"), default="frozen")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--head", type=int, default=0)
    args = ap.parse_args()
    if args.steps < 7:
        ap.error("--steps must be at least 7")
    if args.head:
        return head(args)
    if args.child:
        return child(args)
    lines = ["tagger_bench: one train step of the tagger, B = %d, 3 x %d x %d, S = %d; per side %d fresh processes x %d steps after %d "
             "warm-up steps, each step between two device events, sides alternating; ms per step: median [min .. max]"
             % (B, IMG, IMG, S, args.rounds, args.steps, args.warmup)]
    print(lines[0], flush=True)
    ok = True
    for trunk, dtype in CONFIGS:
        ms = {"fused": [], "module": []}
        for _ in range(args.rounds):
            for side in ("fused", "module"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--trunk", trunk, "--dtype", dtype,
                       "--steps", str(args.steps), "--warmup", str(args.warmup)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
                got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not got:        # a child that failed ends the run: nothing more is started
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit("tagger_bench: the %s child of %s/%s ended with status %d" % (side, trunk, dtype, r.returncode))
                ms[side] += json.loads(got[0][7:])["ms"]
        f, m = statistics.median(ms["fused"]), statistics.median(ms["module"])
        spread = max(ms["module"]) - min(ms["module"])
        accept = f <= m + spread
        ok = ok and accept
        line = ("trunk %-8s %-4s  fused %8.3f [%8.3f .. %8.3f]  module %8.3f [%8.3f .. %8.3f]  fused - module %+7.3f ms (%+.2f %%), "
                "module range %.3f ms: %s" % (trunk, dtype, f, min(ms["fused"]), max(ms["fused"]), m, min(ms["module"]),
                                              max(ms["module"]), f - m, 100.0 * (f - m) / m, spread,
                                              "accepted" if accept else "NOT accepted"))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
