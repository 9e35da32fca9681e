"""Eval-mode ResNet-152 trunk: images/s of `EncoderCaption(...).eval()` forward under no_grad on the fused eval
Bottleneck (scnattn/conv_eval.py: BatchNorm folded into the convolution epilogues) against the module path
(`scnattn.conv.ENABLED = False`: nn.Conv2d on MIOpen + the fused BatchNorm kernels), in one process, alternating,
after warm-up, timed with device events; B = 32 and B = 1 at 3 x 256 x 256, channels_last True and False.  Also the
kernel launches of one Bottleneck forward on each path (torch.profiler device trace).

    python tools/eval_bench.py [--reps 5] [--iters 4]
    python tools/eval_bench.py --bf16                # the same protocol under torch.autocast("cuda", dtype=torch.bfloat16):
                                                     # fused bf16 eval (scnattn/conv_eval16.py), the bf16 module path
                                                     # (conv.ENABLED = False under autocast) and the fused fp32 eval forward
    python tools/eval_bench.py --validate-batch      # one validate() batch (EncoderCaption + EncoderTagger +
                                                     # AttentionSCN, B = 32), for `rocprofv3 --kernel-trace --stats`"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indonesian-image-captioning_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from models.encoders.caption import EncoderCaption  # noqa: E402
from scnattn import conv as SC  # noqa: E402

dev = torch.device("cuda:0")


def timed_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def run_path(fused, fn):
    SC.ENABLED = fused
    try:
        return fn()
    finally:
        SC.ENABLED = True


def launches_per_block(block, x):
    """Device kernels of one forward of `block` on each path (torch.profiler), or None when the trace is unavailable."""
    out = {}
    for fused in (True, False):
        def one():
            with torch.no_grad():
                block(x)
        run_path(fused, one)
        torch.cuda.synchronize()
        try:
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                run_path(fused, one)
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            out[fused] = names
        except Exception as e:  # noqa: BLE001 -- a profiler that cannot attach is reported, not fatal
            out[fused] = None
            print("profiler unavailable: %s" % e, flush=True)
    return out


def bench(args):
    print("eval_bench: EncoderCaption(...).eval() forward under no_grad, 3x256x256, images/s (median of %d rounds x %d "
          "forwards, fused and module path alternating)" % (args.reps, args.iters), flush=True)
    torch.manual_seed(0)
    results = []
    for cl in (True, False):
        enc = EncoderCaption(channels_last=cl).to(dev).eval()
        for B in (32, 1):
            x = torch.randn(B, 3, 256, 256, device=dev)
            t0 = time.time()
            with torch.no_grad():
                for fused in (True, False):       # warm-up (the module path's first call pays MIOpen's solver selection)
                    for _ in range(2):
                        run_path(fused, lambda: enc(x))
            torch.cuda.synchronize()
            warm = time.time() - t0
            ms = {True: [], False: []}
            with torch.no_grad():
                for _ in range(args.reps):
                    for fused in (True, False):
                        ms[fused].append(run_path(fused, lambda: timed_ms(lambda: enc(x), args.iters)))
            with torch.no_grad():
                ya = run_path(True, lambda: enc(x, pooled=False))
                yb = run_path(False, lambda: enc(x, pooled=False))
                diff = ((ya - yb).norm() / yb.norm()).item()
            f, m = statistics.median(ms[True]), statistics.median(ms[False])
            line = ("channels_last=%-5s B=%-2d  fused %8.3f ms  %8.1f img/s | module %8.3f ms  %8.1f img/s | speed-up %.2fx"
                    " | trunk map rel-l2 fused vs module %.1e | warm-up %.1f s" %
                    (cl, B, f, B * 1e3 / f, m, B * 1e3 / m, m / f, diff, warm))
            print(line, flush=True)
            results.append(line)
        del enc
        torch.cuda.empty_cache()
    # launches of one Bottleneck forward (layer3.1 and layer3.0 at B = 32, 256 x 256 input: 16 x 16 maps)
    enc = EncoderCaption(channels_last=True).to(dev).eval()
    for name, idx, cin, H in (("layer3.1", 1, 1024, 16), ("layer3.0", 0, 512, 32)):
        block = enc.resnet[6][idx]
        x = torch.randn(32, cin, H, H, device=dev).contiguous(memory_format=torch.channels_last)
        got = launches_per_block(block, x)
        for fused in (True, False):
            names = got[fused]
            if names is None:
                print("%s %s: launches n/a" % (name, "fused " if fused else "module"), flush=True)
                continue
            print("%s %s: %d kernel launches: %s" % (name, "fused " if fused else "module", len(names),
                                                     ", ".join(n[:60] for n in names)), flush=True)


def bench_bf16(args):
    """Three paths, one process, alternating after warm-up, device events: fused bf16 eval, bf16 module path, fused fp32."""
    print("eval_bench --bf16: EncoderCaption(...).eval() forward under no_grad, 3x256x256, images/s (median of %d rounds x %d "
          "forwards; fused bf16, bf16 module path and fused fp32 alternating)" % (args.reps, args.iters), flush=True)
    torch.manual_seed(0)
    ac = lambda: torch.autocast("cuda", dtype=torch.bfloat16)      # noqa: E731

    def path(kind, enc, x, **kw):
        if kind == "fp32":
            return enc(x, **kw)
        with ac():
            return run_path(kind == "bf16", lambda: enc(x, **kw))

    kinds = ("bf16", "bf16-module", "fp32")
    for cl in (True, False):
        enc = EncoderCaption(channels_last=cl).to(dev).eval()
        for B in (32, 1):
            x = torch.randn(B, 3, 256, 256, device=dev)
            t0 = time.time()
            with torch.no_grad():
                for kind in kinds:       # warm-up (the module path's first call pays MIOpen's solver selection)
                    for _ in range(2):
                        path(kind, enc, x)
            torch.cuda.synchronize()
            warm = time.time() - t0
            ms = {k: [] for k in kinds}
            with torch.no_grad():
                for _ in range(args.reps):
                    for kind in kinds:
                        ms[kind].append(timed_ms(lambda: path(kind, enc, x), args.iters))
                maps = {k: path(k, enc, x, pooled=False) for k in kinds}
            d16 = ((maps["bf16"] - maps["fp32"]).norm() / maps["fp32"].norm()).item()
            dm = ((maps["bf16-module"] - maps["fp32"]).norm() / maps["fp32"].norm()).item()
            t = {k: statistics.median(v) for k, v in ms.items()}
            print("channels_last=%-5s B=%-2d  fused bf16 %8.3f ms %8.1f img/s | bf16 module %8.3f ms %8.1f img/s | fused fp32 %8.3f ms "
                  "%8.1f img/s | bf16 fused vs module %.2fx, vs fused fp32 %.2fx | trunk map rel-l2 vs fused fp32: fused bf16 %.1e, "
                  "bf16 module %.1e | warm-up %.1f s" % (cl, B, t["bf16"], B * 1e3 / t["bf16"], t["bf16-module"], B * 1e3 / t["bf16-module"],
                                                         t["fp32"], B * 1e3 / t["fp32"], t["bf16-module"] / t["bf16"], t["fp32"] / t["bf16"],
                                                         d16, dm, warm), flush=True)
        del enc
        torch.cuda.empty_cache()
    # launches of one Bottleneck forward on bf16 maps (layer3.1 and layer3.0 at B = 32, 256 x 256 input)
    from scnattn import conv16 as C16
    enc = EncoderCaption(channels_last=True).to(dev).eval()
    C16.refresh_weights(enc.resnet)
    for name, idx, cin, H in (("layer3.1", 1, 1024, 16), ("layer3.0", 0, 512, 32)):
        block = enc.resnet[6][idx]
        x = torch.randn(32, cin, H, H, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        with ac():
            got = launches_per_block(block, x)
        for fused in (True, False):
            names = got[fused]
            if names is None:
                print("%s bf16 %s: launches n/a" % (name, "fused " if fused else "module"), flush=True)
                continue
            print("%s bf16 %s: %d kernel launches: %s" % (name, "fused " if fused else "module", len(names),
                                                          ", ".join(n[:60] for n in names)), flush=True)


def validate_batch():
    """One validate() batch through the real EncoderCaption + EncoderTagger (full ResNet-152 trunks, channels-last)
    and an AttentionSCN decoder at B = 32, 256 x 256: the eval path a training run takes once per epoch."""
    from models.decoders.attention_scn import AttentionSCN
    from models.encoders.tagger import EncoderTagger
    from trains.harness import validate
    torch.manual_seed(0)
    enc = EncoderCaption(channels_last=True).to(dev)
    tag = EncoderTagger(semantic_size=1000, channels_last=True).to(dev)
    V, L, B = 1000, 20, 32
    dec = AttentionSCN(512, 512, 512, 512, 1000, V, encoder_dim=2048, dropout=0.5).to(dev)
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(6, L + 1, (B,), generator=g)
    caps = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        n = int(lens[b])
        caps[b, 0] = V - 2
        caps[b, 1:n - 1] = torch.randint(1, V - 3, (n - 2,), generator=g)
        caps[b, n - 1] = V - 1
    allcaps = torch.stack([caps, caps.roll(1, 0)], dim=1)
    batch = (torch.randn(B, 3, 256, 256, generator=g).to(dev), caps.to(dev), lens.unsqueeze(1).to(dev), allcaps.to(dev))
    bleu, loss, top5 = validate([batch], enc, tag, dec, torch.nn.CrossEntropyLoss().to(dev), wm)
    torch.cuda.synchronize()
    print("validate batch: bleu %.4f loss %.4f top5 %.2f" % (bleu, loss, top5), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--validate-batch", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    a = ap.parse_args()
    if a.validate_batch:
        validate_batch()
    elif a.bf16:
        bench_bf16(a)
    else:
        bench(a)
