"""Image resize throughput and the Captioner end to end.

    python tools/resize_bench.py [--images 32] [--repeats 9] [--part resize|pillow|captioner ...] [--out profiles/NAME.txt]

resize     `resize_normalize` at B = 32, 256 x 256 target, channels-last fp32 and bf16, for 375 x 500 and 480 x 640 RGB
           sources (random bytes, one seed).  Three figures per case, each the median of `--repeats` windows after a
           warm-up window, a window between two device events:
             kernel   `--inner` back-to-back launches on an uploaded batch (time / launches; bytes = source bytes read
                      once + output bytes written, over that time; share of the 8 TB/s HBM peak);
             upload   one host-to-device copy of the packed batch + one launch;
             packed   `pack_images` on the host + the copy + the launch (host clock around a synchronise).
pillow     `PIL.Image.resize((256, 256), BILINEAR)` on the same arrays, 1 thread and 16 threads, if Pillow is importable;
           the host column stays empty otherwise.
captioner  `Captioner(EncoderCaption, AttentionSCN, tagger=EncoderTagger)` at the train step's widths on 32 images of
           375 x 500, fp32 and bf16 trunks, from numpy arrays to records, next to its parts timed alone in the same
           process: resize_normalize, the caption trunk, the tagger trunk, sample_batch.
Prints one JSON line per figure.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "indonesian-image-captioning_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SOURCES = ((375, 500), (480, 640))
SIZE = (256, 256)
HBM_PEAK = 8.0e12      # bytes/s


def images_of(shape, n, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=shape + (3,)).astype(np.uint8) for _ in range(n)]


def emit(lines, **kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


def event_ms(torch, fn, repeats):
    fn()                                              # warm-up window: code objects, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def host_ms(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def part_resize(args, lines):
    import torch
    from scnattn import data as SD
    assert torch.cuda.is_available(), "resize_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    lut = torch.from_numpy(SD.normalize_lut()).to(dev)
    B = args.images
    for shape in SOURCES:
        imgs = images_of(shape, B)
        packed = SD.pack_images(imgs, SIZE)
        up = SD.upload_images(packed, dev)
        src_bytes = B * shape[0] * shape[1] * 3
        for dtype in (torch.float32, torch.bfloat16):
            out_bytes = B * 3 * SIZE[0] * SIZE[1] * (4 if dtype == torch.float32 else 2)
            name = "%dx%d %s channels-last" % (shape + (str(dtype).split(".")[1],))

            def kernel():
                for _ in range(args.inner):
                    SD.resize_uploaded(packed, up, lut, dtype=dtype, channels_last=True)

            ms = [m / args.inner for m in event_ms(torch, kernel, args.repeats)]
            med = statistics.median(ms)
            emit(lines, part="resize", figure="kernel", case=name, images=B, launches_per_window=args.inner,
                 images_per_s=round(B * 1e3 / med, 1), bytes_moved=src_bytes + out_bytes,
                 tb_per_s=round((src_bytes + out_bytes) / (med * 1e-3) / 1e12, 3),
                 share_of_hbm_peak=round((src_bytes + out_bytes) / (med * 1e-3) / HBM_PEAK, 4), **summary(ms))
            ms = event_ms(torch, lambda: SD.resize_normalize(packed, lut, SIZE, dtype=dtype, channels_last=True), args.repeats)
            emit(lines, part="resize", figure="upload", case=name, images=B,
                 images_per_s=round(B * 1e3 / statistics.median(ms), 1), **summary(ms))
            ms = host_ms(torch, lambda: SD.resize_normalize(imgs, lut, SIZE, dtype=dtype, channels_last=True), args.repeats)
            emit(lines, part="resize", figure="packed", case=name, images=B,
                 images_per_s=round(B * 1e3 / statistics.median(ms), 1), **summary(ms))


def part_pillow(args, lines):
    try:
        import PIL
        from PIL import Image
    except ImportError:
        emit(lines, part="pillow", available=False)
        return
    from concurrent.futures import ThreadPoolExecutor
    B = args.images

    def one(im):
        return np.asarray(Image.fromarray(im).resize((SIZE[1], SIZE[0]), resample=2))

    for shape in SOURCES:
        imgs = images_of(shape, B)
        for threads in (1, 16):
            pool = ThreadPoolExecutor(threads) if threads > 1 else None
            run = (lambda: list(pool.map(one, imgs))) if pool else (lambda: [one(im) for im in imgs])
            run()
            ms = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                run()
                ms.append((time.perf_counter() - t0) * 1e3)
            if pool:
                pool.shutdown()
            emit(lines, part="pillow", version=PIL.__version__, case="%dx%d" % shape, threads=threads, images=B,
                 images_per_s=round(B * 1e3 / statistics.median(ms), 1), **summary(ms))


def part_captioner(args, lines):
    import torch
    from models.decoders.attention_scn import AttentionSCN
    from models.encoders.caption import EncoderCaption
    from models.encoders.tagger import EncoderTagger
    from scnattn import data as SD
    from scnattn.inference import Captioner
    assert torch.cuda.is_available(), "resize_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, E, S, B = 10000, 2048, 1000, args.images
    dec = AttentionSCN(512, 512, 512, 512, S, V, encoder_dim=E, dropout=0.0)
    with torch.no_grad():                             # as tools/beam_bench.py: searches that end at mixed lengths
        dec.fc.weight.mul_(10.0)
        dec.fc.bias[V - 1] += 2.0
    dec = dec.to(dev).eval()
    enc = EncoderCaption(channels_last=True).to(dev).eval()
    tag = EncoderTagger(semantic_size=S, channels_last=True).to(dev).eval()
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    wm.update(("w%d" % i, i) for i in range(1, V - 3))
    imgs = images_of(SOURCES[0], B)
    for dtype in (torch.float32, torch.bfloat16):
        name = str(dtype).split(".")[1]
        cap = Captioner(enc, dec, wm, tagger=tag, beam_size=5, dtype=dtype)
        ms = host_ms(torch, lambda: cap(imgs), args.repeats)
        emit(lines, part="captioner", figure="end_to_end", trunk=name, images=B, source="375x500",
             captions_per_s=round(B * 1e3 / statistics.median(ms), 1), **summary(ms))
        ac = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)      # noqa: E731
        with torch.no_grad():
            batch = cap.images_to_batch(imgs)
            with ac():
                eo, tg = enc(batch).float(), tag(batch).float()

            def trunk(m):
                with ac():
                    return m(batch)

            parts = {"resize_normalize": host_ms(torch, lambda: cap.images_to_batch(imgs), args.repeats),
                     "caption_trunk": host_ms(torch, lambda: trunk(enc), args.repeats),
                     "tagger_trunk": host_ms(torch, lambda: trunk(tag), args.repeats),
                     "sample_batch": host_ms(torch, lambda: dec.sample_batch(5, wm, eo, tg), args.repeats)}
        total = 0.0
        for k, v in parts.items():
            total += statistics.median(v)
            emit(lines, part="captioner", figure=k, trunk=name, images=B, **summary(v))
        emit(lines, part="captioner", figure="sum_of_parts", trunk=name, images=B, median_ms=round(total, 4),
             end_to_end_over_sum=round(statistics.median(ms) / total, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--part", action="append", choices=["resize", "pillow", "captioner"])
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    for part in args.part or ["resize", "pillow", "captioner"]:
        {"resize": part_resize, "pillow": part_pillow, "captioner": part_captioner}[part](args, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/resize_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
