"""Attention overlays: the device path next to the host path it replaces.

    python tools/overlay_bench.py [--images 32] [--maps 12] [--repeats 9] [--part device|host ...] [--out profiles/NAME.txt]

Workload: `--images` RGB photographs of 375 x 500 (random bytes, one seed) with `--maps` 14 x 14 attention maps each (map 0
the row of ones, the others softmax of scaled normal draws) -> per map one 336 x 336 x 3 uint8 overlay.

device   `scnattn.viz.attention_overlays`.  Figures, each the median of `--repeats` windows after a warm-up window:
           resize    the LANCZOS launch alone on an uploaded batch (between two device events);
           overlay   the two overlay launches alone, photographs and maps on the device, in both forms -- the blend
                     recomputing the smoothed map, or reading back the fp32 maps the first launch stored (device events;
                     bytes = photograph bytes read per map + overlay bytes written + the fp32 maps written and read, over
                     that time, as a share of the 8 TB/s HBM peak; the timed window includes the small index / weight copy);
           expand    the expand launch alone, without and with the fp32 maps stored -- what a form that keeps S in memory
                     instead of recomputing it would at least add is the difference, plus reading it back;
           end2end   numpy arrays in, overlays on the device (host clock around a synchronise): packing, the copies, the
                     three launches.
host     per image `PIL.Image.resize((336, 336), LANCZOS)`, per map `scipy.ndimage.zoom(order=1, mode='mirror',
         grid_mode=True)` + `gaussian_filter(8, mode='reflect', truncate=4.0)` and the numpy blend with the same rounding,
         images spread over 1 and 16 threads; skipped if Pillow or scipy is missing.
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

SOURCE, SIZE, MAP, UPSCALE, SIGMA, WEIGHT = (375, 500), (336, 336), (14, 14), 24, 8, 0.8
HBM_PEAK = 8.0e12      # bytes/s


def workload(n_images, n_maps, seed=0):
    rng = np.random.RandomState(seed)
    imgs = [rng.randint(0, 256, size=SOURCE + (3,)).astype(np.uint8) for _ in range(n_images)]
    z = rng.randn(n_images, n_maps, MAP[0] * MAP[1]) * 2.0
    e = np.exp(z - z.max(axis=2, keepdims=True))
    maps = (e / e.sum(axis=2, keepdims=True)).astype(np.float32).reshape((n_images, n_maps) + MAP)
    maps[:, 0] = 1.0
    return imgs, list(maps)


def emit(lines, **kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


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


def part_device(args, lines):
    import torch
    from scnattn import data as SD
    from scnattn import viz
    assert torch.cuda.is_available(), "overlay_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    imgs, maps = workload(args.images, args.maps)
    n = args.images * args.maps
    packed = SD.pack_images(imgs, SIZE, filter="lanczos")
    up = SD.upload_images(packed, dev)
    ms = event_ms(torch, lambda: SD.resize_uploaded(packed, up), args.repeats)
    emit(lines, part="device", figure="resize", images=args.images, **summary(ms))
    photos = SD.resize_uploaded(packed, up)
    a = torch.from_numpy(np.concatenate(maps)).to(dev)
    idx = np.repeat(np.arange(args.images, dtype=np.int32), args.maps)
    beta = np.tile(np.asarray([0.0] + [WEIGHT] * (args.maps - 1), np.float32), args.images)
    for recompute in (True, False):
        ms = event_ms(torch, lambda: viz.overlay_maps(photos, a, idx, beta, UPSCALE, SIGMA, recompute=recompute), args.repeats)
        moved = n * SIZE[0] * SIZE[1] * (3 * 2 + (0 if recompute else 8))
        med = statistics.median(ms)
        emit(lines, part="device", figure="overlay", form="recompute" if recompute else "stored maps", maps=n, launches=2,
             bytes_moved=moved, tb_per_s=round(moved / (med * 1e-3) / 1e12, 3),
             share_of_hbm_peak=round(moved / (med * 1e-3) / HBM_PEAK, 4), **summary(ms))
    for store in (False, True):
        ms = event_ms(torch, lambda: viz._expand(a, UPSCALE, SIGMA, store, False), args.repeats)
        emit(lines, part="device", figure="expand", maps=n, stores_fp32_maps=store, **summary(ms))
    ms = []
    viz.attention_overlays(imgs, maps)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        viz.attention_overlays(imgs, maps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    emit(lines, part="device", figure="end2end", images=args.images, maps=n,
         maps_per_s=round(n * 1e3 / statistics.median(ms), 1), **summary(ms))


def part_host(args, lines):
    try:
        import PIL
        import scipy
        import scipy.ndimage as ndi
        from PIL import Image
    except ImportError:
        emit(lines, part="host", available=False)
        return
    from concurrent.futures import ThreadPoolExecutor
    imgs, maps = workload(args.images, args.maps)
    n = args.images * args.maps

    def one(k):
        photo = np.asarray(Image.fromarray(imgs[k]).resize((SIZE[1], SIZE[0]), resample=Image.LANCZOS)).astype(np.float32)
        out = np.empty((args.maps,) + SIZE + (3,), np.uint8)
        for t in range(args.maps):
            s = ndi.gaussian_filter(ndi.zoom(maps[k][t].astype(np.float64), UPSCALE, order=1, mode="mirror", grid_mode=True),
                                    SIGMA, mode="reflect", truncate=4.0)
            lo, hi = s.min(), s.max()
            norm = np.clip((s - lo) / (hi - lo), 0, 1) if hi > lo else np.zeros_like(s)
            b = 0.0 if t == 0 else WEIGHT
            out[t] = np.minimum((1 - b) * photo + (b * 255 * norm)[:, :, None] + 0.5, 255).astype(np.uint8)
        return out

    for threads in (1, 16):
        pool = ThreadPoolExecutor(threads) if threads > 1 else None
        run = (lambda: list(pool.map(one, range(args.images)))) if pool else (lambda: [one(k) for k in range(args.images)])
        run()
        ms = []
        for _ in range(args.host_repeats):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        if pool:
            pool.shutdown()
        emit(lines, part="host", pillow=PIL.__version__, scipy=scipy.__version__, threads=threads, images=args.images, maps=n,
             maps_per_s=round(n * 1e3 / statistics.median(ms), 1), **summary(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--maps", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--part", action="append", choices=["device", "host"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for part in args.part or ["device", "host"]:
        {"device": part_device, "host": part_host}[part](args, lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/overlay_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
