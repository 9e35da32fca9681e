"""Augmentation in the device loader (csrc/augment.hip, scnattn.augment) against its yardstick and against what a user would
write today.

The case is the train step's batch: 32 images of 3 x 256 x 256 gathered from a resident uint8 set of 256 (seeded random
bytes), channels-last, fp32 and bf16.  Everything is on the device before the clock starts.  Per side a burst of `--burst`
calls between two device events, a warm-up burst and then `--reps` repetitions with the sides interleaved; the figure is
microseconds per call (median and range over the bursts), and for the two kernels the bytes the algorithm needs (1 byte read
and 4 or 2 bytes written per element, the parameter and grey tables aside) over that time.

    (a) gather_normalize          the plain batch: ONE launch, the yardstick (the augmenting kernel reads at most what it
                                  reads and writes exactly what it writes)
    (b) draw + gather_augment     the two launches of an augmented batch; the draw alone and the gather alone as well
    (c) torch ops on the device   the same augmentation as a user would write it: index_select of the uint8 rows, float, / 255,
                                  affine_grid + grid_sample (bilinear, border, align_corners=False) with the flip folded into
                                  theta, the three colour ops element-wise, Normalize, to(dtype, channels_last); the records
                                  are drawn beforehand and are not timed
    (d) one loader epoch          DeviceBatchLoader over a synthetic resident TRAIN split (256 images, 5 captions each, 40
                                  batches of 32) without and with `augment`, wall clock around a device synchronise; and the
                                  one-off mean-grey pass over the resident set

and the largest |(b) - (c)| so that the two are seen to compute the same thing.  Needs an MI355X.

    python tools/augment_bench.py [--reps 7] [--burst 200] [--out profiles/augment_bench.txt]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indonesian-image-captioning_amd"))
sys.path.insert(0, ROOT)

NSRC, BATCH, SIDE, CPI = 256, 32, 256, 5


def _fmt(name, us, nbytes=None):
    s = "%-58s median %9.2f us  [%9.2f .. %9.2f]  n = %d" % (name, statistics.median(us), min(us), max(us), len(us))
    if nbytes:
        s += "   %6.0f GB/s of needed bytes" % (nbytes / statistics.median(us) * 1e-3)
    return s


def torch_augment(src, rows, params, grey, mean, std, dtype):
    """the record's semantics in torch ops (fp32), channels-last output"""
    import torch
    import torch.nn.functional as F
    n, H, W = rows.numel(), src.shape[2], src.shape[3]
    x = src.index_select(0, rows).float() / 255.0
    x0, y0, w, h, flip, bright, contr, sat = params.unbind(1)
    sgn = 1.0 - 2.0 * flip
    theta = torch.zeros(n, 2, 3, device=src.device)
    theta[:, 0, 0] = sgn * w / W                    # normalised coordinates: gx_src = (2 x0 + w) / W - 1 + (w / W) gx_out
    theta[:, 0, 2] = (2.0 * x0 + w) / W - 1.0
    theta[:, 1, 1] = h / H
    theta[:, 1, 2] = (2.0 * y0 + h) / H - 1.0
    grid = F.affine_grid(theta, (n, 3, H, W), align_corners=False)
    v = F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)
    b, c, s = (t.view(n, 1, 1, 1) for t in (bright, contr, sat))
    v = (b * v).clamp(0.0, 1.0)
    m = (b * grey.index_select(0, rows).view(n, 1, 1, 1)).clamp(max=1.0)
    v = (c * v + (1.0 - c) * m).clamp(0.0, 1.0)
    g = 0.299 * v[:, 0:1] + 0.587 * v[:, 1:2] + 0.114 * v[:, 2:3]
    v = (s * v + (1.0 - s) * g).clamp(0.0, 1.0)
    v = (v - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)
    return v.to(dtype=dtype, memory_format=torch.channels_last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scnattn import augment as A
    from scnattn import data as SD
    from scnattn import h5lite
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs an MI355X; nothing is measured without one")
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    u8 = rng.randint(0, 256, size=(NSRC, 3, SIDE, SIDE)).astype(np.uint8)
    src = torch.from_numpy(u8).to(dev)
    rows = torch.from_numpy(rng.randint(0, NSRC, size=BATCH).astype(np.int64)).to(dev)
    sid = torch.from_numpy(rng.randint(0, NSRC * CPI, size=BATCH).astype(np.int64)).to(dev)
    lut = torch.from_numpy(SD.normalize_lut()).to(dev)
    mean, std = torch.tensor(SD.IMAGENET_MEAN, device=dev), torch.tensor(SD.IMAGENET_STD, device=dev)
    aug = A.Augment(seed=1)
    grey = A.mean_grey(src)
    params = aug.draw(sid, 0, SIDE, SIDE)
    lines = ["augment_bench: %d repetitions of a burst of %d calls after one warm-up burst, device events around a burst, sides "
             "interleaved; batch %d x 3 x %d x %d from %d resident images, channels-last; Augment() defaults"
             % (args.reps, args.burst, BATCH, SIDE, SIDE, NSRC)]

    def burst(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.burst):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.burst

    for dtype in (torch.float32, torch.bfloat16):
        esz = 4 if dtype == torch.float32 else 2
        need = BATCH * 3 * SIDE * SIDE * (1 + esz)
        out = torch.empty((BATCH, 3, SIDE, SIDE), device=dev, dtype=dtype, memory_format=torch.channels_last)
        sides = [
            ("(a) gather_normalize: one launch", lambda: SD.gather_normalize(src, rows, lut, dtype=dtype, channels_last=True, out=out), need),
            ("(b) draw + gather_augment: two launches",
             lambda: A.gather_augment(src, rows, aug.draw(sid, 0, SIDE, SIDE), SD.IMAGENET_MEAN, SD.IMAGENET_STD, grey=grey,
                                      dtype=dtype, channels_last=True, out=out), need),
            ("    the draw alone", lambda: aug.draw(sid, 0, SIDE, SIDE), None),
            ("    gather_augment alone", lambda: A.gather_augment(src, rows, params, SD.IMAGENET_MEAN, SD.IMAGENET_STD, grey=grey,
                                                                  dtype=dtype, channels_last=True, out=out), need),
            ("    gather_augment alone, identity records", lambda ip=A.identity_params(BATCH, SIDE, SIDE, dev): A.gather_augment(
                src, rows, ip, SD.IMAGENET_MEAN, SD.IMAGENET_STD, grey=grey, dtype=dtype, channels_last=True, out=out), need),
            ("(c) torch ops: index_select, grid_sample, colour ops", lambda: torch_augment(src, rows, params, grey, mean, std, dtype), None),
        ]
        times = [[] for _ in sides]
        for rep in range(args.reps + 1):
            for k, (_, fn, _) in enumerate(sides):
                t = burst(fn)
                if rep:
                    times[k].append(t)
        lines.append("-- %s" % str(dtype).replace("torch.", ""))
        for (name, _, nbytes), t in zip(sides, times):
            lines.append(_fmt(name, t, nbytes))
        med = [statistics.median(t) for t in times]
        lines.append("    medians over (a): (b) %.2fx, gather_augment alone %.2fx, torch ops %.2fx" % (med[1] / med[0], med[3] / med[0], med[5] / med[0]))
        ours = A.gather_augment(src, rows, params, SD.IMAGENET_MEAN, SD.IMAGENET_STD, grey=grey, dtype=dtype, channels_last=True)
        theirs = torch_augment(src, rows, params, grey, mean, std, dtype)
        lines.append("    largest |(b) - (c)| over the batch: %.3e (values within [%.2f, %.2f])"
                     % (float((ours.float() - theirs.float()).abs().max()), float(ours.float().min()), float(ours.float().max())))

    # (d) a loader epoch over a resident split
    with tempfile.TemporaryDirectory() as d:
        base = "bench_5_cap_per_img_5_min_word_freq"
        h5lite.write_arrays(os.path.join(d, "TRAIN_IMAGES_%s.hdf5" % base), {"images": u8}, {"captions_per_image": CPI})
        json.dump(rng.randint(1, 50, size=(NSRC * CPI, 12)).tolist(), open(os.path.join(d, "TRAIN_CAPTIONS_%s.json" % base), "w"))
        json.dump(rng.randint(3, 13, size=NSRC * CPI).tolist(), open(os.path.join(d, "TRAIN_CAPLENS_%s.json" % base), "w"))
        loaders = [("(d) loader epoch, augment=None", SD.DeviceBatchLoader(d, base, "TRAIN", BATCH, dev, cpi=CPI, seed=0, resident=True)),
                   ("(d) loader epoch, augment=Augment()", SD.DeviceBatchLoader(d, base, "TRAIN", BATCH, dev, cpi=CPI, seed=0, resident=True,
                                                                                augment=aug))]
        times = [[] for _ in loaders]
        for rep in range(args.reps + 1):
            for k, (_, ld) in enumerate(loaders):
                ld.set_epoch(rep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for batch in ld:
                    pass
                torch.cuda.synchronize()
                if rep:
                    times[k].append((time.perf_counter() - t0) * 1e6 / len(ld))
        lines.append("-- one epoch of %d batches of %d over a resident split of %d images, fp32 channels-last, wall clock around a "
                     "device synchronise, per batch (images, captions and lengths; nothing consumes them)" % (len(loaders[0][1]), BATCH, NSRC))
        for (name, _), t in zip(loaders, times):
            lines.append(_fmt(name, t))
        g = []
        for rep in range(args.reps + 1):
            t = burst(lambda: A.mean_grey(src))
            if rep:
                g.append(t)
        lines.append(_fmt("    mean_grey over the %d resident images (one-off)" % NSRC, g, NSRC * 3 * SIDE * SIDE))
    lines.append("not measured: staged mode under PCIe load, other image sizes, the effect on a full train step")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
