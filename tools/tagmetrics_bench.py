"""Tagger evaluation on the device (csrc/tagmetrics.hip, scnattn.tagmetrics.TagScorer) against two other ways to the same numbers.

Synthetic validation passes of n = 5000 and n = 40 000 images, S = 1000 tags, batches of 32, about 1 % positives (seeded;
positives score higher than negatives on average, scores are distinct fp32 draws).  The probabilities and targets of every
batch are on the device before the clock starts, as they are after the tagger's forward pass.  Per size, wall clock around a
device synchronise, a warm-up and then repetitions, median and range, the three sides interleaved:

    TagScorer                 all update() calls plus result() (one launch per batch, two at the end, one download);
                              the update() calls and result() also on their own
    (a) torch on the device   the batches copied into one [n, S] tensor, then torch.sort per column and per row + cumsum,
                              ties resolved to the end of their group (flip / cummin / gather): tag mAP, per-image AP,
                              precision / recall at k, micro / macro P, R, F1, binary accuracy; one download
    (b) host                  download of the [n, S] tensors plus tagmetrics_refs.reference_fp64 (numpy, one thread)

and the values of the three sides next to each other.  Needs an MI355X.

    python tools/tagmetrics_bench.py [--reps 5] [--warmup 1] [--host-reps 1] [--sizes 5000,40000] [--out profiles/tagmetrics_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "indonesian-image-captioning_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

S, BATCH, RATE = 1000, 32, 0.01
KS, THRESHOLDS = (1, 5, 10, 20), (0.5,)


def _fmt(name, ms):
    return "%-58s median %10.3f ms  [%10.3f .. %10.3f]  n = %d" % (name, statistics.median(ms), min(ms), max(ms), len(ms))


def make_pass(n, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(n)
    t = (torch.rand(n, S, generator=g) < RATE)
    p = torch.rand(n, S, generator=g)
    p = torch.where(t, p.sqrt(), p * p)
    p, t = p.to(dev), t.float().to(dev)
    return [(p[a:a + BATCH], t[a:a + BATCH]) for a in range(0, n, BATCH)]


def torch_ap(s, pos, dim):
    """tie-invariant AP along `dim` by sorting: (ap fp64, npos) with ap = 0 where npos = 0"""
    import torch
    if dim == 0:
        s, pos = s.t(), pos.t()
    s, order = torch.sort(s, dim=1, descending=True, stable=True)
    lab = pos.gather(1, order)
    L = s.shape[1]
    idx = torch.arange(L, device=s.device).expand_as(s)
    last = torch.ones_like(lab)
    last[:, :-1] = s[:, :-1] != s[:, 1:]
    end = torch.where(last, idx, torch.full_like(idx, L)).flip(1).cummin(1)[0].flip(1)       # index of the end of my tie group
    tp = lab.long().cumsum(1).gather(1, end)
    npos = lab.sum(1)
    ap = (lab * (tp.double() / (end + 1).double())).sum(1) / npos.clamp_min(1).double()
    return ap, npos, lab


def torch_side(batches, dev):
    import torch
    n = sum(p.shape[0] for p, _ in batches)
    P, T = torch.empty(n, S, device=dev), torch.empty(n, S, device=dev)
    a = 0
    for p, t in batches:
        P[a:a + p.shape[0]], T[a:a + p.shape[0]] = p, t
        a += p.shape[0]
    pos = T >= 0.5
    ap_t, np_t, _ = torch_ap(P, pos, 0)
    ap_i, np_i, lab = torch_ap(P, pos, 1)
    vt, vi = np_t > 0, np_i > 0
    hits = lab.long().cumsum(1)[:, [k - 1 for k in KS]].double()
    out = [ap_t[vt].mean(), ap_i[vi].mean()]
    out += [(hits[vi, q] / k).mean() for q, k in enumerate(KS)] + [(hits[vi, q] / np_i[vi].double()).mean() for q in range(len(KS))]
    for th in THRESHOLDS:
        pred = P >= th
        tp, fp, fn = (pred & pos).sum(0).double(), (pred & ~pos).sum(0).double(), (~pred & pos).sum(0).double()
        z = torch.zeros((), dtype=torch.float64, device=dev)

        def div(x, y):
            return torch.where(y > 0, x / y.clamp_min(1), z)

        out += [div(tp.sum(), (tp + fp).sum()), div(tp.sum(), (tp + fn).sum()), div(2 * tp.sum(), (2 * tp + fp + fn).sum()),
                div(tp, tp + fp)[vt].mean(), div(tp, tp + fn)[vt].mean(), div(2 * tp, 2 * tp + fp + fn)[vt].mean()]
    out.append(100.0 * ((P >= 0.5) == pos).sum().double() / (n * S))
    v = torch.stack([x.double() for x in out]).cpu().tolist()
    res = {"map_tags": v[0], "ap_images": v[1], "precision_at": dict(zip(KS, v[2:6])), "recall_at": dict(zip(KS, v[6:10])),
           "binary_accuracy": v[-1]}
    for q, th in enumerate(THRESHOLDS):
        res["threshold_%g" % th] = dict(zip(("micro_precision", "micro_recall", "micro_f1", "macro_precision", "macro_recall",
                                             "macro_f1"), v[10 + 6 * q:16 + 6 * q]))
    return res


def host_side(batches):
    import torch
    import tagmetrics_refs as R
    P = torch.cat([p for p, _ in batches]).cpu().numpy()
    T = torch.cat([t for _, t in batches]).cpu().numpy()
    return R.reference_fp64(P, T, KS, THRESHOLDS)


def flat(res):
    out = [("map_tags", res["map_tags"]), ("ap_images", res["ap_images"])]
    out += [("P@%d" % k, res["precision_at"][k]) for k in KS] + [("R@%d" % k, res["recall_at"][k]) for k in KS]
    for th in THRESHOLDS:
        out += [("%s@%g" % (k, th), v) for k, v in sorted(res["threshold_%g" % th].items())]
    return out + [("binary_accuracy", res["binary_accuracy"])]


def one_size(n, dev, args):
    import torch
    from scnattn.tagmetrics import TagScorer
    batches = make_pass(n, dev)
    sync = torch.cuda.synchronize
    sc = TagScorer(S, n, ks=KS, thresholds=THRESHOLDS, device=dev)

    def ours():
        sc.reset()
        for p, t in batches:
            sc.update(p, t)
        return sc.result()

    ms = {"ours": [], "updates": [], "result": [], "torch": [], "host": []}
    res = {}
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        sync()
        t0 = time.perf_counter()
        res["ours"] = ours()
        sync()
        t1 = time.perf_counter()
        res["torch"] = torch_side(batches, dev)
        sync()
        t2 = time.perf_counter()
        sc.reset()
        sync()
        t3 = time.perf_counter()
        for p, t in batches:
            sc.update(p, t)
        sync()
        t4 = time.perf_counter()
        sc.result()
        sync()
        t5 = time.perf_counter()
        if keep:
            for k, v in (("ours", t1 - t0), ("torch", t2 - t1), ("updates", t4 - t3), ("result", t5 - t4)):
                ms[k].append(1e3 * v)
    for i in range(args.host_reps):
        t0 = time.perf_counter()
        res["host"] = host_side(batches)
        ms["host"].append(1e3 * (time.perf_counter() - t0))
    lines = ["-- n = %d images, S = %d, %d batches of %d, %.1f %% positives" % (n, S, len(batches), BATCH, 100 * RATE)]
    lines.append(_fmt("TagScorer: %d x update() + result()" % len(batches), ms["ours"]))
    lines.append(_fmt("    the update() calls alone (row kernel, store)", ms["updates"]))
    lines.append(_fmt("    result() alone (column kernel, finalize, download)", ms["result"]))
    lines.append(_fmt("(a) torch on the device: copy, 2 sorts, cumsum, download", ms["torch"]))
    if ms["host"]:
        lines.append(_fmt("(b) host: download + numpy reference_fp64, one thread", ms["host"]))
    a = statistics.median(ms["ours"])
    lines.append("    medians over TagScorer's: torch %.2fx%s" % (statistics.median(ms["torch"]) / a, (
        ", host %.1fx" % (statistics.median(ms["host"]) / a)) if ms["host"] else ""))
    for side in ("ours", "torch", "host"):
        if side in res:
            lines.append("values %-6s " % side + "  ".join("%s %.9f" % kv for kv in flat(res[side])))
    for side in ("torch", "host"):
        if side in res:
            worst = max(abs(x - y) for (_, x), (_, y) in zip(flat(res["ours"]), flat(res[side])))
            lines.append("largest |TagScorer - %s| over the %d values: %.3g" % (side, len(flat(res["ours"])), worst))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--sizes", default="5000,40000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tagmetrics_bench: needs an MI355X; there is nothing to measure without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    lines = ["tagmetrics_bench: %d repetitions after %d warm-up rounds on the device sides, %d on the host side; wall clock around a "
             "device synchronise; inputs on the device before the clock starts" % (args.reps, args.warmup, args.host_reps)]
    for n in (int(x) for x in args.sizes.split(",")):
        lines += one_size(n, dev, args)
        for ln in lines[-12:]:
            print(ln, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
