#!/usr/bin/env python
"""bench.py -- images/sec of one train step of the SCN+Attention captioner on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N=1 default.  With N>1 the script may be started either way: under ``python -m torch.distributed.run
--nproc-per-node N`` (one rank per GPU, RANK/LOCAL_RANK/WORLD_SIZE in the environment), or bare -- then it starts
that launcher itself as a CHILD process before anything touches the GPU, relays rank 0's JSON line and exits with
the child's status.  A rank whose WORLD_SIZE differs from --gpus refuses to run.

A "step" = trains/attention_scn.py:212-252 on one synthetic batch per rank (32 images 256x256, 52-token
captions, 1000 tags, V=10000, fp32): ResNet-152 encoder fwd (fine-tuning layer2-4) -> AttentionSCN
decoder fwd -> loss -> zero_grad -> backward (+ RCCL gradient all-reduce when N>1) -> clamp +-5 -> Adam.
Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline (`value` images/sec, `ms_per_step`).
--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step returned to its caller as .npy
files (see dump_outputs); inputs and weights are seeded, so two builds can be compared file for file.
--full: also everything that costs runs of its own or extra timing (per-step HIP events and the median step,
allocator statistics, the decode step's roofline, the trunk's roofline, the reference's literal call sequence as a
second figure, the CPU baseline), added to the same JSON line:
  roofline     -- the per-timestep decode kernel group (the "fused SCN-cell + attention step" of
                  north_star; 7 launches per step in this round): algorithmic bytes per step
                  (enc + att1 + recurrent weights) / average step duration measured with
                  HIP events recorded by the library on the launch stream, against HBM peak 8 TB/s.
  cpu_baseline -- the CPU oracle (op-for-op restatement of the reference, oracle/scnattn_ref.py) timed
                  on the host cores on a bounded sample (rank 0, N=1 only).
"""
import argparse
import ctypes
import json
import os

# kernel arguments in device memory: measured 44.0 vs 54.2 us per decode step (the image sets it; keep it set)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")

import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(ROOT, "indonesian-image-captioning_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

LAUNCH_FLOOR_US = 1.87     # see roofline.launch_floor
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK_TF = 157.3   # fp32-input matrix peak (v_mfma_f32_32x32x2_f32 at 2.4 GHz), same guide
MFMA_BF16_PEAK_TF = 2500.0 # dense bf16 matrix peak
ENC_GFLOP_PER_IMAGE = {True: 86.1, False: 30.07}    # ResNet-152 trunk fwd + bwd of layer2-4 / fwd only


def step_bytes(cfg, B, P=196, E=2048):
    """Algorithmic fp32 bytes one forward decode step must move at batch B:
    enc (B,P,E) + att1 (B,P,A) + recurrent weights (decoder_att, f_beta, weight_ia[M:], weight_ic/ha/hc)."""
    A, D, F = cfg["attention_dim"], cfg["decoder_dim"], cfg["factored_dim"]
    weights = D * A + D * E + E * 4 * F + 3 * D * 4 * F
    return 4 * (B * P * E + B * P * A + weights)


def cpu_baseline(kind, cfg, fine_tune, batch, budget_s=20.0):
    """Time the CPU oracle on a bounded sample of the SAME step: full train steps at the metric's batch size, full
    sequence length / vocabulary / model size, one untimed warm-up step then as many timed steps as fit ~budget_s
    (at least 2); images/sec = B * steps / time."""
    from oracle import scnattn_ref as R
    from scnattn.resnet import resnet152_trunk
    from trains.harness import build_decoder, synthetic_batch
    # the GPU box exposes every host core but grants a 16-core share per GPU: more threads than that
    # only oversubscribes
    try:
        ncores = len(os.sched_getaffinity(0))
    except AttributeError:
        ncores = os.cpu_count() or 1
    ncores = max(1, min(ncores, 16))
    torch.set_num_threads(ncores)
    torch.manual_seed(0)
    Bc = batch
    dec = build_decoder(kind, dict(cfg, dropout=0.0))
    P = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    trunk = resnet152_trunk().train()
    for i, child in enumerate(trunk.children()):
        for p in child.parameters():
            p.requires_grad = bool(fine_tune and i >= 5)
    enc_opt = torch.optim.Adam([p for p in trunk.parameters() if p.requires_grad], lr=cfg["encoder_lr"]) \
        if fine_tune else None
    imgs, tags, caps, caplens = synthetic_batch(Bc, cfg["vocab_size"], cfg["max_len"], cfg["image_size"],
                                                cfg["semantic_dim"], "cpu", 99)
    opt_state = {}

    def one_step(step_no):
        feat = trunk(imgs)
        enc = R.pool_permute(feat, 14)
        enc_leaf = enc.detach().requires_grad_(fine_tune)
        _, _, denc = R.decoder_train_step(kind, P, enc_leaf, tags, caps, caplens, opt_state, step_no, lr=cfg["decoder_lr"],
                                          grad_clip=cfg["grad_clip"], alpha_c=cfg["alpha_c"],
                                          enc_requires_grad=fine_tune)
        if fine_tune:
            enc_opt.zero_grad()
            enc.backward(denc)
            for p in trunk.parameters():
                if p.grad is not None:
                    p.grad.clamp_(-cfg["grad_clip"], cfg["grad_clip"])
            enc_opt.step()

    one_step(1)                                   # warm-up: allocator, thread pool, oneDNN primitive caches
    steps, t0 = 0, time.perf_counter()
    while steps < 2 or (time.perf_counter() - t0 < budget_s and steps < 64):
        steps += 1
        one_step(steps + 1)
    dt = time.perf_counter() - t0
    return {"value": round(Bc * steps / dt, 4), "unit": "images/sec", "cores": ncores, "kind": "port",
            "sample": "%d full train steps (encoder%s + un-hoisted %s decoder, T=%d, V=%d) at batch %d in %.1f s after "
                      "one warm-up step, torch CPU fp32 with %d threads"
                      % (steps, " fine-tune" if fine_tune else " frozen", kind, cfg["max_len"] + 1, cfg["vocab_size"],
                         Bc, dt, ncores)}


def dump_outputs(d, ts, loss, fwd, k=1 << 20):
    """--dump-outputs D: what the last timed step handed its caller, one float32 D/<name>.npy per array.  A train step
    returns the loss and leaves the model state it updated: each optimizer's parameters and gradients (decoder_*,
    encoder_* when fine-tuning), taken in parameter order, row-major, as one fixed seeded sample of k elements (the
    same positions for parameters and gradients).  --forward-only: the decoder's scores (and alphas), sampled alike.
    At most 4 arrays of k floats: 16 MiB."""
    import numpy as np
    os.makedirs(d, exist_ok=True)

    def sample(tensors):
        flat = torch.cat([t.detach().reshape(-1).float() for t in tensors])
        if flat.numel() > k:
            idx = np.sort(np.random.default_rng(0).choice(flat.numel(), k, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        return flat.cpu().numpy()

    arrays = {}
    if fwd is not None:
        arrays["scores"] = sample([fwd[0]])
        if len(fwd) == 5:                       # (scores, caps_sorted, decode_lengths, alphas, sort_ind)
            arrays["alphas"] = sample([fwd[3]])
    else:
        arrays["loss"] = loss.detach().float().reshape(1).cpu().numpy()
        for name, opt in (("decoder", ts.decoder_optimizer), ("encoder", ts.encoder_optimizer)):
            if opt is not None:
                arrays[name + "_params"] = sample(opt.params)
                arrays[name + "_grads"] = sample([p.grad if p.grad is not None else torch.zeros_like(p)
                                                  for p in opt.params])
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)


def warm_miopen(dev, batch, fine_tune):
    """One throw-away ResNet-152 forward/backward so that MIOpen's compiled kernels are in the on-disk
    cache before the other ranks start."""
    from models.encoders.caption import EncoderCaption
    torch.backends.cudnn.benchmark = True
    enc = EncoderCaption(channels_last=True).to(dev)
    enc.fine_tune(fine_tune)
    enc.train()
    x = torch.randn(batch, 3, 256, 256, device=dev)
    y = enc(x)
    if fine_tune:
        y.sum().backward()
    torch.cuda.synchronize()
    del enc, x, y
    torch.cuda.empty_cache()


def hdf5_batches(args, cfg, dev, rank, world):
    """Endless stream of device batches read from the reference's file formats (utils/dataset.py:332-414):
    rank 0 writes a synthetic split into a temp dir (uint8 images, full-length captions as in SURVEY 8d),
    every rank then opens it with the device loader."""
    import tempfile
    import numpy as np
    from scnattn import h5lite
    from scnattn.data import DeviceBatchLoader
    root = os.path.join(tempfile.gettempdir(), "scnattn_bench_data_%d" % os.getuid())
    base = "synth_5_cap_per_img_5_min_word_freq"
    L, V, N, cpi = cfg["max_len"] + 2, cfg["vocab_size"], args.data_images, 5
    if rank == 0:
        os.makedirs(root, exist_ok=True)
        rng = np.random.RandomState(1234)
        imgs = rng.randint(0, 256, size=(N, 3, cfg["image_size"], cfg["image_size"]), dtype=np.uint8)
        h5lite.write_arrays(os.path.join(root, "TRAIN_IMAGES_" + base + ".hdf5"), {"images": imgs},
                            {"captions_per_image": cpi})
        caps = rng.randint(1, V - 3, size=(N * cpi, L))
        caps[:, 0], caps[:, L - 1] = V - 2, V - 1
        with open(os.path.join(root, "TRAIN_CAPTIONS_" + base + ".json"), "w") as fh:
            json.dump(caps.tolist(), fh)
        with open(os.path.join(root, "TRAIN_CAPLENS_" + base + ".json"), "w") as fh:
            json.dump([L] * (N * cpi), fh)
    if world > 1:
        dist.barrier()
    loader = DeviceBatchLoader(root, base, "TRAIN", args.batch, dev, cpi=cpi, shuffle=True, seed=0, rank=rank,
                               world=world, channels_last=True, resident=(args.data == "hdf5-resident"),
                               drop_last=True)

    def gen():
        epoch = 0
        while True:
            loader.set_epoch(epoch)
            for b in loader:
                yield b
            epoch += 1
    return gen()


def launch_ranks(n):
    """`bench.py --gpus N` started without a launcher: run `python -m torch.distributed.run --nproc-per-node N
    bench.py <same arguments>` as a child process (never exec: nothing here has touched the GPU yet, and it stays
    that way), pass its stdout/stderr through and return its exit status."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("[bench] --gpus %d without WORLD_SIZE: starting %d ranks: %s" % (n, n, " ".join(cmd)), file=sys.stderr,
          flush=True)
    return subprocess.call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="attention_scn", choices=["attention_scn", "pure_scn", "pure_attention"])
    ap.add_argument("--no-finetune", action="store_true", help="freeze the encoder (reference default)")
    ap.add_argument("--decoder-only", action="store_true", help="feed a synthetic encoder_out (diagnostics)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--max-len", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--full", action="store_true",
                    help="also the figures beyond the headline: median step, allocator, rooflines, the reference's "
                         "literal call sequence, CPU baseline (extra steps and timing after the timed region)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (dump_outputs)")
    ap.add_argument("--ksplit", type=int, default=0)
    ap.add_argument("--with-tagger", action="store_true",
                    help="also run the frozen EncoderTagger ResNet-152 each step (the reference's real step)")
    ap.add_argument("--encoder-dtype", default="f32", choices=["f32", "bf16"],
                    help="bf16: ResNet trunk under bf16 autocast (BASELINE config 5 flavour; not the fp32 headline)")
    ap.add_argument("--decoder-dtype", default="f32", choices=["f32", "bf16", "bf16mfma"],
                    help="bf16: the decode step streams bf16 copies of the recurrent weights, att1 and the trunk map "
                         "(fp32 accumulate / state / master weights / gradients)")
    ap.add_argument("--dtype", default=None, choices=["f32", "bf16"],
                    help="shorthand: bf16 = --encoder-dtype bf16 --decoder-dtype bf16mfma (BASELINE configs[4] flavour, a "
                         "second line next to the fp32 headline)")
    ap.add_argument("--host-lengths", action="store_true",
                    help="A/B: caption lengths also as a CPU tensor -> no host sync in the decoder's forward pass (measured slower)")
    ap.add_argument("--no-tagger-overlap", action="store_true",
                    help="A/B (--with-tagger): the tagger's forward pass in line on the main stream instead of beside the "
                         "caption encoder's on the side stream")
    ap.add_argument("--lib-option", action="append", default=[], metavar="NAME=INT",
                    help="A/B: scnattn_set_option(NAME, INT) before the step is built (include/scnattn.h lists the names)")
    ap.add_argument("--force-dist", action="store_true",
                    help="diagnostics: run the multi-rank code path (RCCL group, barriers, reducers) with one rank")
    ap.add_argument("--forward-only", action="store_true", help="diagnostics: decoder forward only (PMC passes)")
    ap.add_argument("--data", default="synthetic", choices=["synthetic", "hdf5-resident", "hdf5-staged"],
                    help="hdf5-*: every step takes its batch from the reference's on-disk format (a synthetic "
                         "*_IMAGES_*.hdf5 + JSON captions written to a temp dir) through scnattn.data.DeviceBatchLoader "
                         "inside the timed region; resident = uint8 dataset in HBM, staged = pinned uint8 batches over PCIe")
    ap.add_argument("--data-images", type=int, default=1024, help="images in the synthetic HDF5 file")
    ap.add_argument("--dense-attention", action="store_true",
                    help="A/B: attention over the materialised 14x14 pooled map (the reference's data flow) instead "
                         "of the trunk's 8x8 source map (scnattn_pool)")
    ap.add_argument("--bn-mask-from-y", action="store_true", help="A/B: BatchNorm backward reads y for the ReLU mask")
    ap.add_argument("--attn-depth", type=int, default=1, help="0: shallower load batches in attn_context/dalpha (A/B)")
    ap.add_argument("--gemm-opts", default="", help="diagnostics: target,kmin,kmin_small of the split-K policy")
    ap.add_argument("--graph", action="store_true", help="replay the encoder as HIP graphs (measured slower)")
    ap.add_argument("--no-fused-conv", action="store_true",
                    help="A/B: the round-1 trunk (every convolution on MIOpen, BatchNorm as separate passes) instead of "
                         "the fused Bottleneck on the hand-written 1x1-convolution kernels (scnattn/conv.py)")
    ap.add_argument("--no-cgemm", action="store_true", help="A/B: dense products on the round-1 sgemm kernel")
    ap.add_argument("--dp-backend", default=os.environ.get("SCNATTN_DP_BACKEND", "torch"), choices=["torch", "cabi"],
                    help="gradient all-reduce through torch.distributed (RCCL) or through the library's own RCCL "
                         "communicator (include/scnattn.h scnattn_dp_comm_*)")
    ap.add_argument("--bucket-mb", type=int, default=32, help="data-parallel all-reduce bucket size (MiB)")
    ap.add_argument("--no-side-wgrad", action="store_true", help="A/B: weight gradients on the main stream")
    ap.add_argument("--drop-in-call", action="store_true",
                    help="time ONLY the reference's literal call sequence (encoder(imgs) -> decoder(encoder_out, ...), "
                         "trains/attention_scn.py:213-216) as the headline; by default it is timed as a second figure "
                         "(`drop_in_call` in the JSON line) after the harness sequence")
    args = ap.parse_args()
    if args.dtype:
        args.encoder_dtype = args.dtype
        args.decoder_dtype = "bf16mfma" if args.dtype == "bf16" else args.dtype
    os.environ["SCNATTN_DP_BACKEND"] = args.dp_backend

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))       # before any GPU call
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: WORLD_SIZE=%d but --gpus %d: launch with torch.distributed.run --nproc-per-node %d "
                 "(or run bare and let bench.py start the ranks)" % (world, args.gpus, args.gpus))
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback for the product path)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist_on = world > 1 or args.force_dist
    if dist_on:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend="nccl", device_id=dev)
        assert dist.get_world_size() == world, "RCCL group has %d ranks, expected %d" % (dist.get_world_size(), world)

    from scnattn import _lib
    from scnattn import functional as SF
    from trains.harness import TrainStep, synthetic_batch
    if args.no_fused_conv:
        from scnattn import conv as _conv
        _conv.ENABLED = False
    if args.no_cgemm:
        SF.set_option("use_cgemm", 0)
    if args.no_side_wgrad:
        from scnattn import conv as _conv2
        _conv2.SIDE_WGRAD = False
    for kv in args.lib_option:
        name, _, val = kv.partition("=")
        SF.set_option(name, int(val))
    if args.ksplit:
        SF.set_option("ksplit", args.ksplit)
    if args.bn_mask_from_y:
        SF.BN_MASK_FROM_Z = False
    if args.dense_attention:
        from models.decoders import _common as _dec_common
        _dec_common.USE_PREPOOL = False          # also ignore the map EncoderCaption attaches to its output
    SF.set_option("attn_depth", args.attn_depth)
    if args.gemm_opts:
        for name, v in zip(("gemm_target", "gemm_kmin", "gemm_kmin_small", "gemm_gate"), args.gemm_opts.split(",")):
            SF.set_option(name, int(v))
    fine_tune = not args.no_finetune
    # MIOpen JIT-compiles its convolution kernels on first use (this image has no gfx950 kernel database)
    # and caches the binaries per user.  With N ranks starting together every rank would compile the same
    # ~150 kernels at once on shared host cores: let rank 0 populate the cache first.
    if dist_on:
        if rank == 0 and not args.decoder_only:
            warm_miopen(dev, args.batch, fine_tune)      # no collective inside
        dist.barrier()                                    # first collective on every rank
    ts = TrainStep(kind=args.workload, fine_tune_encoder=fine_tune, device=dev, encoder=not args.decoder_only,
                   batch_size=args.batch, max_len=args.max_len, graph_encoder=args.graph, tagger=args.with_tagger, force_reduce=args.force_dist,
                   encoder_dtype=args.encoder_dtype, decoder_dtype=args.decoder_dtype,
                   tagger_overlap=not args.no_tagger_overlap,
                   pooled_attention=not args.dense_attention, bucket_mb=args.bucket_mb)
    cfg = ts.cfg
    imgs, tags, caps, caplens = synthetic_batch(args.batch, cfg["vocab_size"], cfg["max_len"], cfg["image_size"],
                                                cfg["semantic_dim"], dev, 1234 + rank)
    enc_in = pre_in = None
    if args.decoder_only:
        if args.workload == "attention_scn" and not args.dense_attention:
            pre_in = torch.rand(args.batch, 8, 8, 2048, device=dev)     # the trunk's map at 256x256 input
        else:
            enc_in = torch.rand(args.batch, 14, 14, 2048, device=dev)

    batches = None
    if args.data != "synthetic":
        batches = hdf5_batches(args, cfg, dev, rank, world)

    last_loss = [None]
    last_fwd = [None]      # --forward-only: what the decoder returned
    # --host-lengths (experiment): hand the decoder the caption lengths as a CPU tensor too, so that its forward pass
    # needs no device synchronisation to learn its loop bounds.  Round 3, after a long warm-up: 815 vs 812 images/s with
    # 18.8 instead of 10.4 GiB reserved (the host runs a step ahead, so blocks the side stream still holds cannot be
    # reused); with the default warm-up the extra hipMallocs make it slower.  Not worth a second copy of the activations.
    caplens_host = caplens.cpu() if (args.host_lengths and batches is None) else None

    step_marks = []      # --full: one HIP event per step end (no synchronisation): per-step durations -> the median of SURVEY 8(d)

    def run(n, mark=False):
        nonlocal imgs, caps, caplens
        for _ in range(n):
            if batches is not None:
                imgs, caps, caplens = next(batches)
            if args.forward_only:
                with torch.no_grad():
                    last_fwd[0] = ts.decoder(enc_in, tags, caps, caplens, prepool=pre_in) if pre_in is not None else \
                        ts.decoder(enc_in, tags, caps, caplens)
            else:
                last_loss[0] = ts.step(imgs, tags, caps, caplens, enc_in, pre_in, drop_in=drop_in[0],
                                       caplens_host=caplens_host)
            if mark:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                step_marks.append(e)

    drop_in = [bool(args.drop_in_call)]
    dbg = (lambda m: print("[bench] " + m, file=sys.stderr, flush=True)) if os.environ.get("BENCH_DEBUG") else (lambda m: None)
    dbg("built; warm-up")
    run(args.warmup)
    dbg("warm-up done")
    prof = (ctypes.c_double * 6)()
    if args.full:
        SF.set_option("profile", 1)
        torch.cuda.synchronize()
        _lib.call("scnattn_profile_collect", prof)   # drop warm-up events
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    ms0 = torch.cuda.memory_stats(dev) if args.full else None
    t0 = time.perf_counter()
    if args.full:
        e_start = torch.cuda.Event(enable_timing=True)
        e_start.record()
        step_marks.append(e_start)
    run(args.steps, mark=args.full)
    torch.cuda.synchronize()
    alloc_stats = None
    if args.full:
        ms1 = torch.cuda.memory_stats(dev)
        # device allocations (hipMalloc) inside the timed region: each one stalls the device
        alloc_stats = {"segments_allocated_in_timed_region": int(ms1.get("segment.all.allocated", 0) - ms0.get("segment.all.allocated", 0)),
                       "alloc_retries_in_timed_region": int(ms1.get("num_alloc_retries", 0) - ms0.get("num_alloc_retries", 0)),
                       "reserved_GiB": round(ms1.get("reserved_bytes.all.current", 0) / 2**30, 2)}
        dbg("allocator: %r" % (alloc_stats,))
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dbg("timed region done")

    # outside the timed region, before any further step: the last timed step's results
    if last_loss[0] is not None:     # the model must still be training on finite numbers
        final_loss = float(last_loss[0].detach())
        assert final_loss == final_loss and abs(final_loss) < 1e6, "loss diverged: %r" % final_loss
    else:
        final_loss = None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ts, last_loss[0], last_fwd[0])
        dbg("outputs written to " + args.dump_outputs)

    ctx_us, ctx_per_step = None, 1.0
    enc_ms = None
    elapsed_di = None
    if args.full:
        _lib.call("scnattn_profile_collect", prof)
        # outside the timed region: per-launch HIP-event timing of the dominant single kernel (attn_context)
        if args.workload == "attention_scn" and not args.forward_only:
            SF.set_option("profile", 2)
            run(2)
            torch.cuda.synchronize()
            p2 = (ctypes.c_double * 6)()
            _lib.call("scnattn_profile_collect", p2)
            if p2[5] > 0 and p2[1] > 0:
                ctx_us = 1e3 * p2[4] / p2[5]
                ctx_per_step = p2[5] / p2[1]      # 2 with the two-chain recurrence (half the batch rows per launch)
        SF.set_option("profile", 0)
        # outside the timed region: the encoder's forward + backward time by HIP events (3 extra steps) -> roofline_trunk
        if not args.decoder_only and not args.forward_only:
            ts.encoder_events = []
            run(3)
            torch.cuda.synchronize()
            per = []
            for ev in ts.encoder_events:
                fwd = ev[0].elapsed_time(ev[1])
                bwd = ev[2].elapsed_time(ev[3]) if fine_tune else 0.0
                per.append((fwd, bwd))
            ts.encoder_events = None
            if per:
                per.sort(key=lambda fb: fb[0] + fb[1])
                enc_ms = per[len(per) // 2]
        # second figure, outside the headline's timed region: the same K steps through the reference's literal call
        # sequence (the pooled (B,14,14,2048) map is materialised and the decoder picks the trunk map up from the tag)
        if not args.drop_in_call and not args.decoder_only and not args.forward_only and args.workload != "pure_scn":
            drop_in[0] = True
            run(2)
            torch.cuda.synchronize()
            if dist_on:
                dist.barrier()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            if dist_on:
                dist.barrier()
            torch.cuda.synchronize()
            elapsed_di = time.perf_counter() - t1
            drop_in[0] = False
    if dist_on:
        tmax = torch.tensor([elapsed, elapsed_di or 0.0], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax[0].item())
        if elapsed_di is not None:
            elapsed_di = float(tmax[1].item())

    dbg("reductions done")
    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        value = world * args.batch * args.steps / elapsed
        T = cfg["max_len"] + 1
        out = {
            "metric": "images/sec (train step, SCN+Attention, bs32/GPU)" if args.workload == "attention_scn"
            else "images/sec (train step, %s, bs%d/GPU)" % (args.workload, args.batch),
            "value": round(value, 3), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_step, 3),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "loss_after_timed_steps": None if final_loss is None else round(final_loss, 4),
            "dtype": {("f32", "f32"): "f32",
                      ("bf16", "f32"): "bf16 encoder convs (fp32 accumulate/master) + f32 decoder",
                      ("f32", "bf16"): "f32 encoder + bf16-storage decoder step (fp32 accumulate/state/master/gradients)",
                      ("bf16", "bf16"): "bf16 encoder convs + bf16-storage decoder step (fp32 accumulate/state/master/gradients)",
                      ("f32", "bf16mfma"): "f32 encoder + bf16 decoder step (bf16 operands on the bf16 MFMA, fp32 accumulate/state/master/gradients)",
                      ("bf16", "bf16mfma"): "bf16 encoder convs + bf16 decoder step (bf16 operands on the bf16 MFMA, fp32 accumulate/state/master/gradients)"
                      }[(args.encoder_dtype, args.decoder_dtype)],
            "data": "synthetic" if args.data == "synthetic" else
            "synthetic %d-image HDF5 split read through scnattn.data.DeviceBatchLoader (%s) inside the timed region"
            % (args.data_images, args.data),
            "config": {"workload": "%s decoder (emb/att/factor/dec=512, 1000 tags, V=%d, T=%d)%s, bs=%d/GPU, "
                                   "256x256 images, fp32" % (args.workload, cfg["vocab_size"], T,
                                                             " decoder only" if args.decoder_only else
                                                             (" + ResNet-152 fine-tune" if fine_tune
                                                              else " + frozen ResNet-152") +
                                                             (" + tagger ResNet-152" if args.with_tagger else
                                                              ", synthetic tags"), args.batch),
                       "global_batch": world * args.batch, "parallelism": "dp%d" % world,
                       "call_sequence": "drop-in: encoder(imgs) -> decoder(encoder_out, ...)" if args.drop_in_call else
                       "harness: encoder(imgs, pooled=False) -> decoder(None, ..., prepool=trunk map)"},
            "rccl_world_size": dist.get_world_size() if dist_on else 1,
            "dp_backend": (args.dp_backend if dist_on else None),
        }
        if args.full:
            # SURVEY 8(d) defines the metric on the MEDIAN step; `value` / `ms_per_step` stay the whole-region figures the
            # driver's own clock can check (K steps / wall time between two barriers), the median (rank 0's GPU timeline,
            # HIP events at every step end) rides beside them
            durs = sorted(step_marks[i].elapsed_time(step_marks[i + 1]) for i in range(len(step_marks) - 1))
            ms_median = durs[len(durs) // 2] if durs else None
            out["ms_per_step_median"] = None if ms_median is None else round(ms_median, 3)
            out["value_at_median_step"] = None if not ms_median else round(world * args.batch * 1e3 / ms_median, 3)
            out["allocator"] = alloc_stats
        if not args.decoder_only and not args.no_fused_conv:
            from scnattn import conv as _conv
            out["config"]["trunk"] = ("stem (7x7 conv + BN + ReLU + max-pool) on csrc/stem.hip; fused Bottleneck: every convolution "
                                      "(1x1 and 3x3; fwd, dgrad, wgrad) on csrc/cgemm.hip / csrc/conv3.hip with BatchNorm "
                                      "prologues/epilogues; SCNATTN_CONV3=%s" % _conv.CONV3)
            out["config"]["side_stream"] = "; ".join("weight gradients on a second HIP stream, found concurrent with the main "
                                                     "stream by experiment (%s)" % sd.probe for sd in _conv._sides.values()) or None
        if elapsed_di is not None:
            out["drop_in_call"] = {"value": round(world * args.batch * args.steps / elapsed_di, 3), "unit": "images/sec",
                                   "ms_per_step": round(1e3 * elapsed_di / args.steps, 3),
                                   "what": "same K steps through the reference's literal call sequence "
                                           "(trains/attention_scn.py:213-216): encoder(imgs) materialises the "
                                           "(B,14,14,2048) map, decoder(encoder_out, ...) gets only that tensor"}
        if args.workload == "attention_scn" and prof[1] > 0:
            step_us = 1e3 * prof[0] / prof[1]
            ab = step_bytes(cfg, args.batch)
            ach = ab / (step_us * 1e-6) / 1e9
            traffic, tsrc = None, None
            pooled = not args.dense_attention
            dbf = args.decoder_dtype in ("bf16", "bf16mfma")
            pmc_name = ("r02_pmc_decode_step_fwd_%s_bf16mfma.json" if args.decoder_dtype == "bf16mfma" else
                        "r02_pmc_decode_step_fwd_%s_bf16.json" if dbf else
                        "r03_pmc_decode_step_fwd_%s.json" if pooled else "r01_pmc_decode_step_fwd_%s.json") \
                % ("pooled" if pooled else "dense")
            pmc = os.path.join(ROOT, "profiles", pmc_name)
            if args.batch == 32 and os.path.exists(pmc):   # PMC passes cannot run inside this process;
                with open(pmc) as fh:                        # the committed rocprofv3 result is quoted
                    traffic = json.load(fh).get("hbm_bytes_per_step")
                tsrc = "profiles/%s (separate rocprofv3 --pmc passes)" % pmc_name
            # `achieved` prices the step at SURVEY 8d's algorithmic bytes (the reference's formulation: the pooled
            # 14x14 map is read every step).  The pooled path moves fewer: the context reads the 8x8 source map.
            eb = step_bytes(cfg, args.batch, P=64) + 4 * args.batch * (196 - 64) * cfg["attention_dim"] if pooled else ab
            if dbf:            # every operand the step streams is stored as bf16 in this mode
                eb //= 2
            ach_e = eb / (step_us * 1e-6) / 1e9
            nlaunch = 7
            ctx_bytes = (2 if dbf else 4) * args.batch * (64 if pooled else 196) * 2048
            # "if an algebraic shortcut is used that executes fewer [bytes] than this formula, report
            # executed [work] instead" -- `achieved` / `frac` are on the bytes the kernels actually have to move;
            # the figure priced on the reference formulation's 98.8 MB stays as a named side field.
            out["roofline"] = {"bound": "hbm", "achieved": round(ach_e, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(ach_e / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": tsrc,
                               "achieved_on_reference_formulation_bytes": round(ach, 1),
                               "frac_on_reference_formulation_bytes": round(ach / HBM_PEAK_GBS, 4),
                               "kernel": "decode step fwd = skinny_kernel x3 + attn_scores + attn_context + scn_mix_fwd + "
                                         "lstm_fwd: 7 launches (the fused SCN-cell+attention step of north_star)",
                               # measured floor of a dependent launch on this chip (tools/chain_floor.hip, hipGraph replay
                               # of trivial 256-workgroup kernels: profiles/r02_decode_step_launch_floor.txt): what the
                               # step's launch boundaries cost before any byte of its operands moves
                               "launch_floor": {"us_per_dependent_launch": LAUNCH_FLOOR_US, "launches": nlaunch,
                                                "floor_us": round(nlaunch * LAUNCH_FLOOR_US, 1),
                                                "achieved_GBs_in_the_remaining_time":
                                                    round(eb / max(step_us - nlaunch * LAUNCH_FLOOR_US, 1e-3) / 1e3, 1),
                                                "source": "profiles/r02_decode_step_launch_floor.txt"},
                               "algorithmic_bytes_per_step": ab, "avg_step_us": round(step_us, 2),
                               "executed_bytes_per_step": eb,
                               "attention_path": "pooled: context / d alpha over the trunk's 8x8 map (scnattn_pool), "
                                                 "same numbers by linearity of the average pool" if pooled else
                                                 "dense: over the materialised 14x14 pooled map, as the reference",
                               "dominant_single_kernel": None if ctx_us is None else {
                                   "name": "attn_context_kernel (softmax + sum_p alpha*enc + gate)",
                                   "launches_per_step": round(ctx_per_step, 2),
                                   "algorithmic_bytes": int(ctx_bytes / ctx_per_step),
                                   "avg_us": round(ctx_us, 2),
                                   "achieved_GBs": round(ctx_bytes / ctx_per_step / (ctx_us * 1e-6) / 1e9, 1),
                                   "frac": round(ctx_bytes / ctx_per_step / (ctx_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                   "note": ("one launch bracketed by two HIP event records on the launch stream, measured in "
                                            "two extra steps outside the timed region: the bracket adds the processing of "
                                            "its own two markers (~3 us); rocprofv3's duration of this kernel inside the same "
                                            "step is 7.7 us (profiles/r03_full_step_kernel_stats_fp32.csv)")
                                   },
                               "bwd_avg_step_us": round(1e3 * prof[2] / prof[3], 2) if prof[3] > 0 else None}
        if enc_ms is not None:
            bf = args.encoder_dtype == "bf16"
            gflop = ENC_GFLOP_PER_IMAGE[bool(fine_tune)] * args.batch
            tot = enc_ms[0] + enc_ms[1]
            peak = MFMA_BF16_PEAK_TF if bf else MFMA_F32_PEAK_TF
            out["roofline_trunk"] = {
                "bound": "mfma", "achieved": round(gflop / tot, 1), "peak": peak, "unit": "TFLOP/s",
                "frac": round(gflop / tot / peak, 4),
                "flops_per_step": gflop * 1e9, "encoder_fwd_ms": round(enc_ms[0], 3), "encoder_bwd_ms": round(enc_ms[1], 3),
                "what": "ResNet-152 trunk of one rank, %s: SURVEY 8(d)'s algorithmic %.2f GFLOP per image x %d images over the "
                        "encoder's forward + backward time (HIP events on the launch stream around encoder(imgs) and from the "
                        "moment the decoder's backward pass hands over d(feature map) to the end of backward(), side-stream "
                        "weight gradients joined; median of 3 extra steps outside the timed region); peak = %s matrix peak at "
                        "2.4 GHz -- the chip sustains ~2.0 GHz under this load (csrc/cgemm.hip: 131-134 TFLOP/s at 4096^3)"
                        % ("fine-tuning layer2-4" if fine_tune else "frozen (forward only)",
                           ENC_GFLOP_PER_IMAGE[bool(fine_tune)], args.batch, "bf16" if bf else "fp32-input")}
        if args.full and world == 1 and not args.no_cpu_baseline and not args.decoder_only:
            print("[bench] GPU part done: %.1f images/sec; timing the CPU oracle sample ..." % value,
                  file=sys.stderr, flush=True)
            try:
                out["cpu_baseline"] = cpu_baseline(args.workload, cfg, fine_tune, args.batch)
            except Exception as e:  # the baseline must never take the GPU number down with it
                out["cpu_baseline"] = {"value": None, "unit": "images/sec", "cores": os.cpu_count(), "kind": "port",
                                       "sample": "failed: %r" % (e,)}
        sys.stdout.flush()
        print(json.dumps(out), flush=True)      # the LAST stdout line (RCCL may print a version banner before it)
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
