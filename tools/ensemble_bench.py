"""Ensemble caption generation throughput: DecoderEnsemble.sample_batch() -- M decoders under one beam search on the
device -- against the M single sample_batch() calls on the same inputs and against the module-path ensemble.

    python tools/ensemble_bench.py [--images 32] [--beam 5] [--repeats 7] [--out profiles/ensemble_bench.txt]

The three decoders (A = AttentionSCN, S = PureSCN, P = PureAttention) get random weights from one seed at the train step's
widths (P=196, E=2048, A=D=F=M=512, S=1000, V=10000), fc sharpened and the <end> bias raised so that searches end at
mixed lengths.  Sides, each in a FRESH process (`--side NAME`, started from here):
    ens:A+S:logprob  ens:A+S:prob  ens:A+S+P:logprob  ens:A+S+P:prob     the ensemble search on the device
    single:A  single:S  single:P                                         one decoder's sample_batch
    module:A+S  module:A+S+P      the host ensemble: per image and step one nn.Module step per member, the combination
                                  (logprob) in torch, one topk and one .tolist() -- what there was without the driver
A warm-up pass over the whole batch, then `--repeats` timed passes, each bracketed by device events around the whole
batch (the searches synchronise inside, so the events see host time too); the median is reported.  Prints one JSON line
per side and a summary that sets each ensemble beside the sum of its members' single searches.  Not part of bench.py."""
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

SIDES = ["ens:A+S:logprob", "ens:A+S:prob", "ens:A+S+P:logprob", "ens:A+S+P:prob", "single:A", "single:S", "single:P",
         "module:A+S", "module:A+S+P"]
WEIGHTS = {"A+S": (0.625, 0.375), "A+S+P": (0.5, 0.25, 0.25)}


def word_map(V):
    wm = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
    for i in range(1, V - 3):
        wm["w%d" % i] = i
    return wm


def module_ensemble(members, weights, k, wm, enc1, tags1):
    """models/decoders/_common.beam_search for M decoders and one image, candidates ranked by sum_m w_m log_softmax_m:
    one module step per member per time step, a host topk and a .tolist()"""
    import torch
    import torch.nn.functional as F
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    from scnattn import functional as SF
    V, dev = len(wm), enc1.device
    E = enc1.size(3)
    enc = enc1.reshape(1, -1, E).expand(k, -1, E).contiguous()
    tags = tags1.expand(k, tags1.size(1)).contiguous()
    prev = torch.full((k, 1), wm["<start>"], dtype=torch.long, device=dev)
    seqs, top = prev, torch.zeros(k, 1, device=dev)
    state = [m.init_hidden_state(enc) for m in members]
    done, done_scores, step = [], [], 1
    while True:
        comb = None
        for i, m in enumerate(members):
            h, c = state[i]
            x = m.embedding(prev).squeeze(1)
            if not isinstance(m, PureSCN):
                awe, _ = m.attention(enc, h)
                x = torch.cat([x, torch.sigmoid(SF.linear(h, m.f_beta.weight, m.f_beta.bias)) * awe], dim=1)
            h, c = m.decode_step(x, (h, c)) if isinstance(m, PureAttention) else m.decode_step(x, tags, (h, c))
            state[i] = (h, c)
            lp = weights[i] * F.log_softmax(SF.linear(h, m.fc.weight, m.fc.bias), dim=1)
            comb = lp if comb is None else comb + lp
        scores = top.expand_as(comb) + comb
        top, words = (scores[0] if step == 1 else scores.view(-1)).topk(k, 0, True, True)
        src = torch.div(words, V, rounding_mode="floor")
        nxt = words % V
        seqs = torch.cat([seqs[src], nxt.unsqueeze(1)], dim=1)
        host = nxt.tolist()
        keep = [i for i, w in enumerate(host) if w != wm["<end>"]]
        fin = [i for i in range(len(host)) if i not in keep]
        if fin:
            done.extend(seqs[fin].tolist())
            done_scores.extend(top[fin].tolist())
        k -= len(fin)
        if k == 0:
            break
        seqs = seqs[keep]
        sel = src[keep]
        state = [(h[sel], c[sel]) for h, c in state]
        enc, tags = enc[sel], tags[sel]
        top, prev = top[keep].unsqueeze(1), nxt[keep].unsqueeze(1)
        if step > 50:
            break
        step += 1
    if not done_scores:
        done, done_scores = seqs.tolist(), top.view(-1).tolist()
    return done[done_scores.index(max(done_scores))]


def side(args):
    import torch
    from models.decoders import DecoderEnsemble
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    assert torch.cuda.is_available(), "ensemble_bench needs an MI355X: there is nothing to measure on a CPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    V, E, S = args.vocab, 2048, 1000
    pool = {"A": AttentionSCN(512, 512, 512, 512, S, V, encoder_dim=E, dropout=0.0),
            "S": PureSCN(512, 512, 512, S, V, encoder_dim=E, dropout=0.0),
            "P": PureAttention(512, 512, 512, V, encoder_dim=E, dropout=0.0)}       # always all three: the same weights on every side
    for m in pool.values():
        with torch.no_grad():
            m.fc.weight.mul_(args.sharpen)
            m.fc.bias[V - 1] += args.end_bias
    enc = torch.rand(args.images, 14, 14, E).to(dev)
    tags = torch.rand(args.images, S).to(dev)
    wm = word_map(V)
    what, names = args.side.split(":")[0], args.side.split(":")[1]
    members = [pool[n].to(dev).eval() for n in names.split("+")]
    if what == "ens":
        ens = DecoderEnsemble(members, weights=WEIGHTS[names], combine=args.side.split(":")[2]).to(dev).eval()

    from scnattn import functional as SF
    steps_run = []          # the steps the device searches enqueued (whole chunks of 8): a search goes on until EVERY beam has
    for fn in ("beam_search_run", "ensemble_search_run"):       # ended, so the chosen length says little about its cost

        def counted(*a, _run=getattr(SF, fn), **kw):
            out = _run(*a, **kw)
            steps_run.append(out[1])
            return out
        setattr(SF, fn, counted)

    def first(r):
        return r[0] if isinstance(r, tuple) else r

    def run():
        with torch.no_grad():
            if what == "ens":
                return [first(r) for r in ens.sample_batch(args.beam, wm, enc, tags)]
            if what == "single":
                m = members[0]
                res = m.sample_batch(args.beam, wm, enc) if names == "P" else m.sample_batch(args.beam, wm, enc, tags)
                return [first(r) for r in res]
            return [module_ensemble(members, WEIGHTS[names], args.beam, wm, enc[i:i + 1], tags[i:i + 1])
                    for i in range(args.images)]

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
    print(json.dumps({"side": args.side, "images": args.images, "beam": args.beam, "median_ms": round(med, 3),
                      "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "captions_per_s": round(args.images * 1e3 / med, 2),
                      "steps_run": steps_run[-1] if steps_run else None,
                      "us_per_step": round(med * 1e3 / steps_run[-1], 1) if steps_run else None,
                      "steps_longest": max(lens) - 1, "lengths": sorted(lens), "digest": hash(tuple(map(tuple, seqs))) & 0xffffffff}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sharpen", type=float, default=10.0)
    ap.add_argument("--end-bias", type=float, default=2.0)
    ap.add_argument("--side", choices=SIDES)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.side:
        side(args)
        return
    lines, res = [], {}
    for s in SIDES:
        cmd = [sys.executable, os.path.abspath(__file__), "--side", s] + [a for a in sys.argv[1:]]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
        lines.append(r.stdout.strip().splitlines()[-1])
        res[s] = json.loads(lines[-1])
        print(lines[-1], flush=True)
    for names in ("A+S", "A+S+P"):
        singles = sum(res["single:" + n]["median_ms"] for n in names.split("+"))
        step_sum = sum(res["single:" + n]["us_per_step"] for n in names.split("+"))
        for mode in ("logprob", "prob"):
            e = res["ens:%s:%s" % (names, mode)]
            lines.append(json.dumps({"ensemble": names, "mode": mode, "median_ms": e["median_ms"], "steps_run": e["steps_run"],
                                     "us_per_step": e["us_per_step"], "sum_of_single_us_per_step": round(step_sum, 1),
                                     "step_ens_over_sum": round(e["us_per_step"] / step_sum, 3),
                                     "sum_of_single_ms": round(singles, 3), "ens_over_sum": round(e["median_ms"] / singles, 3),
                                     "module_path_ms": res["module:" + names]["median_ms"],
                                     "module_over_ens": round(res["module:" + names]["median_ms"] / e["median_ms"], 2),
                                     "same_captions_as_module_path": e["digest"] == res["module:" + names]["digest"]
                                     if mode == "logprob" else None}))
            print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/ensemble_bench.py %s\n" % " ".join(sys.argv[1:]) + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
