"""The cases of tests/test_gpu_sampling_kernels.py, stated once: the GPU module runs them, tests/test_sampling_refs.py checks on
the CPU reference alone that their caps hold (at least 80 % of the judged rows SHARP), so a bad seed fails without a GPU.

A RUN is one state walked over STEPS = 3 steps (rows close on the way) with one filter, one kind of logits, one base
alignment (mis), one inv_temp and one draw.  A CASE is a shape (V, row configuration) with its list of runs: the ten filters
of the issue, the kind of logits / alignment / temperature cycling along so that over the shapes every filter meets every
kind on both load paths.

Kinds of logits (per step [R, V]):
    u3, u9   uniform in +-3 / +-9
    quant    uniform in +-3 rounded to multiples of 0.25: many exact ties, straddling both cuts
    peaked   u3 with one word per row raised by 20: more than 0.999 of the mass, nkeep = 1 under every top_p used
    flat     all equal: nkeep is decided by the index alone
    neginf   u3 with the words 1 .. V // 3 at -inf: mass 0, last in the order
As in tests/test_gpu_rollout_kernels.py the arg-max rows of step 0 get two or three exactly equal maxima (kinds u3, u9, quant,
neginf) and <end> = V - 1 is raised by 20 on rows r % 3 == 1 at step 1, so that rows close."""
import torch

import sampling_refs as SR

SEED = 0x5eed0123456789ab
STEPS = 3
VS = (5, 257, 1003, 1024, 2051)
# (N, K, greedy_first, closed image or None)
CONFIGS = {"R1": (1, 1, False, None), "R7": (7, 1, False, None), "K3greedy": (3, 3, True, 1), "K7greedy": (1, 7, True, None)}
INV_TEMPS = (1.0, float(torch.tensor(1.0 / 0.7, dtype=torch.float32)))
KINDS = ("u3", "u9", "quant", "peaked", "flat", "neginf")
SHARP_SHARE = 0.8


def filters(V):
    """(top_k, top_p): top-k alone, top-p alone, both, one where top-k binds, one where top-p binds"""
    return [(1, 1.0), (2, 1.0), (50, 1.0), (V - 1, 1.0), (0, 0.9), (0, 0.5), (0, 1e-6), (50, 0.9), (2, 0.999), (V - 1, 0.5)]


def gen_logits(V, N, K, greedy_first, kind, salt):
    g = torch.Generator().manual_seed(12000 + 7 * V + 131 * N + 17 * K + 1009 * salt + KINDS.index(kind))
    R = N * K
    out = []
    for t in range(STEPS):
        x = (torch.rand(R, V, generator=g) * 6 - 3).float()
        if kind == "u9":
            x = x * 3
        elif kind == "quant":
            x = torch.round(x * 4) / 4
        elif kind == "flat":
            x = torch.full((R, V), 0.5)
        elif kind == "peaked":
            at = torch.randint(0, V, (R,), generator=g)
            x[torch.arange(R), at] += 20.0
        elif kind == "neginf":
            x[:, 1:1 + max(V // 3, 1)] = float("-inf")
        if t == 0 and greedy_first and V >= 5 and kind in ("u3", "u9", "quant", "neginf"):
            top = float(x[torch.isfinite(x)].max()) + 0.5
            for r in range(0, R, K):
                a = int(torch.randint(0, V - 3, (1,), generator=g))
                x[r, a + 1] = x[r, a + 3] = top
                if r == 0:
                    x[r, V - 2] = top
        if t == 1 and V > 5:
            x[1::3, V - 1] += 20.0
        out.append(x)
    return out


def runs_of(V, cfg, which=None, salt=0):
    """the runs of the case (V, cfg): dicts(top_k, top_p, kind, mis, it_idx, draw); which: indices into filters(V)"""
    vi = VS.index(V) if V in VS else 0
    ci = sorted(CONFIGS).index(cfg)
    out = []
    for fi, (k, p) in enumerate(filters(V)):
        if which is not None and fi not in which:
            continue
        out.append(dict(top_k=k, top_p=p, kind=KINDS[(fi + vi + ci + salt) % len(KINDS)], mis=(fi + ci) % 2, it_idx=(fi // 2 + vi) % 2,
                        draw=1 + fi, salt=salt))
    return out


# the cases beyond the table VS x CONFIGS: (name, V, cfg, which filters, force_passes, salt)
EXTRA = [("V10000", 10000, "R7", (7,), 0, 1),                      # the row in registers at the flagship's vocabulary, once
         ("V3077", 3077, "R7", (5, 8), 0, 8),                       # just inside the largest register size: mostly empty slots
         ("V20011", 20011, "K3greedy", (4, 9), 0, 2),              # beyond the registers: the global-memory path, once
         ("V2051-passes-R1", 2051, "R1", (1, 5, 7, 9), 1, 3),      # the same path at a small V (force_passes)
         ("V2051-passes-R7", 2051, "R7", (0, 4, 6, 8), 1, 4),
         ("V2051-passes-K3greedy", 2051, "K3greedy", (2, 5, 7, 9), 1, 5),
         ("V2051-passes-K7greedy", 2051, "K7greedy", (3, 4, 7, 8), 1, 6)]


def run_logits(V, cfg, run):
    N, K, greedy, _ = CONFIGS[cfg]
    return gen_logits(V, N, K, greedy, run["kind"], run["salt"] * 16 + run["draw"])


def reference_steps(V, cfg, run, logits):
    """per step: sampling_refs.pick on the device's y (the fp32 product, widened): the exact ORDER, fp64 masses"""
    N, K, greedy, _ = CONFIGS[cfg]
    return [SR.pick(SR.y32(logits[t], INV_TEMPS[run["it_idx"]]).double(), K, 1.0, SEED, run["draw"], t, greedy,
                    run["top_k"], run["top_p"]) for t in range(STEPS)]


def sharp_share_on_reference(V, cfg, runs):
    """(sharp, judged) over the rows the reference itself leaves open, following ITS tokens: what the cap needs, without a
    device"""
    N, K, greedy, closed = CONFIGS[cfg]
    R = N * K
    sharp = judged = 0
    for run in runs:
        logits = run_logits(V, cfg, run)
        ps = reference_steps(V, cfg, run, logits)
        done = [closed is not None and r // K == closed for r in range(R)]
        for t in range(STEPS):
            for r in range(R):
                if done[r]:
                    continue
                judged += 1
                sharp += int(ps[t]["kept"][r]["sharp"])
                if int(ps[t]["token"][r]) == V - 1:
                    done[r] = True
    return sharp, judged


# ---- the cases of tests/test_gpu_sampling.py: whole filtered rollouts ---------------------------------------------------------
DRIVER_FILTERS = {"k3": (3, 1.0), "p0.8": (0, 0.8), "k4p0.9": (4, 0.9)}
DRIVER_INV_TEMP = float(torch.tensor(1.0 / 0.7, dtype=torch.float32))
# (fixture, K, filter) -> (seed, draw), picked on the CPU reference alone so that the caps on rows left out hold
# None leaves a row out there.  Lengths the table holds (0: a row that uses all 51 steps): 1 .. 45 and many 0, e.g.
# attention_scn_odd K=3 p0.8: 3 3 35 1 29 10 1 30 31 1 32 2 3 5 17 1 28 7; pure_attention_distinct K=1 k3: all four cut off.
DRIVER_SEEDS = {(name, K, filt): (3, 0) for name in ("attention_scn_odd", "attention_scn_distinct", "pure_scn_distinct",
                                                     "pure_attention_distinct") for K in (1, 3) for filt in DRIVER_FILTERS}
DRIVER_SEEDS[("attention_scn_odd", 3, "p0.8")] = (3, 1)
VECTOR_FILTER = (50, 0.9)
VECTOR_SEED = (6, 5, 1)         # (parameter seed, rollout seed, draw): V = 1003, N = 3, K = 3 with the arg-max slot
_CACHE = {}


def driver_reference(kind, d, wm, enc, tags, K, seed, draw, inv_temp, greedy_first, top_k, top_p):
    """-> (fp64 filtered rollout, per-row decidability under the extended rule); CPU only"""
    from helpers import params_from
    P64, P32 = params_from(d, dtype=torch.float64), params_from(d, dtype=torch.float32)
    tg = None if kind == "pure_attention" else tags
    r64 = SR.rollout(kind, P64, K, wm, enc.double(), None if tg is None else tg.double(), seed, draw, inv_temp, greedy_first,
                     top_k, top_p)
    r32 = SR.rollout(kind, P32, K, wm, enc.float(), None if tg is None else tg.float(), seed, draw, inv_temp, greedy_first,
                     top_k, top_p, tokens=r64["tokens"])
    return r64, SR.decidable_rows(r64, r32)


def fixture_case(name, kind, K, filt, seed_draw=None):
    """computed once per process: the GPU module and the CPU module's cap test share it and leave it unchanged"""
    import beam_refs as BR
    from helpers import t
    key = (name, K, filt, seed_draw)
    if key not in _CACHE:
        d, V = BR.sharpened(name)
        wm = BR.word_map(V)
        enc = t(d["enc"])
        tags = t(d["tags"]) if kind != "pure_attention" else None
        seed, draw = seed_draw or DRIVER_SEEDS[(name, K, filt)]
        top_k, top_p = DRIVER_FILTERS[filt]
        ref, ok = driver_reference(kind, d, wm, enc, tags, K, seed, draw, DRIVER_INV_TEMP, K > 1, top_k, top_p)
        _CACHE[key] = (d, wm, enc, tags, seed, draw, ref, ok)
    return _CACHE[key]


def vector_case(kind="attention_scn", K=3):
    from test_gpu_beam_search import _uniform_params
    import beam_refs as BR
    key = ("vector", kind, K)
    if key not in _CACHE:
        pseed, seed, draw = VECTOR_SEED
        g = torch.Generator().manual_seed(pseed)
        d, V, E, S = _uniform_params(kind, g)
        enc, tags = torch.rand(3, 7, 7, E, generator=g), torch.rand(3, S, generator=g)
        wm = BR.word_map(V)
        ref, ok = driver_reference(kind, d, wm, enc, tags, K, seed, draw, 1.0, K > 1, *VECTOR_FILTER)
        _CACHE[key] = (d, wm, enc, tags, seed, draw, ref, ok)
    return _CACHE[key]
