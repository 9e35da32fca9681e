"""The two kernels a search in groups changes (csrc/beam.hip), through the C ABI, one launch per call:

  * scnattn_beam_merge_groups on hand-made candidates against tests/diverse_beam_refs.merge_state.  EXACT, no tolerance:
    values, the penalty and every selection value fmaf(-penalty, c, r) are small multiples of 1/8, so fp32 computes them
    without rounding and ties are real ties.  Every state array sits in a guarded window.
  * scnattn_beam_row_topk_groups, the row selection with the group liveness: rows of dead slots are neither read (their
    logits are NaN) nor written (guard values around and inside outv / outi), and a live row gets, bit for bit, what the
    plain selection gives that row.
"""
import ctypes as C

import pytest
import torch

import diverse_beam_refs as DR
from kernel_harness import GBuf, GBufI, NAN, SENT, _call

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5), (2, 2), (3, 2), (2, 4), (4, 2), (8, 1)]      # (G, Kg)
VOCABS = (8, 1003)
FLOATS = ("best_score", "scores", "comp_score")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


class State:
    """the 12 state arrays of scnattn_beam_merge_groups, each in a guarded window of its own"""

    def __init__(self, dev, host):
        self.host = host
        self.buf = {}
        for name in DR.STATE:
            x = host[name].reshape(-1)
            self.buf[name] = GBuf(dev, x.shape, None, x, out=True) if name in FLOATS else GBufI(dev, x.numel(), x)
        self.ptrs = (C.c_void_p * 12)(*[self.buf[name].ptr.value for name in DR.STATE])

    def read(self):
        return {name: self.buf[name].read(name).reshape(self.host[name].shape).to(self.host[name].dtype) for name in DR.STATE}


def _pool(V):
    """8 words, <end> = V - 1 among them: rows of K <= 8 distinct words collide across rows and groups all the time"""
    return list(range(8)) if V == 8 else [0, 1, 2, 3, 500, 501, V - 2, V - 1]


def _candidates(g, N, K, V):
    """per row K distinct pool words with values in {0, -1/4, .., -3}, in the search order (value descending, word
    ascending) as the row selection emits them"""
    pool = torch.tensor(_pool(V))
    candv, candi = torch.zeros(N * K, K), torch.zeros(N * K, K, dtype=torch.int32)
    for r in range(N * K):
        words = pool[torch.randperm(8, generator=g)[:K]].tolist()
        vals = (-0.25 * torch.randint(0, 13, (K,), generator=g)).tolist()
        order = sorted(range(K), key=lambda q: (-vals[q], words[q]))
        candv[r] = torch.tensor([vals[q] for q in order])
        candi[r] = torch.tensor([words[q] for q in order], dtype=torch.int32)
    return candv, candi


def _state(g, N, G, Kg, T, t):
    """image 0: the first step of a search (one live source per group, Kg to fill, nothing completed);
    image 1: every group part-way (nsrc = kk in 1 .. Kg, the rest completed, a running best that a new <end> must beat by
             more than a tie), with a FINISHED group (ncomp = Kg) in the middle when there are three or more groups and as the
             first when there are two;
    image 2: nsrc = kk = max(Kg - 1, 1) < Kg where Kg > 1, its last group finished where G > 1"""
    K, R, NG = G * Kg, N * G * Kg, N * G
    nsrc, kk, ncomp = [1] * G, [Kg] * G, [0] * G
    best_i, best_s = [-1] * G, [0.0] * G
    for n in range(1, N):
        for grp in range(G):
            k = int(torch.randint(1, Kg + 1, (1,), generator=g)) if n == 1 else max(Kg - 1, 1)
            done = (n == 1 and G >= 2 and grp == (G // 2 if G >= 3 else 0)) or (n == 2 and G > 1 and grp == G - 1)
            if done:
                k = 0
            nsrc.append(k)
            kk.append(k)
            ncomp.append(Kg - k)
            best_i.append(0 if Kg - k > 0 else -1)
            best_s.append(-0.5 if Kg - k > 0 else 0.0)
    comp_score = torch.zeros(R)
    comp_step = torch.full((R,), -1, dtype=torch.int32)
    for n in range(N):
        for grp in range(G):
            for q in range(ncomp[n * G + grp]):
                comp_score[n * K + grp * Kg + q] = -0.5 - 0.25 * q
                comp_step[n * K + grp * Kg + q] = 0
    scores = -0.125 * torch.randint(0, 9, (R,), generator=g).float()
    return {"open_images": torch.tensor([N], dtype=torch.int32), "nsrc": torch.tensor(nsrc, dtype=torch.int32),
            "kk": torch.tensor(kk, dtype=torch.int32), "ncomp": torch.tensor(ncomp, dtype=torch.int32),
            "best_idx": torch.tensor(best_i, dtype=torch.int32), "best_score": torch.tensor(best_s), "scores": scores,
            "comp_score": comp_score, "comp_step": comp_step, "comp_parent": torch.zeros(R, dtype=torch.int32),
            "token": torch.full((T, R), -7, dtype=torch.int32), "parent": torch.full((T, R), -7, dtype=torch.int32)}


def _merge(dev, host, candv, candi, N, K, Kg, V, end, t, lam, entry="scnattn_beam_merge_groups"):
    st = State(dev, host)
    cv, ci = GBuf(dev, candv.shape, None, candv), candi.to(dev)
    args = (N, K, Kg, lam, V, end, t) if entry.endswith("groups") else (N, K, V, end, t)
    _call(entry, dev, *args, cv.ptr, C.c_void_p(ci.data_ptr()), st.ptrs)
    return st.read()


def _same(got, want, where):
    for name in DR.STATE:
        assert torch.equal(got[name], want[name]), (where, name, got[name].tolist(), want[name].tolist())


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("G,Kg", SHAPES)
def test_merge_groups_is_exact_on_hand_made_candidates(dev, G, Kg, V):
    """N = 3 images in the states of _state; candidates of dead slots are NaN (never read); penalties 0.5 and 0.25; every
    array of the state EQUAL to the restatement's, records of other steps and all guard words untouched"""
    N, K, T, t, end = 3, G * Kg, 3, 1, V - 1
    for seed, lam in ((11, 0.5), (12, 0.25), (13, 0.0)):
        g = torch.Generator().manual_seed(1000 * seed + 10 * G + Kg + V)
        candv, candi = _candidates(g, N, K, V)
        host = _state(g, N, G, Kg, T, t)
        for n in range(N):
            for grp in range(G):
                for s in range(Kg):
                    if s >= int(host["nsrc"][n * G + grp]):
                        candv[n * K + grp * Kg + s] = NAN
        want = DR.merge_state(host, candv, candi, N, K, Kg, V, end, t, lam)
        got = _merge(dev, host, candv, candi, N, K, Kg, V, end, t, lam)
        _same(got, want, (G, Kg, V, lam))
        assert bool((got["token"][0] == -7).all()) and bool((got["token"][2] == -7).all())


def test_merge_groups_hand_made_rules(dev):
    """diverse_beam_refs.hand_made: a tie between a penalised and an unpenalised candidate decided by the flat index, a
    word picked three times by earlier groups (c = 3), an <end> pick counted, a finished group in the middle that penalises
    nobody, nsrc_g < Kg -- the picks spelled out"""
    V, Kg, end, lam, candv, candi = DR.hand_made()
    N, K, G, T = 1, 6, 3, 1

    def start(nsrc, kk):
        g = torch.Generator().manual_seed(5)
        host = _state(g, N, G, Kg, T, 0)
        host["nsrc"], host["kk"] = torch.tensor(nsrc, dtype=torch.int32), torch.tensor(kk, dtype=torch.int32)
        host["ncomp"] = torch.tensor([Kg - k for k in kk], dtype=torch.int32)
        host["open_images"][0] = 1
        return host

    cv = candv.clone()
    cv[1] = cv[5] = NAN                               # slot 1 of groups 0 and 2 is dead
    host = start([1, 2, 1], [2, 2, 2])
    got = _merge(dev, host, cv, candi, N, K, Kg, V, end, 0, lam)
    _same(got, DR.merge_state(host, cv, candi, N, K, Kg, V, end, 0, lam), "all groups open")
    assert got["token"][0].tolist() == [3, 3, 3, 3, 4, 4] and got["parent"][0].tolist() == [0, 0, 3, 2, 4, 4]
    assert got["scores"].tolist() == [-1.0, 0.0, -0.25, -1.0, -1.75, 0.0]
    assert got["nsrc"].tolist() == [1, 2, 1] and got["ncomp"].tolist() == [1, 0, 1]
    assert got["comp_score"].tolist() == [-1.5, 0.0, 0.0, 0.0, -1.0, 0.0] and got["comp_parent"].tolist() == [0, 0, 0, 0, 4, 0]
    cv[2] = cv[3] = NAN                               # group 1 finished: its candidates are not read
    host = start([1, 0, 1], [2, 0, 2])
    got = _merge(dev, host, cv, candi, N, K, Kg, V, end, 0, lam)
    _same(got, DR.merge_state(host, cv, candi, N, K, Kg, V, end, 0, lam), "group 1 finished")
    assert got["token"][0].tolist() == [3, 3, -7, -7, 3, 3] and got["scores"][4:].tolist() == [-0.5, 0.0]
    assert got["comp_score"][4:].tolist() == [-1.0, 0.0] and int(got["open_images"]) == 1


def test_last_open_group_closes_the_image_and_a_closed_image_is_a_no_op(dev):
    """(G, Kg) = (2, 1): group 0 finished earlier, group 1 picks <end>: open_images drops by one; the same call again on the
    closed image writes nothing"""
    V, N, K, Kg, end = 8, 1, 2, 1, 7
    g = torch.Generator().manual_seed(3)
    host = _state(g, N, 2, Kg, 1, 0)
    host["nsrc"], host["kk"] = torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    host["ncomp"], host["open_images"][0] = torch.tensor([1, 0], dtype=torch.int32), 1
    candv = torch.tensor([[NAN, NAN], [-0.5, -1.0]])
    candi = torch.tensor([[0, 0], [7, 2]], dtype=torch.int32)
    got = _merge(dev, host, candv, candi, N, K, Kg, V, end, 0, 0.5)
    _same(got, DR.merge_state(host, candv, candi, N, K, Kg, V, end, 0, 0.5), "closing")
    assert int(got["open_images"]) == 0 and got["kk"].tolist() == [0, 0] and got["comp_score"].tolist()[1] == -0.5
    again = _merge(dev, got, candv, candi, N, K, Kg, V, end, 0, 0.5)
    _same(again, got, "closed image")


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("lam", [0.0, 0.5, 1e4])
def test_one_group_is_beam_merge_bit_for_bit(dev, V, lam):
    """G = 1, Kg = K = 5: every state array equals what scnattn_beam_merge writes from the same inputs, for any penalty"""
    N, K, T, t, end = 3, 5, 2, 1, V - 1
    g = torch.Generator().manual_seed(77 + V)
    candv, candi = _candidates(g, N, K, V)
    host = _state(g, N, 1, K, T, t)
    want = _merge(dev, host, candv, candi, N, K, K, V, end, t, lam, entry="scnattn_beam_merge")
    got = _merge(dev, host, candv, candi, N, K, K, V, end, t, lam)
    _same(got, want, (V, lam))


def test_merge_groups_refusals(dev):
    V, N, K, Kg = 8, 1, 4, 2
    g = torch.Generator().manual_seed(1)
    candv, candi = _candidates(g, N, K, V)
    host = _state(g, N, 2, Kg, 1, 0)
    for k, kg, lam in ((4, 3, 0.5), (4, 0, 0.5), (9, 3, 0.5), (4, 2, -1.0), (4, 2, float("nan")), (4, 2, float("inf"))):
        with pytest.raises(RuntimeError):
            _merge(dev, host, candv, candi, N, k, kg, V, V - 1, 0, lam)


# ---- the row selection with the group liveness ----------------------------------------------------------------------------
@pytest.mark.parametrize("V,passes", [(8, 0), (1003, 0), (1003, 1)])
@pytest.mark.parametrize("G,Kg", SHAPES)
def test_row_topk_groups_leaves_dead_slots_alone(dev, G, Kg, V, passes):
    """nsrc per (image, group) as in _state (a first step, part-way groups with finished ones, nsrc < Kg): the live rows are
    no prefix of an image's slots.  Logits of dead rows are NaN and their score too: read, they would poison a result; their
    rows of outv / outi still hold the sentinel afterwards, as do the words around the windows.  A live row holds the bits
    the plain selection (all rows live, dead rows zero-filled) writes for it."""
    N, K = 3, G * Kg
    R, ld = N * K, V + 3
    g = torch.Generator().manual_seed(500 + 10 * G + Kg + V)
    nsrc = _state(g, N, G, Kg, 1, 0)["nsrc"]
    live = torch.tensor([s < int(nsrc[n * G + grp]) for n in range(N) for grp in range(G) for s in range(Kg)])
    assert G == 1 or not all(bool(live[n * K:n * K + int(live[n * K:(n + 1) * K].sum())].all()) for n in range(N))
    logits = torch.randn(R, V, generator=g) * 3
    logits[:, :3] = logits[:, 3:6]                  # equal values inside a row: the tie rule at work
    scores = torch.randn(R, generator=g)

    def run(entry, lg, sc, ns, *kg):
        b_l, b_s = GBuf(dev, (R, V), (ld, 1), lg), GBuf(dev, (R,), None, sc)
        b_v, b_i = GBuf(dev, (R, K), None, out=True), GBuf(dev, (R, K), None, out=True)
        nd = ns.to(dev)
        _call(entry, dev, N, K, *kg, V, b_l.ptr, ld, b_s.ptr, C.c_void_p(nd.data_ptr()), b_v.ptr, b_i.ptr, passes)
        return b_v.read("outv"), b_i.read("outi").view(torch.int32)

    lg, sc = logits.clone(), scores.clone()
    lg[~live], sc[~live] = NAN, NAN
    gv, gi = run("scnattn_beam_row_topk_groups", lg, sc, nsrc, Kg)
    assert bool((gv[~live].view(torch.int32) == SENT).all()) and bool((gi[~live] == SENT).all()), "a dead slot's row was written"
    lg, sc = logits.clone(), scores.clone()
    lg[~live], sc[~live] = 0.0, 0.0
    pv, pi = run("scnattn_beam_row_topk", lg, sc, torch.full((N,), K, dtype=torch.int32))
    assert torch.equal(gv[live].view(torch.int32), pv[live].view(torch.int32)) and torch.equal(gi[live], pi[live])
    assert bool(torch.isfinite(gv[live]).all()) and bool(((gi[live] >= 0) & (gi[live] < V)).all())
    with pytest.raises(RuntimeError):
        run("scnattn_beam_row_topk_groups", lg, sc, nsrc, Kg + 1 if K % (Kg + 1) else K + 1)
