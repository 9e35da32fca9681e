"""CPU tests of the references of truncated sampling (tests/sampling_refs.py), of the host-side refusals and the bindings, and
of the caps the GPU modules assert, on the reference alone and for exactly their cases and seeds."""
import ctypes as C
import math
import os

import pytest
import torch

import beam_refs as BR
import rollout_refs as RR
import sampling_cases as SC
import sampling_refs as SR
from helpers import params_from, t

F64 = torch.float64
SEED = 0x1234abcd5678ef01


def _logits(R, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(R, V, generator=g, dtype=F64) * 2 - 1) * scale


# ---- the kept set ----------------------------------------------------------------------------------------------------------
def test_filter_off_is_the_plain_pick_exactly():
    x = _logits(5, 37, 1)
    for top_k, top_p in ((0, 1.0), (37, 1.0), (99, 1.0)):
        for greedy in (False, True):
            a = RR.pick(x, 5, 1.0 / 0.7, SEED, 2, 1, greedy)
            b = SR.pick(x, 5, 1.0 / 0.7, SEED, 2, 1, greedy, top_k, top_p)
            assert torch.equal(a["token"], b["token"]) and torch.equal(a["logp"], b["logp"]) and torch.equal(a["lse"], b["lse"])
            assert b["nkeep"] == [37] * 5 and bool(b["mask"].all())


def test_top_k_of_one_is_the_arg_max_and_tiny_top_p_keeps_one_word():
    x = _logits(6, 41, 2)
    x[0, 7] = x[0, 30] = 5.0                                       # equal maxima: the lower index
    for top_k, top_p in ((1, 1.0), (0, 1e-30), (0, 1e-6), (1, 0.3)):
        p = SR.pick(x, 1, 1.0, SEED, 0, 0, False, top_k, top_p)
        assert p["nkeep"] == [1] * 6
        assert p["token"].tolist() == [RR.first_in_order(x[i]) for i in range(6)] and p["token"][0] == 7
        assert bool((p["logp"] == 0).all()) and not bool(torch.signbit(p["logp"]).any())


def test_kept_set_is_a_prefix_of_the_order_and_grows_with_both_limits():
    x = torch.round(_logits(1, 300, 3)[0] * 4) / 4                 # ties everywhere
    o = SR.order(x)
    assert all((x[o[i]] > x[o[i + 1]]) or (x[o[i]] == x[o[i + 1]] and o[i] < o[i + 1]) for i in range(299))
    last = 0
    for k in (1, 2, 3, 10, 50, 299, 300, 0):
        n = SR.kept(x, k, 1.0)["nkeep"]
        assert n == (k if 1 <= k < 300 else 300) and n >= last
        last = n
    last = 0
    for p in (1e-6, 0.1, 0.3, 0.5, 0.8, 0.9, 0.99, 0.999999, 1.0):
        k = SR.kept(x, 0, p)
        n = k["nkeep"]
        assert n >= last and k["lo"] <= n <= k["hi"]
        if p < 1.0:                                                 # the shortest prefix that holds top_p of the mass
            assert float(k["c"][n - 1]) >= SR.f32(p) and (n == 1 or float(k["c"][n - 2]) < SR.f32(p))
        else:
            assert n == 300
        last = n
    for k, p in ((5, 0.9), (200, 0.5), (2, 0.999), (299, 0.5)):    # both: the shorter prefix, each measured on the FULL row
        assert SR.kept(x, k, p)["nkeep"] == min(SR.kept(x, k, 1.0)["nkeep"], SR.kept(x, 0, p)["nkeep"])


def test_ties_at_the_cut_go_by_index_and_minus_infinity_sorts_last():
    x = torch.tensor([1.0, 2.0, 1.0, 2.0, 1.0, float("-inf"), 1.0, -0.0, 0.0, float("-inf")], dtype=F64)
    assert SR.order(x).tolist() == [1, 3, 0, 2, 4, 6, 7, 8, 5, 9]
    p = SR.pick(x.unsqueeze(0), 1, 1.0, SEED, 0, 0, True, 4, 1.0)
    assert p["mask"][0].nonzero().reshape(-1).tolist() == [0, 1, 2, 3] and int(p["token"][0]) == 1
    e, m = SR.terms(x)
    assert float(m) == 2.0 and float(e[5]) == 0.0 and float(e[9]) == 0.0
    flat = torch.full((9,), 0.5, dtype=F64)
    k = SR.kept(flat, 0, 0.5)
    assert k["nkeep"] == 5 and k["order"].tolist() == list(range(9))
    k = SR.kept(torch.full((8,), 0.5, dtype=F64), 0, 0.5)          # c_4 == top_p exactly: inside the band, both ends accepted
    assert (k["nkeep"], k["lo"], k["hi"], k["sharp"]) == (4, 4, 5, False)


def test_band_and_range_of_a_near_threshold_row():
    x = _logits(1, 200, 5)[0]
    k = SR.kept(x, 0, 0.7)
    assert k["sharp"] and k["lo"] == k["hi"] == k["nkeep"]
    assert math.isclose(SR.band_m(x), RR.U * (2 * float(x.max() - x.min()) + 16))
    p = SR.pick(x.unsqueeze(0), 1, 1.0, SEED, 0, 0, False, 0, 0.7)
    tok = int(p["token"][0])
    assert SR.nkeep_ok(p, 0, k["nkeep"]) and not SR.nkeep_ok(p, 0, k["nkeep"] + 1)
    assert SR.token_ok(p, 0, tok, k["nkeep"])
    outside = int(k["order"][k["nkeep"]])
    assert not SR.token_ok(p, 0, outside, k["nkeep"])
    want, bound = SR.logp_at(p, 0, tok, k["nkeep"])
    assert abs(want - float(p["logp"][0])) < 1e-12 and 0 < bound < 1e-5


def test_token_frequencies_follow_the_truncated_softmax():
    """4.5 binomial standard deviations per kept word, as the plain rollout's test; words outside are never drawn"""
    V, draws = 12, 2000
    x = _logits(1, V, 6, scale=1.5)
    for top_k, top_p in ((4, 1.0), (0, 0.8), (6, 0.9)):
        k = SR.kept(x[0], top_k, top_p)
        idx = k["order"][:k["nkeep"]]
        prob = torch.zeros(V, dtype=F64)
        prob[idx] = torch.softmax(x[0][idx], 0)
        count = torch.zeros(V)
        for d in range(draws):
            count[int(SR.pick(x, 1, 1.0, SEED, d, 3, False, top_k, top_p)["token"][0])] += 1
        for v in range(V):
            sd = math.sqrt(draws * float(prob[v]) * (1 - float(prob[v])))
            assert abs(float(count[v]) - draws * float(prob[v])) <= 4.5 * sd + 1e-9, (top_k, top_p, v, float(count[v]))
        assert 1 < k["nkeep"] < V


@pytest.mark.parametrize("name,kind", BR.FIXTURES[:2] + BR.FIXTURES[3:])
def test_filtered_rollout_sum_logp_is_the_sum_of_its_truncated_log_probabilities(name, kind):
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    P64 = params_from(d, dtype=F64)
    enc = t(d["enc"]).double()[:2]
    tags = t(d["tags"]).double()[:2] if kind != "pure_attention" else None
    K = 2
    res = SR.rollout(kind, P64, K, wm, enc, tags, seed=11, draw=4, inv_temp=1.0 / 0.7, greedy_first=True, top_k=4, top_p=0.9,
                     max_steps=12)
    plain = RR.rollout(kind, P64, K, wm, enc, tags, seed=11, draw=4, inv_temp=1.0 / 0.7, greedy_first=True, max_steps=12)
    for r in range(2 * K):
        n = SR.open_steps(res, r)
        assert abs(sum(res["logp"][r]) - res["sum_logp"][r]) <= 1e-9 * max(1.0, abs(res["sum_logp"][r]))
        assert all(1 <= res["nkeep"][s][r] <= 4 for s in range(n))
        assert all(x <= 1e-12 for x in res["logp"][r])
        if r % K == 0:                      # the arg-max slot: the same caption, a likelihood no smaller than the full softmax's
            assert RR.caption_of(res, r, V - 2)[:n + 1] == RR.caption_of(plain, r, V - 2)[:n + 1]
            assert res["length"][r] == 0 or res["sum_logp"][r] >= plain["sum_logp"][r] - 1e-9
    r32 = SR.rollout(kind, params_from(d, dtype=torch.float32), K, wm, enc.float(), None if tags is None else tags.float(),
                     seed=11, draw=4, inv_temp=1.0 / 0.7, greedy_first=True, top_k=4, top_p=0.9, max_steps=12,
                     tokens=res["tokens"])
    assert len(SR.decidable_rows(res, r32)) == 2 * K
    assert RR.pick is not None and RR.pick.__module__ == "rollout_refs"        # the plain pick is back in place


# ---- refusals on the host -----------------------------------------------------------------------------------------------
def _dims(V=50):
    return (2, 4, 8, 8, 8, 8, 8, 3, V, 51, 51, 1)


BAD_FILTERS = ((-1, 1.0, "top_k"), (2.5, 1.0, "top_k"), (0, 0.0, "top_p"), (0, -0.1, "top_p"), (0, 1.0001, "top_p"),
               (0, float("nan"), "top_p"), (0, float("inf"), "top_p"), (0, 1e-60, "top_p"))


def test_host_side_refusals_of_the_filter():
    from models.decoders._common import check_rollout_args
    from scnattn import functional as SF
    x = torch.zeros(1)
    for top_k, top_p, what in BAD_FILTERS:
        with pytest.raises(ValueError, match=what):
            check_rollout_args(2, 1.0, top_k=top_k, top_p=top_p)
        with pytest.raises(ValueError, match=what):
            SF.rollout_run(_dims(), 2, (), x, x, 48, 49, 0, 0, top_k=top_k, top_p=top_p)
    assert check_rollout_args(3, 1.0, True, top_k=50, top_p=0.9) == 4
    assert SF.sample_filter_struct(0, 1.0) is None
    f = SF.sample_filter_struct(50, 0.9)
    assert f.top_k == 50 and f.top_p == SR.f32(0.9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a good filter goes on to the device check
        SF.rollout_run(_dims(), 2, (), x, x, 48, 49, 0, 0, top_k=5, top_p=0.9)


_P = 1 << 20        # any non-null, 16-byte aligned address: the checks must reject the call before it is dereferenced


def _refused(h, rc, text):
    assert rc == -1
    assert text in h.scnattn_last_error().decode(), h.scnattn_last_error()


def test_entry_points_refuse_before_launching_and_the_layout_adds_nkeep():
    from scnattn import _lib as L
    h = L.lib()
    d = L.Dims(*_dims())
    w = L.Params()
    nbytes, off, off0 = C.c_size_t(), (C.c_long * L.ROLLOUT_NOFF_F)(), (C.c_long * L.ROLLOUT_NOFF)()
    state = (C.c_void_p * 7)(*([_P] * 7))
    for top_k, top_p in ((-1, 1.0), (0, 0.0), (0, -1.0), (0, 1.5), (0, float("nan")), (3, float("inf"))):
        f = L.SampleFilter(top_k=top_k, top_p=top_p)
        _refused(h, h.scnattn_rollout_workspace_f(C.byref(d), 2, 51, 0, C.byref(f), C.byref(nbytes)), "sample filter")
        _refused(h, h.scnattn_rollout_layout_f(C.byref(d), 2, 51, 0, C.byref(f), off), "sample filter")
        _refused(h, h.scnattn_rollout_init_f(None, C.byref(d), 2, 51, 0, C.byref(f), C.byref(w), _P, _P, 48, _P), "sample filter")
        _refused(h, h.scnattn_rollout_steps_f(None, C.byref(d), 2, 51, 0, C.byref(f), C.byref(w), _P, 49, 1.0, 1, 0, 0, 0, 1, _P),
                 "sample filter")
        _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, state, C.byref(f), _P, 0),
                 "top_k >= 0 and 0 < top_p <= 1")
    f = L.SampleFilter(top_k=5, top_p=0.9)
    _refused(h, h.scnattn_rollout_workspace_f(C.byref(d), 2, 51, 0, None, C.byref(nbytes)), "filter is NULL")
    _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, state, None, _P, 0), "filter is NULL")
    _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, state, C.byref(f), None, 0),
             "nkeep record is NULL")
    # everything _pick refuses, filter on and off
    for flt in (f, L.SampleFilter(top_k=0, top_p=1.0)):
        _refused(h, h.scnattn_rollout_pick_f(None, 2, 9, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, state, C.byref(flt), _P, 0), "slot count")
        _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 49, 1.0, 1, 0, 0, 0, 49, 51, state, C.byref(flt), _P, 0), "bad argument")
        _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 50, 0.0, 1, 0, 0, 0, 49, 51, state, C.byref(flt), _P, 0), "inv_temp")
        _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 51, 0, 49, 51, state, C.byref(flt), _P, 0),
                 "step beyond the records")
        _refused(h, h.scnattn_rollout_pick_f(None, 2, 2, 50, _P, 50, 1.0, 1, 0, 0, 0, 49, 51, None, C.byref(flt), _P, 0), "state is NULL")
    _refused(h, h.scnattn_rollout_steps_f(None, C.byref(d), 2, 51, 0, C.byref(f), C.byref(w), _P, 49, 0.0, 1, 0, 0, 0, 1, _P), "inv_temp")
    _refused(h, h.scnattn_rollout_init_f(None, C.byref(d), 2, 51, 0, C.byref(f), C.byref(w), _P, _P, 50, _P), "start token")
    # the layout: the eight offsets of the plain form, unchanged, then nkeep int[max_steps][N*K] inside the workspace
    for want_alpha in (0, 1):
        small = C.c_size_t()
        assert h.scnattn_rollout_workspace(C.byref(d), 3, 51, want_alpha, C.byref(small)) == 0
        assert h.scnattn_rollout_workspace_f(C.byref(d), 3, 51, want_alpha, C.byref(f), C.byref(nbytes)) == 0
        assert h.scnattn_rollout_layout(C.byref(d), 3, 51, want_alpha, off0) == 0
        assert h.scnattn_rollout_layout_f(C.byref(d), 3, 51, want_alpha, C.byref(f), off) == 0
        assert list(off)[:8] == list(off0)
        rec = 51 * 6
        assert 4 * rec <= nbytes.value - small.value < 4 * rec + 256
        assert off[8] % 4 == 0 and off[8] >= max(off[6] + rec, off[7] + 51 * 6 * 4 if want_alpha else 0)
        assert 4 * (off[8] + rec) <= nbytes.value


def test_header_declares_the_new_symbols_and_keeps_the_version():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "scnattn.h")).read()
    from scnattn import _lib as L
    h = L.lib()
    for sym in ("scnattn_rollout_workspace_f", "scnattn_rollout_layout_f", "scnattn_rollout_init_f", "scnattn_rollout_steps_f",
                "scnattn_rollout_pick_f"):
        assert "int %s(" % sym in header and sym in L.EXPORTS and getattr(h, sym) is not None
    assert "#define SCNATTN_VERSION 109 " in header and h.scnattn_version() == 109
    assert "#define SCNATTN_ROLLOUT_NOFF_F %d" % L.ROLLOUT_NOFF_F in header and L.ROLLOUT_NOFF_F == L.ROLLOUT_NOFF + 1
    assert "} scnattn_sample_filter;" in header and C.sizeof(L.SampleFilter) == 8
    assert [n for n, _ in L.SampleFilter._fields_] == ["top_k", "top_p"]


# ---- the caps of the GPU modules, on the reference alone --------------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(SC.CONFIGS))
@pytest.mark.parametrize("V", SC.VS)
def test_kernel_cases_keep_their_share_of_sharp_rows(V, cfg):
    sharp, judged = SC.sharp_share_on_reference(V, cfg, SC.runs_of(V, cfg))
    assert judged > 0 and sharp >= SC.SHARP_SHARE * judged, (sharp, judged)
    kinds = {r["kind"] for r in SC.runs_of(V, cfg)}
    assert kinds == set(SC.KINDS)


@pytest.mark.parametrize("name,V,cfg,which,force_passes,salt", SC.EXTRA, ids=[e[0] for e in SC.EXTRA])
def test_large_and_passes_cases_keep_their_share_of_sharp_rows(name, V, cfg, which, force_passes, salt):
    sharp, judged = SC.sharp_share_on_reference(V, cfg, SC.runs_of(V, cfg, which, salt))
    assert judged > 0 and sharp >= SC.SHARP_SHARE * judged, (name, sharp, judged)


def test_every_filter_meets_every_kind_of_logits_on_both_load_paths():
    seen = set()
    for V in SC.VS:
        for cfg in SC.CONFIGS:
            for fi, r in enumerate(SC.runs_of(V, cfg)):
                seen.add((fi, r["kind"]))
                seen.add(("mis", fi, r["mis"]))
    assert all((fi, k) in seen for fi in range(10) for k in SC.KINDS)
    assert all(("mis", fi, m) in seen for fi in range(10) for m in (0, 1))


def test_driver_cases_keep_their_caps_on_rows_left_out():
    """tests/test_gpu_sampling.py: at most 1/2 of any fixture's rows and 1/4 of the table's are left out by the extended
    decidability rule; the table holds a row that uses all steps, one that ends at once, and nucleus cuts of several sizes"""
    rows = out = 0
    lens, nkeeps = [], set()
    for name, kind in BR.FIXTURES:
        for K in (1, 3):
            for filt in sorted(SC.DRIVER_FILTERS):
                _, _, _, _, _, _, ref, ok = SC.fixture_case(name, kind, K, filt)
                left = len(ok) - sum(ok)
                assert 2 * left <= len(ok), (name, K, filt, left)
                rows, out = rows + len(ok), out + left
                lens += ref["length"]
                top_k = SC.DRIVER_FILTERS[filt][0]
                for r in range(len(ok)):
                    for s in range(SR.open_steps(ref, r)):
                        nkeeps.add((filt, ref["nkeep"][s][r]))
                        assert not top_k or ref["rank"][s][r] < top_k
    assert 4 * out <= rows, (out, rows)
    assert 0 in lens and 1 in lens
    assert ("k3", 3) in nkeeps and ("k4p0.9", 4) in nkeeps
    assert len({n for f, n in nkeeps if f == "p0.8"}) >= 4, "top_p alone must cut at several places"
    _, _, _, _, _, _, ref, ok = SC.vector_case()
    assert 4 * (len(ok) - sum(ok)) <= len(ok)
