"""scnattn_plan_next (include/scnattn.h) without a GPU: the arming protocol, and the one split rule of cgemm_plan
(csrc/cgemm.hip) that no case table reaches, against rows worked by hand.  Every call here is a plan query or a refusal on
host memory: nothing is launched."""
import ctypes as C

import pytest
import torch

from scnattn import _lib as L

PRESET = 99         # what a test writes into `family` to see whether the library touched the struct


def _cgemm_args(M, N, K, ws_slabs=0, lda=None):
    """scnattn_cgemm, NT layout, plain product: (keep-alive tensors, argument list without the stream)"""
    a, b, c = torch.empty(M * K + 16), torch.empty(N * K + 16), torch.empty(M * N + 16)
    ws = torch.empty(ws_slabs * M * N + 16) if ws_slabs else None
    assert all(t.data_ptr() % 16 == 0 for t in (a, b, c))
    args = [0, 1, M, N, K, 1.0, a.data_ptr(), K if lda is None else lda, b.data_ptr(), K, 0.0, c.data_ptr(), N, None, None, 1,
            0, 0, 0, None if ws is None else ws.data_ptr(), ws_slabs * M * N, None]
    return (a, b, c, ws), args


def _armed(out):
    L.check(L.lib().scnattn_plan_next(None if out is None else C.byref(out)), "scnattn_plan_next")


def _refused():
    """an un-plannable call: lda % 4 != 0 is refused before anything could be launched -> (rc, message)"""
    keep, args = _cgemm_args(8, 8, 8, lda=9)
    rc = L.lib().scnattn_cgemm(None, *args)
    return rc, L.lib().scnattn_last_error().decode()


def test_arming_is_consumed_by_one_call():
    out = L.LaunchPlan(family=PRESET)
    keep, args = _cgemm_args(64, 64, 16)
    _armed(out)
    assert L.lib().scnattn_cgemm(None, *args) == 0
    assert (out.family, out.mi, out.S, out.grid_x, out.grid_y) == (L.PLAN_CGEMM, 2, 1, 1, 1)
    # the thread is disarmed: a refusal now leaves the struct alone (an armed one would clear it)
    rc, msg = _refused()
    assert rc == -1 and "operand alignment / size not supported" in msg and out.family == L.PLAN_CGEMM


def test_refusal_disarms_and_keeps_its_message():
    out = L.LaunchPlan(family=PRESET)
    _armed(out)
    rc, msg = _refused()
    assert rc == -1 and "cgemm: operand alignment / size not supported" in msg and out.family == L.PLAN_NONE
    out.family = PRESET
    assert _refused()[0] == -1 and out.family == PRESET
    keep, args = _cgemm_args(8, 8, 8, lda=9)
    with pytest.raises(RuntimeError, match="cgemm: operand alignment / size not supported"):
        L.plan("scnattn_cgemm", None, *args)


def test_empty_problem_gives_family_0():
    out = L.LaunchPlan(family=PRESET)
    keep, args = _cgemm_args(8, 8, 8)
    args[2] = 0                                     # M = 0: the early return
    _armed(out)
    assert L.lib().scnattn_cgemm(None, *args) == 0 and out.family == L.PLAN_NONE
    out.family = PRESET
    assert _refused()[0] == -1 and out.family == PRESET         # and it disarmed
    assert L.plan("scnattn_cgemm", None, *args).family == L.PLAN_NONE


def test_null_disarms_and_a_second_arming_replaces_the_first():
    first, second = L.LaunchPlan(family=PRESET), L.LaunchPlan(family=PRESET)
    _armed(first)
    _armed(None)
    assert _refused()[0] == -1 and first.family == PRESET
    keep, args = _cgemm_args(64, 64, 16)
    _armed(first)
    _armed(second)
    assert L.lib().scnattn_cgemm(None, *args) == 0
    assert first.family == PRESET and second.family == L.PLAN_CGEMM
    assert _refused()[0] == -1 and second.family == L.PLAN_CGEMM


def test_every_family_answers_through_its_entry_point():
    """sgemm_ws hands an aligned product on to cgemm and keeps an unaligned one; the skinny entry reports its slices"""
    keep, args = _cgemm_args(64, 64, 16)
    assert L.plan("scnattn_sgemm_ws", None, *args[:-1]).family == L.PLAN_CGEMM
    keep, args = _cgemm_args(37, 53, 29)
    p = L.plan("scnattn_sgemm_ws", None, *args[:-1])
    assert (p.family, p.vec, p.S, p.grid_x, p.grid_y, p.grid_z) == (L.PLAN_SGEMM, 0, 1, 1, 1, 1)
    x, w, y, used = torch.empty(32 * 512), torch.empty(512 * 128), torch.empty(16 * 32 * 128), C.c_int(-1)
    p = L.plan("scnattn_skinny_gemm", None, 32, 128, 512, 1, x.data_ptr(), 512, 0, w.data_ptr(), 128, 0, y.data_ptr(), 128, 0,
               32 * 128, 0, C.byref(used))
    assert (p.family, p.S, p.grid_y, p.nb, p.chunks, p.kslice) == (L.PLAN_SKINNY, used.value, used.value, 1, 1, 32)


# The second split rule of cgemm_plan: a grid of one to three residency rounds (224 <= tiles < 768) of a deep product
# (K >= 1536, no 3x3 mode, default cgemm_target) that the first rule left un-split is split to ~1200 workgroups,
# S = (1200 + tiles / 2) / tiles, at most K / 256 and what the workspace holds; kper = ceil(K / S) in whole 16s.
#   10000 x 512 x 1632: ceil(10000 / 128) * 4 = 316 tiles of 128 rows (>= 256: the 128-row tile stays), (1200 + 158) / 316 = 4,
#       K / 256 = 6, kper = ceil(408 / 16) * 16 = 416, ceil(1632 / 416) = 4
#   6272 x 512 x 2048: 49 * 4 = 196 128-row tiles (< 256) -> 64-row tiles, 98 * 4 = 392; (1200 + 196) / 392 = 3, K / 256 = 8,
#       kper = ceil(682.67 / 16) * 16 = 688, ceil(2048 / 688) = 3
# S <= cgemm_combine_max = 8, 16-byte stores, the slab stack below 2 GiB: both are finished inside the launch.
@pytest.mark.parametrize("M,N,K,mi,S,kper", [(10000, 512, 1632, 2, 4, 416), (6272, 512, 2048, 1, 3, 688)])
def test_second_split_rule_against_hand_worked_rows(M, N, K, mi, S, kper):
    keep, args = _cgemm_args(M, N, K, ws_slabs=4)
    p = L.plan("scnattn_cgemm", None, *args)
    assert (p.family, p.tA, p.tB, p.mi, p.S, p.kper) == (L.PLAN_CGEMM, 0, 1, mi, S, kper)
    assert p.in_launch == 1 and p.second == L.SECOND_NONE and p.vec == 1 and (p.grid_x, p.grid_y) == (p.tiles, S)
    # without a workspace the product stays whole
    keep, args = _cgemm_args(M, N, K)
    p = L.plan("scnattn_cgemm", None, *args)
    assert (p.mi, p.S, p.in_launch, p.second) == (mi, 1, 0, L.SECOND_NONE)
