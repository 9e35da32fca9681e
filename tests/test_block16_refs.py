"""CPU tests of tests/block16_refs.py, the stage-wise fp64 reference of the bf16 Bottleneck drivers (csrc/block16.cpp,
scnattn/conv16.py): an honest fp32 / bf16 evaluation of the driver's sequence passes every judge on every geometry over two
consecutive steps (the bounds are attainable without a GPU), every planted composition defect is caught on a geometry that
`applies` names, the case table reaches every branch of csrc/block16.cpp, and the test's own carve of save / tmp equals
scnattn_block16_sizes (host only: the library loads without a GPU)."""
import ctypes as C

import pytest
import torch

import block16_refs as R

_EVAL = {}


def _steps(g, defect=None, variant="full"):
    """[(state, S)] of the evaluator over the consecutive steps, computed once per (geometry, defect, variant)"""
    key = (g.id, defect, variant)
    if key not in _EVAL:
        I = R.inputs(g)
        state, out = R.first_state(I), []
        for t in range(R.STEPS):
            S = R.cpu_eval(g, I, t, state, defect, variant)
            out.append((state, S))
            state = R.next_state(g, S)
        _EVAL[key] = out
    return _EVAL[key]


@pytest.mark.parametrize("variant", ["full", "no_dx", "no_dw", "conv2_frozen"])
@pytest.mark.parametrize("g", R.GEOMS, ids=[g.id for g in R.GEOMS])
def test_the_cpu_evaluation_passes_every_judge(g, variant):
    I = R.inputs(g)
    for t, (state, S) in enumerate(_steps(g, None, variant)):
        T = R.judge_step(g, I, t, state, S, variant)
        worst = max(T.ratios.items(), key=lambda kv: kv[1])
        print("%s %s step %d: %d results, worst err/bound %.3f (%s)" % (g.id, variant, t, len(T.ratios), worst[1], worst[0]))
        assert not T.fails, "%s step %d: %s" % (g.id, t, "; ".join(T.fails))
        assert worst[1] <= 1.0
    assert not torch.equal(I["x"][0], I["x"][1])


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    """each defect fails at least one judge on at least one geometry `applies` names (printed: which, and the first failure)"""
    caught = []
    named = [g for g in R.GEOMS if R.applies(defect, g)]
    assert named, defect
    for g in named:
        I = R.inputs(g)
        fails = []
        for t, (state, S) in enumerate(_steps(g, defect)):
            fails += R.judge_step(g, I, t, state, S).fails
        if fails:
            caught.append(g.id)
            print("%-18s caught on %-6s %s" % (defect, g.id, fails[0]))
    assert caught, "%s passes every judge on %s" % (defect, [g.id for g in named])


def test_the_case_table_reaches_every_branch_of_the_driver():
    """has_down x stride, need_dx 0 and 1, a null and a non-null dw[i] for every i"""
    seen = set()
    for g in R.GEOMS:
        for v in R.VARIANTS:
            seen |= R.branches(g, v)
    kinds = {(g.down, g.s) for g in R.GEOMS}
    assert kinds == {(0, 1), (1, 1), (1, 2)}          # an identity block at stride 2 is refused
    want = {("has_down", 0), ("has_down", 1), ("stride", 1), ("stride", 2), ("need_dx", 0), ("need_dx", 1)}
    want |= {("dw%d" % i, v) for i in range(4) for v in (0, 1)}
    assert want <= seen, want - seen
    # the GPU module runs full, no_dx and no_dw on every geometry: each kind of block meets need_dx = 0 and a null dw[i]
    assert {"full", "no_dx", "no_dw"} <= set(R.VARIANTS)
    assert R.VARIANTS["no_dx"][0] == 0 and not any(R.VARIANTS["no_dw"][1]) and R.VARIANTS["conv2_frozen"][1] == (1, 0, 1, 1)


def test_the_defects_name_geometries_of_the_table():
    for defect in R.DEFECTS:
        assert any(R.applies(defect, g) for g in R.GEOMS), defect
    with_partial = [g.id for g in R.GEOMS if R.applies("drop_last_tile", g)]
    assert with_partial == ["i306", "d2"]


@pytest.mark.parametrize("g", R.GEOMS, ids=[g.id for g in R.GEOMS])
def test_the_carve_equals_the_librarys_sizes(g):
    """cumulative piece sizes in the header's order against scnattn_block16_sizes; part_floats against scnattn/block.py"""
    from scnattn import _lib, block as B
    from scnattn.conv16 import _Block16
    h = _lib.lib()
    b = _Block16(g.N, g.Cin, g.Hi, g.Wi, g.p, g.s, g.down)
    sz = [C.c_long(-1) for _ in range(5)]
    assert h.scnattn_block16_sizes(C.byref(b), *[C.byref(v) for v in sz]) == 0, h.scnattn_last_error()
    cv, d = R.carve(g), R.dims(g)
    assert [v.value for v in sz] == [cv["save_elems"], cv["out_offset"], cv["stats_floats"], cv["tmp_elems"], cv["dgb_floats"]]
    off, rows, cols = cv["save"]["idn" if g.down else "out"]
    assert off + rows * cols == cv["save_elems"]      # nothing behind the last piece
    geo = B.Geom(g.N, g.Cin, g.Hi, g.Wi, g.p, d["C4"], g.s, d["Ho"], d["Wo"], d["Rin"], d["Rout"])
    assert R.part_floats(g) == B.part_floats(geo)
    assert h.scnattn_cgemm_stat_ld(d["Rin"]) == R.CR.stat_ld(d["Rin"]) and h.scnattn_cgemm_row_tiles(d["Rout"]) == R.CR.row_tiles(d["Rout"])


def test_sizes_refuses_what_the_driver_cannot_run():
    from scnattn import _lib
    from scnattn.conv16 import _Block16
    h = _lib.lib()
    for args, text in (((2, 256, 8, 8, 96, 1, 0), b"multiples of 64"), ((2, 256, 6, 5, 64, 2, 1), b"even maps"),
                       ((2, 128, 8, 8, 64, 1, 0), b"keeps its shape"), ((2, 256, 8, 8, 64, 2, 0), b"keeps its shape"),
                       ((2, 256, 8, 8, 64, 3, 1), b"geometry")):
        b = _Block16(*args)
        sz = [C.c_long(-1) for _ in range(5)]
        assert h.scnattn_block16_sizes(C.byref(b), *[C.byref(v) for v in sz]) == -1
        assert text in h.scnattn_last_error(), h.scnattn_last_error()
        assert all(v.value == -1 for v in sz)


def test_the_driver_refuses_before_it_launches():
    """Every refusal of tests/block16_refs.refusals on HOST dummy buffers, without a GPU: -1 and the message.  (That a refused
    call writes nothing is the GPU module's part: tests/test_gpu_block16_driver.py.)"""
    from scnattn import _lib
    from scnattn.conv16 import _Block16
    h = _lib.lib()
    g = R.by_id(R.REFUSAL_GEOM)
    keep = torch.zeros(64)
    ptr = keep.data_ptr()
    valid = _Block16(g.N, g.Cin, g.Hi, g.Wi, g.p, g.s, g.down)
    for name in ("gamma", "beta", "run_mean", "run_var", "shift", "w", "wt", "dw"):
        for i in range(4):
            getattr(valid, name)[i] = ptr
    for name in ("ws", "part", "bnpart", "x", "save", "stats", "dout", "tmp", "dgb"):
        setattr(valid, name, ptr)
    valid.ws_floats, valid.bnpart_floats, valid.need_dx = 64, R.part_floats(g), 1
    n = 0
    for kw, calls, text in R.refusals(g):
        b = _Block16.from_buffer_copy(valid)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(b, k)[v[0]] = v[1]
            else:
                setattr(b, k, v)
        for which in calls:
            dxp, dxdp = C.c_void_p(1), C.c_void_p(1)
            rc = h.scnattn_block16_fwd(None, C.byref(b)) if which == "fwd" else \
                h.scnattn_block16_bwd(None, C.byref(b), C.byref(dxp), C.byref(dxdp))
            msg = h.scnattn_last_error()
            assert rc == -1 and text in msg and b"block16" in msg, (kw, which, rc, msg)
            n += 1
    assert n >= 40
