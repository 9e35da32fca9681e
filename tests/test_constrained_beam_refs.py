"""tests/constrained_beam_refs.py against itself and against tests/beam_refs.py (no GPU): empty lists are the plain search,
the merge's rules on hand-worked candidates, the invariants of whole searches, the refusals -- the restatement's, the
Python layer's and the C calls' that need no device -- and the caps of the tables that
tests/test_gpu_constrained_beam_search.py compares, asserted here from the restatement alone."""
import ctypes as C
import os
import re

import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
import constrained_beam_refs as CR
from helpers import params_from, t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["scnattn_beam_%s_con" % x for x in ("workspace", "layout", "init", "steps")] + \
      ["scnattn_ensemble_%s_con" % x for x in ("workspace", "layout", "init", "steps")] + \
      ["scnattn_beam_row_topk_con", "scnattn_beam_row_topk_ens_con", "scnattn_beam_merge_banks"]
NEG = -float("inf")


# ---- empty lists: the plain search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", BR.FIXTURES)
def test_empty_lists_are_beam_refs_search(name, kind):
    """C_n = 0 for every image: one bank, nothing extra excluded, the picks are the top kk -- results EQUAL beam_refs.search
    on every fixture and beam size"""
    d, V = BR.sharpened(name)
    wm = BR.word_map(V)
    P = params_from(d, dtype=torch.float64)
    enc = t(d["enc"]).double()
    tags = t(d["tags"]).double() if kind != "pure_attention" else None
    for k in BR.BEAMS:
        want = BR.search(kind, P, k, wm, enc, tags)
        got, _, masks = CR.search_one(kind, P, k, wm, enc, tags, [[] for _ in range(enc.shape[0])])
        assert got == want and masks == [0] * enc.shape[0], (name, k)


def test_an_empty_list_in_a_mixed_batch_is_the_plain_result():
    kind, seed = OR.SEEDS[0]
    d, V, enc, tags = OR.inputs(kind, seed)
    wm = BR.word_map(V)
    P = params_from(d, dtype=torch.float64)
    req = CR.required_words(kind, seed, (4, 11))
    req[1] = []
    got, _, masks = CR.search_one(kind, P, 3, wm, enc.double(), tags.double(), req)
    plain, _ = OR.search_one(kind, P, 3, wm, enc.double(), tags.double())
    assert got[1] == plain[1] and masks[1] == 0
    assert got[0] != plain[0] and masks[0] == 3


# ---- the merge, by hand -----------------------------------------------------------------------------------------------------
def _rows(rows):
    """[(ordinary [(value, word)], required [(value, word) or None] * 4)] -> candv, candi, reqv, reqi"""
    K = len(rows[0][0])
    cv = torch.tensor([[v for v, _ in o] for o, _ in rows], dtype=torch.float64)
    ci = torch.tensor([[w for _, w in o] for o, _ in rows])
    rv = torch.tensor([[NEG if x is None else x[0] for x in r] for _, r in rows], dtype=torch.float64)
    ri = torch.tensor([[-1 if x is None else x[1] for x in r] for _, r in rows])
    assert cv.shape == (len(rows), K)
    return cv, ci, rv, ri


def test_merge_one_required_word_end_only_from_the_met_row_and_kk_below_k():
    """V = 100, <end> = 99, C = 1.  Row 0 has not met the word (bank 0; its required candidate lies in bank 1), row 1 has (bank
    1, and only it may offer <end>).  Bank 1 in order: (-1.5, row 1 word 8), (-2.5, row 1 <end>), (-3.5, row 1 word 9),
    (-4.0, row 0's required word 42).  kk = 3: bank 1, bank 0, bank 1 -- then arranged by value."""
    V = 100
    cv, ci, rv, ri = _rows([([(-1.0, 5), (-2.0, 6), (-3.0, 7)], [(-4.0, 42), None, None, None]),
                            ([(-1.5, 8), (-2.5, 99), (-3.5, 9)], [None] * 4)])
    mets = [0, 1]
    assert CR.merge_banks(cv, ci, rv, ri, mets, V, 1, 3) == [(-1.0, 0, 5, 0), (-1.5, 1, 8, 1), (-2.5, 1, 99, 1)]
    assert CR.merge_banks(cv, ci, rv, ri, mets, V, 1, 1) == [(-1.5, 1, 8, 1)]           # kk < K: the highest bank first
    assert CR.merge_banks(cv, ci, rv, ri, mets, V, 1, 2) == [(-1.0, 0, 5, 0), (-1.5, 1, 8, 1)]
    # only row 0 live: its required word is bank 1's only candidate, however low its value
    assert CR.merge_banks(cv[:1], ci[:1], rv[:1], ri[:1], mets[:1], V, 1, 3) == [(-1.0, 0, 5, 0), (-2.0, 0, 6, 0), (-4.0, 0, 42, 1)]


def test_merge_four_required_words_and_a_bank_that_runs_dry():
    """C = 4, one live row that has met words 0 and 1 (bank 2): its two open words are bank 3's candidates, banks 4, 1 and 0
    are empty.  kk = 3: bank 3, bank 2, bank 3 (now dry); kk = 4 goes on in bank 2.  The children's masks carry the new bit."""
    V = 100
    cv, ci, rv, ri = _rows([([(-1.0, 10), (-2.0, 11), (-3.0, 12), (-3.5, 13)], [None, None, (-5.0, 52), (-0.5, 53)])])
    assert CR.merge_banks(cv, ci, rv, ri, [0b0011], V, 4, 3) == [(-0.5, 0, 53, 0b1011), (-1.0, 0, 10, 0b0011), (-5.0, 0, 52, 0b0111)]
    assert CR.merge_banks(cv, ci, rv, ri, [0b0011], V, 4, 4) == [(-0.5, 0, 53, 0b1011), (-1.0, 0, 10, 0b0011),
                                                                  (-2.0, 0, 11, 0b0011), (-5.0, 0, 52, 0b0111)]


def test_merge_ties_across_rows_and_across_banks():
    """equal values everywhere: within a bank the lower flat index (the lower row) wins; the picked set is arranged by flat
    index among equal values, whatever bank a pick came from"""
    V = 100
    row = ([(-1.0, 3), (-2.0, 4)], [(-1.0, 7), None, None, None])
    cv, ci, rv, ri = _rows([row, row])
    assert CR.merge_banks(cv, ci, rv, ri, [0, 0], V, 1, 2) == [(-1.0, 0, 3, 0), (-1.0, 0, 7, 1)]
    # swapped words: the required word has the lower index and now comes first among the equal values
    row = ([(-1.0, 7), (-2.0, 8)], [(-1.0, 3), None, None, None])
    cv, ci, rv, ri = _rows([row, row])
    assert CR.merge_banks(cv, ci, rv, ri, [0, 0], V, 1, 2) == [(-1.0, 0, 3, 1), (-1.0, 0, 7, 0)]


def test_row_select_end_and_required_candidates():
    """<end> is the row's best word: absent while a requirement is open, first once the mask is complete; an unmet required
    word never among the ordinary candidates, a met one may be; a required word the options exclude is not offered"""
    V, end, K = 12, 11, 3
    val = torch.tensor([[-float(v) for v in range(V)]], dtype=torch.float64)
    val[0, end] = 1.0
    req = [2, 0]
    cv, ci, rv, ri = CR.row_select(val, [set()], [req], [0b00], K, end)
    assert ci.tolist() == [[1, 3, 4]] and ri.tolist() == [[2, 0, -1, -1]] and rv[0, :2].tolist() == [-2.0, 0.0]
    cv, ci, rv, ri = CR.row_select(val, [set()], [req], [0b01], K, end)
    assert ci.tolist() == [[1, 2, 3]] and ri.tolist() == [[-1, 0, -1, -1]] and rv[0, 0] == NEG
    cv, ci, rv, ri = CR.row_select(val, [set()], [req], [0b11], K, end)
    assert ci.tolist() == [[end, 0, 1]] and ri.tolist() == [[-1] * 4]
    cv, ci, rv, ri = CR.row_select(val, [{0, 1}], [req], [0b00], K, end)         # word 0 excluded by the options
    assert ci.tolist() == [[3, 4, 5]] and ri.tolist() == [[2, -1, -1, -1]]
    cv, ci, rv, ri = CR.row_select(val, [set()], [[]], [0], K, end)              # nothing required: the plain top K
    assert ci.tolist() == [[end, 0, 1]] and ri.tolist() == [[-1] * 4]


def test_merge_state_records_masks_and_closes_images():
    """one image, K = 2, C = 1, both rows have met the word: <end> twice closes the image; the dead slots get zeros"""
    V, K, end = 100, 2, 99
    cv, ci, rv, ri = _rows([([(-1.0, 99), (-2.0, 5)], [None] * 4), ([(-1.5, 99), (-3.0, 6)], [None] * 4)])
    st = {"open_images": torch.tensor([1]), "nsrc": torch.tensor([2]), "kk": torch.tensor([2]), "ncomp": torch.tensor([0]),
          "best_idx": torch.tensor([-1]), "best_score": torch.zeros(1, dtype=torch.float64),
          "scores": torch.tensor([-0.5, -0.7], dtype=torch.float64), "comp_score": torch.zeros(2, dtype=torch.float64),
          "comp_step": torch.full((2,), -1), "comp_parent": torch.zeros(2, dtype=torch.long),
          "token": torch.full((1, 2), -7), "parent": torch.full((1, 2), -7), "met": torch.tensor([1, 1])}
    out = CR.merge_state(st, cv, ci, rv, ri, torch.tensor([[42, -1, -1, -1]]), 1, K, V, end, 0)
    assert out["comp_score"].tolist() == [-1.0, -1.5] and out["comp_parent"].tolist() == [0, 1]
    assert int(out["best_idx"]) == 0 and int(out["open_images"]) == 0 and out["met"].tolist() == [0, 0]
    assert out["token"].tolist() == [[0, 0]] and int(out["kk"]) == 0
    again = CR.merge_state(out, cv, ci, rv, ri, torch.tensor([[42, -1, -1, -1]]), 1, K, V, end, 0)
    assert all(torch.equal(again[k], out[k]) for k in out)


# ---- whole searches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", sorted(CR.TABLES))
def test_invariants_and_caps(table):
    """every completed caption contains all its required words; the mask returned is what the caption implies (the search
    itself asserts met == the history's for the caption it returns); the caps: at most 1/4 of the cases undecidable, at
    least 3 compared cases in which the requirement changes the caption and is satisfied"""
    _, _, rows = CR.TABLES[table]
    end = 1003 - 1
    for idx, (kind, _) in enumerate(rows):
        for (b, k), (res, ok, mask, changed, req) in CR.cases(table, idx).items():
            one, done = res
            seq = CR.seq_of(one, kind)
            assert mask == sum(1 << c for c, w in enumerate(req) if w in seq)
            for words, _ in done:
                if words[-1] == end:
                    assert all(w in words for w in req), (table, idx, b, k)
            if seq[-1] == end:
                assert mask == CR.full_mask(req)
    total, left, changed = CR.table_counts(table)
    print("%s: %d cases, %d left out, the requirement changes %d compared captions" % (table, total, left, changed))
    assert total == 27 and 4 * left <= total and changed >= 3


def test_refusals_of_the_restatement():
    V, T = 1003, 51
    st, en, pad = V - 2, V - 1, 0
    ok = lambda req, K=5, o=OR.Opts(): CR.refusal(req, V, K, T, st, en, pad, o)        # noqa: E731
    assert ok([[1, 2, 3, 4], [], [7]]) is None
    assert ok([[1, 2, 3, 4, 5]]) == "count" and ok([[V]]) == "vocabulary" and ok([[-1]]) == "vocabulary"
    assert ok([[3, 3]]) == "duplicate"
    assert ok([[st]]) == "special" and ok([[en]]) == "special" and ok([[pad]]) == "special"
    assert ok([[5]], o=OR.Opts(banned_tokens=(5,))) == "banned"
    assert ok([[5]], K=0) == "beam_size" and ok([[5]], K=9) == "beam_size"
    o = OR.Opts(no_repeat_ngram=2)
    assert CR.refusal([[5]], 64, 8, T, 62, 63, 0, o) is None and CR.refusal([[5]], 63, 8, T, 61, 62, 0, o) == "candidates"
    assert OR.refusal(o, 63, 8, T, 62) is None              # ... which the options alone would accept


# ---- the Python layer and the C calls that need no device -------------------------------------------------------------------
def test_python_refusals_are_value_errors_before_the_gpu():
    from models.decoders import DecoderEnsemble, SearchOptions, _common
    from test_gpu_parity import _build_decoder
    d, V = BR.sharpened("attention_scn_distinct")
    wm = BR.word_map(V)
    m = _build_decoder("attention_scn", d, torch.device("cpu")).eval()
    enc, tags = t(d["enc"]), t(d["tags"])
    N = enc.shape[0]
    some = [[1, 2]] + [[] for _ in range(N - 1)]
    assert _common.check_required_args(some, N, wm, 3) == some
    assert _common.check_required_args([torch.tensor([1, 2])] + [()] * (N - 1), N, wm, 3) == some
    bad = [[[1, 2, 3, 4, 5]] + [[]] * (N - 1), [[V]] + [[]] * (N - 1), [[-1]] + [[]] * (N - 1), [[3, 3]] + [[]] * (N - 1),
           [[wm["<start>"]]] + [[]] * (N - 1), [[wm["<end>"]]] + [[]] * (N - 1), [[wm["<pad>"]]] + [[]] * (N - 1),
           [[1]] * (N + 1), [[1]] * (N - 1), [1, 2], [[1.5]] + [[]] * (N - 1), "ab"]
    for target in (m, DecoderEnsemble([m])):
        for req in bad:
            with pytest.raises(ValueError):
                target.sample_constrained(3, req, wm, enc, tags)
        for k in (0, 9, 2.5):
            with pytest.raises(ValueError):
                target.sample_constrained(k, some, wm, enc, tags)
        with pytest.raises(ValueError):             # a required word the options ban
            target.sample_constrained(3, some, wm, enc, tags, options=SearchOptions(banned_tokens=(2,)))
        with pytest.raises(ValueError):             # 23 - 13 - 1 - 4 = 5 >= 3, but < 6
            target.sample_constrained(6, some, wm, enc, tags, options=SearchOptions(banned_tokens=tuple(range(3, 16))))
        with pytest.raises(RuntimeError):           # accepted arguments reach the device check
            target.sample_constrained(3, some, wm, enc, tags)
    from scnattn import functional as SF
    with pytest.raises(ValueError, match="do not compose"):
        SF._search_form(None, 2, 0.5, V, 4, 51, V - 1, required=some, N=N, start_token=V - 2, pad_token=0)


def _con(rows, N=None, pad=0):
    from scnattn import _lib as L
    flat = [w for r in rows for w in list(r) + [-1] * (4 - len(r))]
    tab = (C.c_int32 * len(flat))(*flat)
    con = L.Constraints(n_images=len(rows) if N is None else N, pad_token=pad, required=C.addressof(tab))
    con._keep = tab
    return con


def test_c_refusals_and_layout_without_a_device():
    """_workspace_con / _layout_con run on the host: the refusals that need neither <start> nor <end>, and the two offsets
    the layout appends"""
    from scnattn import _lib as L
    h = L.lib()
    V = 80
    dims = L.Dims(3, 9, 32, 16, 16, 16, 8, 4, V, 51, 51, 1)
    n = C.c_size_t()
    good = [[1, 2, 3, 4], [], [7]]

    def ws(rows, K=3, opt=None, **kw):
        return h.scnattn_beam_workspace_con(C.byref(dims), K, 51, C.byref(opt) if opt is not None else None,
                                            C.byref(_con(rows, **kw)), C.byref(n))

    assert ws(good) == 0 and n.value > 0
    with_con = n.value
    assert h.scnattn_beam_workspace(C.byref(dims), 3, 51, C.byref(n)) == 0 and n.value < with_con
    for rows, kw, word in [([[V], [], []], {}, b"outside"), ([[-2], [], []], {}, b"outside"), ([[3, 3], [], []], {}, b"twice"),
                           ([[0], [], []], {}, b"<pad>"), (good, dict(N=2), b"per image"),
                           ([[1], [], []], dict(K=0), b"beam_size"), ([[1], [], []], dict(K=9), b"beam_size")]:
        K = kw.pop("K", 3)
        assert ws(rows, K=K, **kw) == -1 and word in h.scnattn_last_error(), (rows, h.scnattn_last_error())
    hole = _con(good)
    hole._keep[4], hole._keep[5] = -1, 9                # a word behind a -1
    assert h.scnattn_beam_workspace_con(C.byref(dims), 3, 51, None, C.byref(hole), C.byref(n)) == -1
    assert h.scnattn_beam_workspace_con(C.byref(dims), 3, 51, None, None, C.byref(n)) == -1
    o = L.SearchOpts(min_length=0, no_repeat_ngram=0, n_banned=1)
    o.banned[0] = 7
    assert ws(good, opt=o) == -1 and b"banned" in h.scnattn_last_error()
    o.banned[0] = 8
    assert ws(good, opt=o) == 0
    # the candidate-count rule asks for 4 more words: 80 - 0 - 1 - 51 - 4 = 24 >= 8; V = 63 would leave 7
    g = L.SearchOpts(min_length=0, no_repeat_ngram=2, n_banned=0)
    assert ws(good, K=8, opt=g) == 0
    small = L.Dims(3, 9, 32, 16, 16, 16, 8, 4, 63, 51, 51, 1)
    assert h.scnattn_beam_workspace_con(C.byref(small), 8, 51, C.byref(g), C.byref(_con(good)), C.byref(n)) == -1
    assert b"candidates" in h.scnattn_last_error()
    assert h.scnattn_beam_workspace_opt(C.byref(small), 8, 51, C.byref(g), C.byref(n)) == 0
    off = (C.c_long * L.BEAM_NOFF_CON)()
    assert h.scnattn_beam_layout_con(C.byref(dims), 3, 51, None, C.byref(_con(good)), off) == 0
    assert off[13] == -1 and off[14] > off[12] and off[15] > off[14] and len(set(off)) == L.BEAM_NOFF_CON
    assert h.scnattn_beam_layout_con(C.byref(dims), 3, 51, C.byref(o), C.byref(_con(good)), off) == 0 and off[13] > 0
    ens = (L.Dims * 2)(dims, dims)
    assert h.scnattn_ensemble_workspace_con(2, ens, 3, 51, 0, None, C.byref(_con(good)), C.byref(n)) == 0
    assert h.scnattn_ensemble_workspace_con(2, ens, 3, 51, 0, None, C.byref(_con([[3, 3], [], []])), C.byref(n)) == -1


def test_header_declares_every_new_export():
    from scnattn import _lib as L
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    declared = set(re.findall(r"\b(scnattn_[a-z0-9_]+)\s*\(", header))
    h = L.lib()
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(h, name), name
    assert int(re.search(r"#define SCNATTN_BEAM_NOFF_CON (\d+)", header).group(1)) == L.BEAM_NOFF_CON
    assert int(re.search(r"#define SCNATTN_MAX_REQUIRED (\d+)", header).group(1)) == L.MAX_REQUIRED == CR.MAX_REQUIRED
    assert h.scnattn_version() == 109


def test_trace_back_fallback_prefers_the_beams_that_met_more():
    """nothing completed: the open beam with the largest popcount(met), ties to the higher score, then the lower slot; with
    with_met the mask of that beam; without constraints today's fallback"""
    from models.decoders import _common
    K, steps = 3, 2
    res = {"token": torch.tensor([[5, 6, 7], [8, 9, 10]]), "parent": torch.tensor([[0, 0, 0], [0, 1, 2]]), "alpha": None,
           "ncomp": torch.tensor([0]), "best_idx": torch.tensor([-1]), "nsrc": torch.tensor([3]),
           "scores": torch.tensor([-1.0, -2.0, -2.0]), "comp_step": torch.full((3,), -1), "comp_parent": torch.zeros(3),
           "comp_score": torch.zeros(3), "met": torch.tensor([0b01, 0b11, 0b11]), "required": torch.tensor([[6, 9, -1, -1]])}
    one, score, mask = _common.trace_back(res, steps, 1, K, 1, 2, (1, 1), False, with_met=True)[0]
    assert (one, score, mask) == ([1, 6, 9], -2.0, 0b11)
    res["scores"] = torch.tensor([-1.0, -2.5, -2.0])
    assert _common.trace_back(res, steps, 1, K, 1, 2, (1, 1), False, with_scores=True)[0] == ([1, 7, 10], -2.0)
    res["met"] = res["required"] = None
    assert _common.trace_back(res, steps, 1, K, 1, 2, (1, 1), False, with_scores=True)[0] == ([1, 5, 8], -1.0)
