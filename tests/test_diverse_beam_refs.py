"""tests/diverse_beam_refs.py against itself (no GPU): one group is the search with options, a penalty of zero makes every
group a Kg-beam search, the refusals, the merge's rules on hand-made candidates, and the caps of the tables that
tests/test_gpu_diverse_beam_search.py compares -- asserted here from the restatement alone."""
import pytest
import torch

import beam_options_refs as OR
import beam_refs as BR
import diverse_beam_refs as DR
from helpers import params_from


def _inputs(kind, seed):
    d, V, enc, tags = OR.inputs(kind, seed)
    return params_from(d, dtype=torch.float64), BR.word_map(V), enc.double(), tags.double()


@pytest.mark.parametrize("kind,seed,options", [("attention_scn", 2, OR.Opts()), ("pure_scn", 78, DR.NGRAM),
                                               ("attention_scn", 6, OR.Opts(min_length=6, no_repeat_ngram=1))])
@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_one_group_is_the_search_with_options(kind, seed, options, lam):
    """G = 1: c == 0 for every candidate, so any penalty leaves results AND traces those of beam_options_refs.search"""
    P, wm, enc, tags = _inputs(kind, seed)
    for k in (1, 3, 5):
        want, wtr = OR.search_one(kind, P, k, wm, enc, tags, options)
        got, gtr = DR.search_one(kind, P, k, 1, lam, wm, enc, tags, options)
        assert [g[0] for g in got] == want
        assert gtr == wtr


@pytest.mark.parametrize("kind,seed", OR.SEEDS)
@pytest.mark.parametrize("G,kg", [(2, 2), (4, 2), (2, 3)])
def test_zero_penalty_makes_every_group_a_kg_beam_search(kind, seed, G, kg):
    """lambda = 0: a == r, every group starts from the same row and takes the same picks; sequences equal those of the
    search with kg beams, scores within 1e-9 (the GEMMs run over G*kg rows instead of kg)"""
    P, wm, enc, tags = _inputs(kind, seed)
    want, _ = OR.search_one(kind, P, kg, wm, enc, tags)
    got, _ = DR.search_one(kind, P, kg, G, 0.0, wm, enc, tags)
    for b in range(enc.shape[0]):
        for g in range(G):
            (one, done), (w_one, w_done) = got[b][g], want[b]
            assert DR.seq_of(one, kind) == DR.seq_of(w_one, kind), (b, g)
            assert [s for s, _ in done] == [s for s, _ in w_done]
            assert all(abs(x - y) <= 1e-9 for (_, x), (_, y) in zip(done, w_done))


def test_refusals():
    assert DR.refusal(1, 5, 0.0) is None and DR.refusal(4, 8, 1e4) is None and DR.refusal(8, 8, 0.5) is None
    assert DR.refusal(0, 4, 0.5) == "groups" and DR.refusal(-1, 4, 0.5) == "groups"
    assert DR.refusal(3, 8, 0.5) == "multiple" and DR.refusal(2, 5, 0.5) == "multiple"
    assert DR.refusal(1, 0, 0.5) == "beam_size" and DR.refusal(3, 9, 0.5) == "beam_size"
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert DR.refusal(2, 4, bad) == "penalty"
    # the candidate-count rule takes the total K
    o = OR.Opts(no_repeat_ngram=2)
    assert OR.refusal(o, 59, 2, 51, 58) is None and OR.refusal(o, 59, 8, 51, 58) == "candidates"


def test_merge_groups_rules_on_hand_made_candidates():
    """V = 8, <end> = 7, (G, Kg) = (3, 2): ties between a penalised and an unpenalised candidate go by flat index; a word
    picked twice counts twice; <end> picks count; a finished group penalises nobody; raw values are returned"""
    V, Kg, end, lam, v, i = DR.hand_made()
    assert (end, lam) == (7, 0.5)
    got = DR.merge_groups(v, i, V, Kg, 0.5, nsrc=[1, 2, 1], kk=[2, 2, 2])
    assert got[0] == [(-1.0, 0, 3), (-1.5, 0, 7)]
    assert got[1] == [(-0.25, 1, 3), (-1.0, 0, 3)]
    assert got[2] == [(-1.0, 0, 7), (-1.75, 0, 4)]
    # the same with group 1 finished: group 2 then sees word 3 once: a(3) = -1.0, a(<end>) = -1.5, a(4) = -1.75
    got = DR.merge_groups(v, i, V, Kg, 0.5, nsrc=[1, 0, 1], kk=[2, 0, 2])
    assert got[1] is None and got[2] == [(-0.5, 0, 3), (-1.0, 0, 7)]
    # G = 1 is beam_refs.merge
    one = DR.merge_groups(v[:2, :2], i[:2, :2], V, 2, 3.0, nsrc=[2], kk=[2])[0]
    assert one == BR.merge(v[:2, :2], i[:2, :2], V, 2)


def test_selection_value():
    """c = 0 returns r itself in both precisions; fp32 values are fp32 numbers; a representable case by hand"""
    import numpy as np
    assert DR.selection_value(-2.5, 0, 0.3, torch.float32) == -2.5 and DR.selection_value(-2.5, 0, 0.3, torch.float64) == -2.5
    a = DR.selection_value(-1.0, 3, 0.1, torch.float32)
    assert a == float(np.float32(a)) and abs(a + 1.3) < 1e-7
    assert DR.selection_value(-1.0, 2, 0.25, torch.float32) == -1.5 == DR.selection_value(-1.0, 2, 0.25, torch.float64)


@pytest.mark.parametrize("table", sorted(DR.TABLES))
def test_table_caps(table):
    """the conditions under which the GPU comparison says anything: at most 1/4 of a table's cases undecidable, and at
    least 3 decidable cases in which the penalty changes some group's caption"""
    total, left, changed = DR.table_counts(table)
    print("%s: %d cases, %d undecidable, the penalty changes %d compared cases" % (table, total, left, changed))
    assert total == 9 and 4 * left <= total and changed >= 3
    G, kg, options, rows = DR.TABLES[table]
    for idx, (kind, _, _) in enumerate(rows):
        for groups, _, _ in DR.cases(table, idx).values():
            assert len(groups) == G
            caps = [DR.seq_of(one, kind) for one, _ in groups]
            assert all(len(c) - 2 >= options.min_length or c[-1] != 1002 for c in caps)
            if options.no_repeat_ngram == 2:
                for c in caps:
                    grams = [tuple(c[q:q + 2]) for q in range(1, len(c) - 1)]
                    assert len(grams) == len(set(grams)) and OR.UNK not in c
