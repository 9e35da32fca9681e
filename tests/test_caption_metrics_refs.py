"""CPU tests of tests/caption_metrics_refs.py and of the host side of the caption metrics.

1. The fp64 restatement on tie-free rows (every row a permutation of distinct values, so no order rule is in play): the loss
   equals oracle.scnattn_ref.caption_loss, hits[0] * (100 / N) equals oracle.scnattn_ref.topk_accuracy and
   utils.metric.accuracy on the packed batch, hits[1] the top-1 count, preds equals torch.max(scores, 2)[1].
   Tied rows are judged against the stated rule alone (2.), never against topk, whose choice among equal values is not an
   index rule.
2. The rule on rows written out by hand, and what every adversarial row of the GPU test is meant to contain.
3. Host logic: CPU tensors raise RuntimeError (no fallback) from caption_loss_metrics, TrainStep(metrics=True) and
   validate(fused=True); the symbol is in the ctypes table and in the header; the library's version stays 109."""
import os

import pytest
import torch

import caption_metrics_refs as R

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("Bn,Tn,V,lengths", [(6, 5, 40, [5, 5, 4, 3, 3, 1]), (4, 7, 37, [7, 6, 2, 1]), (5, 4, 257, [4, 4, 4, 4, 4])])
def test_restatement_on_tie_free_rows(Bn, Tn, V, lengths):
    from oracle import scnattn_ref as O
    from utils.metric import accuracy
    scores, targets = R.gen_tie_free(Bn, Tn, V, seed=V)
    caps = torch.cat([torch.zeros(Bn, 1, dtype=torch.long), targets, torch.zeros(Bn, 1, dtype=torch.long)], dim=1)
    want_loss, sp, tp = O.caption_loss(scores.to(F64), caps, lengths, None)
    n = sum(lengths)
    for k in (1, 5, V + 1):
        ref = R.metrics_ref(scores, targets, lengths, k)
        assert ref["n_tokens"] == n
        assert abs(float(ref["total"]) - float(want_loss)) <= 1e-12 * abs(float(want_loss))
        kk = min(k, V)                                      # topk cannot ask for more than V
        assert float(ref["hits"][0]) * (100.0 / n) == O.topk_accuracy(sp, tp, kk) == accuracy(sp.float(), tp, kk)
        assert int(ref["hits"][1]) == int((sp.argmax(dim=1) == tp).sum())
        want = torch.max(scores, 2)[1]
        for b in range(Bn):
            assert torch.equal(ref["preds"][b, :lengths[b]], want[b, :lengths[b]])
            assert int(ref["preds"][b, lengths[b]:].abs().sum()) == 0
            assert bool((ref["rank"].view(Bn, Tn)[b, lengths[b]:] == -1).all())


def test_the_rule_on_rows_written_out():
    x = torch.tensor([1.0, 3.0, 2.0, 3.0, 2.0, float("-inf")])
    assert R.row_ref(x, 1)[2:] == (0, 1)          # the first of the two maxima: rank 0, and the arg-max
    assert R.row_ref(x, 3)[2:] == (1, 1)          # the second maximum comes after the first
    assert R.row_ref(x, 2)[2:] == (2, 1)          # two above
    assert R.row_ref(x, 4)[2:] == (3, 1)          # two above, one equal at a lower index
    assert R.row_ref(x, 0)[2:] == (4, 1)
    assert R.row_ref(x, 5)[2:] == (5, 1)
    lse, loss, rank, pred = R.row_ref(x, 6)
    assert loss != loss and rank == R.INT_MAX and pred == 1
    assert R.row_ref(x, -1)[2] == R.INT_MAX
    e = R.row_ref(torch.full((7,), 0.25), 3)
    assert e[2:] == (3, 0) and abs(e[1] - torch.log(torch.tensor(7.0, dtype=F64)).item()) < 1e-15
    ref = R.metrics_ref(x.view(1, 1, 6).expand(2, 3, 6), torch.tensor([[1, 3, 2], [4, 6, 0]]), [3, 2], 2)
    assert ref["rank"].tolist() == [0, 1, 2, 3, R.INT_MAX, -1] and ref["hits"].tolist() == [2, 1]
    assert ref["preds"].tolist() == [[1, 1, 1], [1, 1, 0]] and ref["n_tokens"] == 5
    assert ref["total"] != ref["total"] and ref["lse"][5] == 0 and ref["loss"][5] == 0


@pytest.mark.parametrize("V", R.VOCABS)
def test_adversarial_rows_contain_what_they_claim(V):
    for k in R.ks_of(V):
        seen = {}
        for variant in R.VARIANTS:
            scores, targets, lengths, names = R.gen_case(V, k, variant)
            ref = R.metrics_ref(scores, targets, lengths, k)
            rows = [(b, t) for b in range(R.B) for t in range(min(lengths[b], R.T))]
            assert len(rows) == len(names) == ref["n_tokens"]
            for (b, t), name in zip(rows, names):
                seen.setdefault(name, []).append((scores[b, t], int(targets[b, t]), int(ref["rank"][b * R.T + t]),
                                                  int(ref["preds"][b, t])))
        assert set(seen) == set(R.KINDS)
        for x, tg, rank, pred in seen["hit"]:
            assert rank == min(k - 1, V - 1) and rank < k
        for x, tg, rank, pred in seen["miss"]:
            assert rank == min(k, V - 1) and (rank >= k or V <= k)
        for x, tg, rank, pred in seen["tied_target"]:
            ties = (x == x[tg]).nonzero().reshape(-1)
            assert rank == int((x > x[tg]).sum()) + int((ties < tg).sum())
            if V >= 255:
                assert int((ties < tg).sum()) >= 3 and int((ties > tg).sum()) >= 3 and int((x > x[tg]).sum()) == 2
        for x, tg, rank, pred in seen["tied_max"]:
            top = (x == x.max()).nonzero().reshape(-1)
            assert pred == int(top[0]) and tg == int(top[-1]) and rank == top.numel() - 1
            if V >= 1030:
                assert top.numel() >= 6
        for x, tg, rank, pred in seen["all_equal"]:
            assert pred == 0 and rank == tg == V // 2
        for x, tg, rank, pred in seen["neg_inf"]:
            assert x[tg] > R.NINF and (V < 3 or (x[0] == R.NINF and int((x == R.NINF).sum()) >= min(8, V - 1)))
        assert all(tg == 0 for _, tg, _, _ in seen["first"]) and all(tg == V - 1 for _, tg, _, _ in seen["last"])
        assert all(tg == pred and rank == 0 for _, tg, rank, pred in seen["argmax"])
        assert all(tg == -1 and rank == R.INT_MAX for _, tg, rank, _ in seen["below"])
        assert all(tg == V and rank == R.INT_MAX for _, tg, rank, _ in seen["above"])


def test_planted_spots_cover_lanes_waves_and_sweeps():
    """of both forms: vector (thread = v % 1024 // 4) and scalar (thread = v % 256)"""
    for n in (5, 21):
        _planted_spots(n)


def _planted_spots(n):
    x, tg = R.row_above(2052, n, torch.Generator().manual_seed(0), n)
    above = (x > x[tg]).nonzero().reshape(-1)
    assert above.numel() == n
    if n == 5:
        assert len({int(v) % 4 for v in above}) >= 3 and len({int(v) % 1024 // 4 // 64 for v in above}) >= 3
        assert {int(v) // 1024 for v in above} == {0, 1, 2} and len({int(v) % 256 // 64 for v in above}) >= 3
        return
    assert {int(v) % 4 for v in above} == {0, 1, 2, 3}
    assert {int(v) % 1024 // 4 // 64 for v in above} == {0, 1, 2, 3} and {int(v) // 1024 for v in above} == {0, 1, 2}
    assert {int(v) % 256 // 64 for v in above} == {0, 1, 2, 3} and len({int(v) // 256 for v in above}) >= 5


# ---- 3. host logic --------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    from scnattn import functional as SF
    scores, targets = R.gen_tie_free(2, 3, 8, seed=1)
    caps = torch.cat([torch.zeros(2, 1, dtype=torch.long), targets, torch.zeros(2, 1, dtype=torch.long)], dim=1)
    with pytest.raises(RuntimeError):
        SF.caption_loss_metrics(scores, caps, [3, 2])
    with pytest.raises(RuntimeError):
        SF.caption_loss_metrics(scores, caps, [3, 2], k=0)


class _Decoder:
    """what validate() needs of a decoder: the five-tuple, from CPU tensors"""

    def eval(self):
        return self

    def __call__(self, encoder_out, tags, caps, caplens):
        scores, _ = R.gen_tie_free(2, 3, 8, seed=2)
        return scores, caps, [3, 2], torch.rand(2, 3, 4), torch.tensor([0, 1])


def test_validate_fused_on_cpu_tensors_raises():
    from trains.harness import validate
    wm = {"<pad>": 0, "<start>": 6, "<end>": 7}
    caps = torch.randint(1, 6, (2, 5))
    batch = (None, caps, torch.tensor([[4], [3]]), torch.stack([caps, caps], dim=1))
    enc = type("E", (), {"eval": lambda s: None, "__call__": lambda s, x: torch.rand(2, 2, 2, 4)})()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validate([batch], enc, lambda x: torch.rand(2, 3), _Decoder(), torch.nn.CrossEntropyLoss(), wm, fused=True)
    bleu, loss, top5 = validate([batch], enc, lambda x: torch.rand(2, 3), _Decoder(), torch.nn.CrossEntropyLoss(), wm)
    assert loss > 0 and 0.0 <= top5 <= 100.0          # the default is the eager path, which runs anywhere


def test_train_step_flag():
    import inspect
    from trains.harness import TrainStep, topk_percent, validate
    assert inspect.signature(TrainStep.__init__).parameters["metrics"].default is False
    assert inspect.signature(validate).parameters["fused"].default is False
    with pytest.raises(ValueError):
        TrainStep(device="cpu", encoder=False, metrics=True, fused_loss=False, vocab_size=12, emb_dim=8, attention_dim=8,
                  decoder_dim=8, factored_dim=8, semantic_dim=4)
    assert topk_percent(torch.tensor([3, 1], dtype=torch.int32), 7) == 3.0 * (100.0 / 7)


def test_symbol_is_declared_and_the_version_stays():
    from scnattn import _lib
    assert "scnattn_caption_loss_metrics_fwd" in _lib.EXPORTS
    fwd, met = _lib._SIGS["scnattn_caption_loss_fwd"], _lib._SIGS["scnattn_caption_loss_metrics_fwd"]
    assert met[0][:len(fwd[0])] == fwd[0] and len(met[0]) == len(fwd[0]) + 5
    with open(os.path.join(ROOT, "include", "scnattn.h")) as f:
        header = f.read()
    assert "int scnattn_caption_loss_metrics_fwd(" in header and "#define SCNATTN_VERSION 109 " in header
