"""GPU tests (``-m gpu``) of scnattn_caption_loss_metrics_fwd (csrc/loss.hip) through the C ABI, judged against the fp64
restatement of tests/caption_metrics_refs.py.

Buffers are guarded windows (tests/kernel_harness.py GBuf): NaN around the scores, the sentinel around and inside every
output (viewed as int32 for row_rank, preds and hits), which must survive; the targets and preds have leading dimensions
wider than their rows.  The scores' base sits on the 16-byte grid (the vector form when V % 4 == 0) and one float off it (the
scalar form).  Every case runs twice and must give the same bits.

row_rank, preds and hits must EQUAL the restatement, every row of every case: they are comparisons of the given fp32 numbers.
row_lse, row_loss and loss must hold the bits scnattn_caption_loss_fwd writes for the same buffers, and lie within 1e-5
relative of fp64 (the bound of tests/test_gpu_parity.py::test_fused_caption_loss_matches_oracle).  Every refusal returns -1 and
leaves the outputs as the sentinel.

The worst err / bound per result goes to the run's parity report; profiles/parity_report_caption_metrics.txt keeps a copy."""
import ctypes as C
import functools

import pytest
import torch

import caption_metrics_refs as R
from kernel_harness import GBuf, SENT, _bound_ok, _call, _note, _write_report      # noqa: F401  (_write_report: the report fixture)

pytestmark = pytest.mark.gpu

F64 = torch.float64
B, T = R.B, R.T
LDT, LDP, P = T + 3, T + 3, 5
ALPHA_C = 0.7
REPORT_TITLE = ("caption loss with metrics vs fp64: row_rank / preds / hits equal to the restatement in every case (err/bound 0); "
                "row_lse, row_loss 1e-5 x the case's largest |ref|, loss 1e-5 |ref|; all three bit-equal to scnattn_caption_loss_fwd")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(V, k, variant):
    scores, targets, lengths, names = R.gen_case(V, k, variant)
    g = torch.Generator().manual_seed(V + 17)
    alphas = torch.softmax(torch.randn(B, T, P, generator=g), dim=2) if variant == "ranks" else None
    return scores, targets, lengths, names, alphas, R.metrics_ref(scores, targets, lengths, k)


class _Outs:
    def __init__(self, dev, metrics):
        self.lse, self.rows, self.loss = (GBuf(dev, (B * T,), out=True), GBuf(dev, (B * T,), out=True), GBuf(dev, (1,), out=True))
        self.sm1, self.reg = GBuf(dev, (B * P,), out=True), GBuf(dev, (B,), out=True)
        self.rank = self.preds = self.hits = None
        if metrics:
            self.rank, self.hits = GBuf(dev, (B * T,), out=True), GBuf(dev, (2,), out=True)
            self.preds = GBuf(dev, (B, T), (LDP, 1), out=True)

    def read(self):
        out = dict(lse=self.lse.read("row_lse"), rows=self.rows.read("row_loss"), loss=self.loss.read("loss"))
        if self.rank is not None:
            out.update(rank=self.rank.read("row_rank").view(torch.int32), preds=self.preds.read("preds").view(torch.int32),
                       hits=self.hits.read("hits").view(torch.int32))
        return out


def _inputs(dev, scores, targets, lengths, alphas, mis):
    sb = GBuf(dev, scores.shape, vals=scores, mis=mis)
    tgt = torch.full((B, LDT), -7, dtype=torch.int64)          # a label nobody may read sits behind every row
    tgt[:, :T] = targets
    ab = None if alphas is None else GBuf(dev, alphas.shape, vals=alphas)
    return sb, tgt.to(dev), torch.tensor(lengths, dtype=torch.int32, device=dev), ab


def _launch(dev, ins, lengths, V, k, metrics, with_reg):
    sb, tgt, dl, ab = ins
    o = _Outs(dev, metrics)
    n = sum(min(l, T) for l in lengths)
    args = [B, T, V, P if ab is not None else 0, sb.ptr, C.c_void_p(tgt.data_ptr()), LDT, C.c_void_p(dl.data_ptr()), n,
            None if ab is None else ab.ptr, ALPHA_C, o.lse.ptr, o.rows.ptr, o.sm1.ptr if with_reg else None,
            o.reg.ptr if with_reg else None, o.loss.ptr]
    if metrics:
        _call("scnattn_caption_loss_metrics_fwd", dev, *args, k, o.rank.ptr, o.preds.ptr, LDP, o.hits.ptr)
    else:
        _call("scnattn_caption_loss_fwd", dev, *args)
    if not with_reg:
        assert bool((o.sm1.flat.view(torch.int32) == SENT).all()) and bool((o.reg.flat.view(torch.int32) == SENT).all())
    return o.read()


def _bits(x):
    return x.contiguous().view(torch.int32)


def _judge(what, got, plain, ref, alphas, names):
    assert torch.equal(got["rank"].long(), ref["rank"]), "%s: row_rank %s, the rule gives %s (rows: %s)" % (
        what, got["rank"].tolist(), ref["rank"].tolist(), names)
    assert torch.equal(got["preds"].long(), ref["preds"]), "%s: preds %s, the rule gives %s (rows: %s)" % (
        what, got["preds"].tolist(), ref["preds"].tolist(), names)
    assert torch.equal(got["hits"].long(), ref["hits"]), "%s: hits %s, the rule gives %s" % (
        what, got["hits"].tolist(), ref["hits"].tolist())
    for name in ("rank", "preds", "hits"):
        _note(what, name, 0.0, "=equal to the restatement, every element")
    for name in ("lse", "rows", "loss"):
        assert torch.equal(_bits(got[name]), _bits(plain[name])), "%s: %s differs from scnattn_caption_loss_fwd's" % (what, name)
    bad = ref["loss"].isnan()
    assert torch.equal(got["rows"].isnan(), bad), "%s: NaN rows %s" % (what, got["rows"].isnan().tolist())
    _bound_ok(what, "row_lse", got["lse"], ref["lse"], R.TOL * ref["lse"].abs().max().reshape(1), "=1e-5 x largest |ref|")
    keep = ~bad
    _bound_ok(what, "row_loss", got["rows"][keep], ref["loss"][keep],
              R.TOL * ref["loss"][keep].abs().max().reshape(1), "=1e-5 x largest |ref|")
    total = ref["total"]
    if alphas is not None:
        total = total + ALPHA_C * ((1.0 - alphas.to(F64).sum(dim=1)) ** 2).mean()
    if bool(bad.any()):
        assert bool(got["loss"].isnan().all()), "%s: a bad label must poison the loss" % what
    else:
        _bound_ok(what, "loss", got["loss"], total.reshape(1), R.TOL * total.abs().reshape(1), "=1e-5 |ref|")


@pytest.mark.parametrize("V", R.VOCABS)
def test_caption_loss_metrics_fwd(dev, V):
    for k in R.ks_of(V):
        for variant in R.VARIANTS:
            scores, targets, lengths, names, alphas, ref = _case(V, k, variant)
            for mis in (0, 1):
                ins = _inputs(dev, scores, targets, lengths, alphas, mis)
                a = _launch(dev, ins, lengths, V, k, True, alphas is not None)
                b = _launch(dev, ins, lengths, V, k, True, alphas is not None)
                for name in a:
                    assert torch.equal(_bits(a[name]), _bits(b[name])), "%s: two runs differ" % name
                plain = _launch(dev, ins, lengths, V, k, False, alphas is not None)
                form = "vector" if (V % 4 == 0 and not mis) else "scalar"
                _judge("caption_loss_metrics_fwd %s" % form, a, plain, ref, alphas, names)


def test_refusals_leave_the_outputs_untouched(dev):
    from scnattn import _lib as L
    h = L.lib()
    V, k = 8, 5
    scores, targets, lengths, _, _, _ = _case(4, 5, "ends")
    scores = torch.cat([scores, scores], dim=2)
    sb, tgt, dl, _ = _inputs(dev, scores, targets, lengths, None, 0)
    ab = GBuf(dev, (B, T, P), vals=torch.rand(B, T, P))
    o = _Outs(dev, True)
    tp, dp = C.c_void_p(tgt.data_ptr()), C.c_void_p(dl.data_ptr())
    n = sum(lengths)

    def call(B_=B, k_=k, ldp=LDP, rank=o.rank.ptr, preds=o.preds.ptr, hits=o.hits.ptr, scores_=sb.ptr, ldt=LDT, n_=n,
             alphas=None, sm1=None, lse=o.lse.ptr, loss=o.loss.ptr):
        return h.scnattn_caption_loss_metrics_fwd(None, B_, T, V, P if alphas is not None else 0, scores_, tp, ldt, dp, n_, alphas,
                                                  ALPHA_C, lse, o.rows.ptr, sm1, None, loss, k_, rank, preds, ldp, hits)

    refused = [call(k_=0), call(k_=-3), call(ldp=T - 1), call(rank=None), call(preds=None), call(hits=None),
               call(scores_=None), call(ldt=T - 1), call(B_=0), call(n_=0), call(lse=None), call(loss=None),
               call(alphas=ab.ptr, sm1=o.sm1.ptr)]                  # alphas without the reg_part workspace
    torch.cuda.synchronize()
    assert refused == [-1] * len(refused), refused
    assert b"invalid argument" in h.scnattn_last_error()
    for name in ("lse", "rows", "loss", "sm1", "reg", "rank", "preds", "hits"):
        assert bool((getattr(o, name).flat.view(torch.int32) == SENT).all()), name
    assert call() == 0 and call(k_=V + 1, ldp=T) == 0               # what is legal still runs: k > V, ldp = T
    torch.cuda.synchronize()
