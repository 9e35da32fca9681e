"""GPU tests (``-m gpu``) of the caption metrics above the kernel: scnattn.functional.caption_loss_metrics inside
TrainStep(metrics=True) and validate(fused=True), small widths, no encoder, V = 40, B = 6.

1. Two steps of TrainStep with metrics=True and with metrics=False from the same seed: the same loss bits and bit-equal
   flat parameter buffers (the metrics ride in the pass, they do not touch it); `last_metrics` / topk_percent() equal the
   eager utils.metric.accuracy on the step's own scores, which are checked to be tie-free.
2. validate(fused=True) over two ragged batches, for each of the three decoders, against the reference's bookkeeping
   (trains/attention_scn.py:320-378) done here with torch ops on the same decoder outputs: BLEU-4 and top-5 exactly equal,
   the loss within the 1e-4 relative of tests/test_gpu_parity.py::test_validate_path; for AttentionSCN also against
   validate() itself.
3. caption_loss_metrics: the loss has caption_loss's bits and gradient; hits and preds carry no gradient; preds holds 0
   behind every row's decoded part and nothing but (B, T) entries."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence

pytestmark = pytest.mark.gpu

V, B = 40, 6
WM = {"<pad>": 0, "<unk>": V - 3, "<start>": V - 2, "<end>": V - 1}
SMALL = dict(vocab_size=V, batch_size=B, emb_dim=20, attention_dim=24, decoder_dim=28, factored_dim=36, semantic_dim=14,
             max_len=7)
KINDS = ("attention_scn", "pure_scn", "pure_attention")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _tie_free(scores, decode_lengths):
    for b, n in enumerate(decode_lengths):
        for t in range(n):
            assert scores[b, t].unique().numel() == scores.shape[2], "row (%d, %d) has equal logits" % (b, t)


def _packed(scores, caps_sorted, decode_lengths):
    return (pack_padded_sequence(scores, decode_lengths, batch_first=True).data,
            pack_padded_sequence(caps_sorted[:, 1:], decode_lengths, batch_first=True).data)


def _forward(ts, enc, tags, caps, caplens):
    if ts.kind == "pure_attention":
        scores, caps_sorted, dl, _, _ = ts.decoder(enc, caps, caplens)
    else:
        scores, caps_sorted, dl = ts.decoder(enc, tags, caps, caplens)[:3]
    return scores, caps_sorted, dl


@pytest.mark.parametrize("kind", KINDS)
def test_train_step_with_metrics_trains_identically(dev, kind):
    from trains.harness import TrainStep, synthetic_batch
    from utils.metric import accuracy
    ends = []
    for metrics in (True, False):
        ts = TrainStep(kind=kind, fine_tune_encoder=False, device=dev, encoder=False, dropout=0.0, seed=4, metrics=metrics,
                       **SMALL)
        assert ts.last_metrics is None
        losses = []
        for step in range(2):
            _, tags, caps, caplens = synthetic_batch(B, V, SMALL["max_len"], 8, SMALL["semantic_dim"], dev, 6 + step, ragged=True)
            enc = torch.rand(B, 3, 3, 2048, generator=torch.Generator().manual_seed(8 + step)).to(dev)
            with torch.no_grad():                                   # the scores this step will see (dropout is off)
                scores, caps_sorted, dl = _forward(ts, enc, tags, caps, caplens)
            loss = ts.step(None, tags, caps, caplens, enc)
            losses.append(loss.detach().clone())
            if metrics:
                _tie_free(scores.cpu(), dl)
                sp, tp = _packed(scores, caps_sorted, dl)
                lm_loss, hits, n = ts.last_metrics
                assert hits.is_cuda and hits.dtype == torch.int32 and tuple(hits.shape) == (2,) and n == sum(dl)
                assert torch.equal(lm_loss, loss.detach())
                assert ts.topk_percent() == accuracy(sp, tp, 5)
                assert int(hits[1]) == int((sp.argmax(dim=1) == tp).sum())
        if not metrics:
            assert ts.last_metrics is None
            with pytest.raises(RuntimeError):
                ts.topk_percent()
        ts.decoder_optimizer.flat.gather()
        ends.append((losses, ts.decoder_optimizer.flat.flat_p.clone()))
        del ts
    for a, b in zip(ends[0][0], ends[1][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the loss differs with metrics on"
    assert torch.equal(ends[0][1].view(torch.int32), ends[1][1].view(torch.int32)), "the parameters differ with metrics on"


def _decoder(kind):
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_attention import PureAttention
    from models.decoders.pure_scn import PureSCN
    torch.manual_seed(3)
    if kind == "attention_scn":
        return AttentionSCN(24, 20, 28, 36, 14, V, encoder_dim=40, dropout=0.5)
    if kind == "pure_scn":
        return PureSCN(20, 28, 36, 14, V, encoder_dim=40, dropout=0.5)
    return PureAttention(24, 20, 28, V, encoder_dim=40, dropout=0.5)


def _batches(dev):
    g = torch.Generator().manual_seed(5)
    out = []
    for lens, L in (([9, 7, 8, 5, 6, 4], 9), ([3, 11, 6, 6, 2, 8], 11)):
        caps = torch.zeros(B, L, dtype=torch.long)
        for b, n in enumerate(lens):
            caps[b, 0] = V - 2
            caps[b, 1:n - 1] = torch.randint(1, V - 3, (n - 2,), generator=g)
            caps[b, n - 1] = V - 1
        allcaps = torch.stack([caps, caps.roll(1, 0)], dim=1)           # 2 references per image
        imgs = (torch.rand(B, 3, 3, 40, generator=g).to(dev), torch.rand(B, 14, generator=g).to(dev))
        out.append((imgs, caps.to(dev), torch.tensor(lens).unsqueeze(1).to(dev), allcaps.to(dev)))
    return out


class _Encoder:
    """the batch carries (encoder_out, tags) in place of the images"""

    def eval(self):
        return self

    def __call__(self, imgs):
        return imgs[0]


@pytest.mark.parametrize("kind", KINDS)
def test_validate_fused_equals_the_reference_bookkeeping(dev, kind):
    from trains.harness import validate
    from utils.metric import AverageMeter, accuracy, corpus_bleu
    dec = _decoder(kind).to(dev)
    batches = _batches(dev)
    seen = []
    hook = dec.register_forward_hook(lambda m, i, o: seen.append(o))
    crit = torch.nn.CrossEntropyLoss()
    bleu, loss, top5 = validate(batches, _Encoder(), lambda imgs: imgs[1], dec, crit, WM, alpha_c=0.7, fused=True)
    hook.remove()
    assert not dec.training and len(seen) == len(batches)
    losses, top5accs, refs, hyps = AverageMeter(), AverageMeter(), [], []
    skip = {WM["<start>"], WM["<pad>"]}
    for (_, _, _, allcaps), out in zip(batches, seen):
        scores, caps_sorted, dl = out[:3]
        alphas, sort_ind = (out[3] if len(out) == 5 else None), out[-1]
        _tie_free(scores.cpu(), dl)
        scores_copy = scores.clone()
        sp, tp = _packed(scores, caps_sorted, dl)
        batch_loss = crit(sp, tp)
        if alphas is not None:
            batch_loss = batch_loss + 0.7 * ((1. - alphas.sum(dim=1)) ** 2).mean()
        losses.update(batch_loss.item(), sum(dl))
        top5accs.update(accuracy(sp, tp, 5), sum(dl))
        ac = allcaps[sort_ind]
        for j in range(ac.shape[0]):
            refs.append([[w for w in c if w not in skip] for c in ac[j].tolist()])
        preds = torch.max(scores_copy, dim=2)[1].tolist()
        hyps.extend(p[:dl[j]] for j, p in enumerate(preds))
    assert bleu == corpus_bleu(refs, hyps)
    assert top5 == top5accs.avg
    assert abs(loss - losses.avg) < 1e-4 * abs(losses.avg)
    if kind == "attention_scn":
        eager = validate(batches, _Encoder(), lambda imgs: imgs[1], dec, crit, WM, alpha_c=0.7)
        assert eager[0] == bleu and eager[2] == top5 and abs(eager[1] - loss) < 1e-4 * abs(loss)


@pytest.mark.parametrize("with_alpha", (True, False))
def test_functional_loss_bits_gradient_and_outputs(dev, with_alpha):
    from scnattn import functional as SF
    import caption_metrics_refs as R
    Tn, P, lens = 5, 9, [7, 5, 4, 3, 3, 1]                       # one length greater than T
    scores, targets = R.gen_tie_free(B, Tn, V, seed=11)
    caps = torch.cat([torch.zeros(B, 1, dtype=torch.long), targets, torch.zeros(B, 2, dtype=torch.long)], dim=1).to(dev)
    g = torch.Generator().manual_seed(12)
    alphas = torch.softmax(torch.randn(B, Tn, P, generator=g), dim=2).to(dev) if with_alpha else None
    ref = R.metrics_ref(scores, targets, lens, 5)
    grads = []
    for metrics in (True, False):
        sd = scores.to(dev).requires_grad_(True)
        ad = alphas.clone().requires_grad_(True) if with_alpha else None
        if metrics:
            loss, hits, preds = SF.caption_loss_metrics(sd, caps, lens, ad, alpha_c=0.7)
            assert not hits.requires_grad and not preds.requires_grad
            assert hits.dtype == preds.dtype == torch.int32 and tuple(hits.shape) == (2,) and tuple(preds.shape) == (B, Tn)
            assert torch.equal(hits.cpu().long(), ref["hits"]) and torch.equal(preds.cpu().long(), ref["preds"])
            for b, n in enumerate(lens):
                assert int(preds[b, n:].abs().sum()) == 0           # nothing behind the decoded part of a row
            hits1 = SF.caption_loss_metrics(sd.detach(), caps, lens, None, k=1)[1]
            assert int(hits1[0]) == int(hits1[1]) == int(ref["hits"][1])
            every = SF.caption_loss_metrics(sd.detach(), caps, lens, None, k=V + 1)[1]
            assert int(every[0]) == ref["n_tokens"]
        else:
            loss = SF.caption_loss(sd, caps, lens, ad, alpha_c=0.7)
        (2.5 * loss).backward()
        grads.append((loss.detach().clone(), sd.grad.clone(), ad.grad.clone() if with_alpha else None))
    assert torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32))
    assert torch.equal(grads[0][1].view(torch.int32), grads[1][1].view(torch.int32))
    if with_alpha:
        assert torch.equal(grads[0][2].view(torch.int32), grads[1][2].view(torch.int32))
    with pytest.raises(RuntimeError):
        SF.caption_loss_metrics(scores.to(dev), caps, lens, k=0)
