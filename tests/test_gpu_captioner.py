"""GPU tests of scnattn.inference.Captioner: decoded images of different sizes in, caption records out, against the
composition written out by hand -- the numpy restatement of Pillow's resize (tests/resize_refs.py), the reference's
`/ 255.` + Normalize (oracle/data_ref.py), the same modules, `sample_batch`.  The decoders have the small dimensions
of tests/test_beam_host.py; encoder and tagger are tiny stand-ins (the real trunk behind the same tensor is covered by
the eval-trunk tests)."""
import numpy as np
import pytest
import torch
from torch import nn

import beam_refs as BR
import resize_refs as RR
from oracle import data_ref as DR

pytestmark = pytest.mark.gpu

V, SIZE = 12, (16, 16)
KINDS = ("attention_scn", "pure_scn", "pure_attention")


class TinyEncoder(nn.Module):
    """[N, 3, 16, 16] -> (N, 2, 2, 8)"""
    input_size = SIZE

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, kernel_size=8, stride=8)

    def forward(self, x):
        return torch.tanh(self.conv(x)).permute(0, 2, 3, 1)


class TinyTagger(nn.Module):
    """[N, 3, 16, 16] -> (N, 3)"""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(3, 3)

    def forward(self, x):
        return torch.sigmoid(self.fc(x.mean(dim=(2, 3))))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _decoder(kind):
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_scn import PureSCN
    from models.decoders.pure_attention import PureAttention
    if kind == "attention_scn":
        return AttentionSCN(5, 4, 6, 7, 3, V, encoder_dim=8)
    if kind == "pure_scn":
        return PureSCN(4, 6, 7, 3, V, encoder_dim=8)
    return PureAttention(5, 4, 6, V, encoder_dim=8)


def _images():
    return [RR.random_image((33, 47), 21), RR.random_image((5, 9), 22, grey=True), RR.checker_image((16, 16)),
            RR.random_image((7, 5), 23)]


def _modules(kind, dev):
    torch.manual_seed(KINDS.index(kind))
    return TinyEncoder().to(dev), TinyTagger().to(dev), _decoder(kind).to(dev)


def _by_hand(kind, enc, tag, dec, wm, images, beam, dtype, dev, image_dtype=torch.float32):
    batch = torch.stack([DR.image_item(RR.rows(im, SIZE)) for im in images]).to(image_dtype).to(dev)
    enc.eval(), tag.eval(), dec.eval()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            encoder_out, tags = enc(batch), tag(batch)
        encoder_out, tags = encoder_out.float(), tags.float()
        if kind == "pure_attention":
            return dec.sample_batch(beam, wm, encoder_out), tags
        return dec.sample_batch(beam, wm, encoder_out, tags), tags


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", KINDS)
def test_captioner_equals_the_composition_by_hand(dev, kind, dtype):
    from scnattn.inference import Captioner
    wm = BR.word_map(V)
    rev = {v: k for k, v in wm.items()}
    enc, tag, dec = _modules(kind, dev)
    images = _images()
    cap = Captioner(enc, dec, wm, tagger=tag, beam_size=3, dtype=dtype)
    assert cap.size == SIZE
    records = cap(images, tag_count=2)
    want, tags = _by_hand(kind, enc, tag, dec, wm, images, 3, dtype, dev)
    tags = tags.cpu().numpy()
    assert len(records) == len(images) == len(want)
    special = {wm["<start>"], wm["<end>"], wm["<pad>"]}
    for i, (rec, res) in enumerate(zip(records, want)):
        seq, alphas = (res, None) if kind == "pure_scn" else res
        assert rec["tokens"] == seq and seq[0] == wm["<start>"]
        if alphas is None:
            assert rec["alphas"] is None
        else:
            assert torch.equal(torch.as_tensor(rec["alphas"]), torch.as_tensor(alphas))
        assert rec["words"] == [rev[w] for w in seq if w not in special]
        assert all(w not in ("<start>", "<end>", "<pad>") for w in rec["words"])
        t = np.asarray(tags[i].flatten().tolist())
        idx = np.argsort(t)[-2:]
        assert np.array_equal(rec["tags"][0], idx) and np.array_equal(rec["tags"][1], t[idx])


def test_captioner_size_argument_tags_off_and_missing_tagger(dev):
    from scnattn.inference import Captioner
    wm = BR.word_map(V)
    enc, tag, dec = _modules("pure_attention", dev)
    enc.input_size = (256, 256)                           # the argument wins over the module's attribute
    cap = Captioner(enc, dec, wm, beam_size=2, size=SIZE)
    records = cap(_images()[:3])
    want, _ = _by_hand("pure_attention", enc, tag, dec, wm, _images()[:3], 2, torch.float32, dev)
    assert [r["tokens"] for r in records] == [w[0] for w in want] and all(r["tags"] is None for r in records)
    cap16 = Captioner(enc, dec, wm, beam_size=2, size=SIZE, dtype=torch.bfloat16, image_dtype=torch.bfloat16)
    assert cap16.images_to_batch(_images()[:3]).dtype == torch.bfloat16
    want16, _ = _by_hand("pure_attention", enc, tag, dec, wm, _images()[:3], 2, torch.bfloat16, dev, torch.bfloat16)
    assert [r["tokens"] for r in cap16(_images()[:3])] == [w[0] for w in want16]
    with pytest.raises(ValueError, match="tagger"):
        Captioner(enc, _decoder("pure_scn").to(dev), wm)
    with pytest.raises(ValueError, match="word_map"):
        Captioner(enc, dec, {"<start>": 0})
