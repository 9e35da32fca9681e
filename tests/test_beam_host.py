"""CPU-only tests of the batched beam search's host side: the three decoders have sample_batch, it refuses CPU tensors
instead of falling back, rejects beam sizes the kernels do not cover, the workspace query validates its arguments without
touching a GPU, and include/scnattn.h declares every new export."""
import ctypes as C
import os
import re

import pytest
import torch

import beam_refs as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("scnattn_beam_workspace", "scnattn_beam_layout", "scnattn_beam_init", "scnattn_beam_steps",
       "scnattn_beam_attn_scores", "scnattn_beam_attn_context", "scnattn_beam_row_topk", "scnattn_beam_merge",
       "scnattn_beam_advance")


def _decoders(V=12):
    from models.decoders.attention_scn import AttentionSCN
    from models.decoders.pure_scn import PureSCN
    from models.decoders.pure_attention import PureAttention
    return [(AttentionSCN(5, 4, 6, 7, 3, V, encoder_dim=8), True), (PureSCN(4, 6, 7, 3, V, encoder_dim=8), True),
            (PureAttention(5, 4, 6, V, encoder_dim=8), False)]


def _args(m, has_tags, N=2):
    enc = torch.rand(N, 2, 2, 8)
    return (enc, torch.rand(N, 3)) if has_tags else (enc,)


def test_sample_batch_exists_and_refuses_cpu_tensors():
    wm = BR.word_map(12)
    for m, has_tags in _decoders():
        assert callable(getattr(m, "sample_batch"))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.sample_batch(3, wm, *_args(m, has_tags))


@pytest.mark.parametrize("k", [0, 9])
def test_beam_size_out_of_range(k):
    wm = BR.word_map(12)
    for m, has_tags in _decoders():
        with pytest.raises(ValueError, match="8"):
            m.sample_batch(k, wm, *_args(m, has_tags))


def test_vocabulary_smaller_than_beam():
    wm = BR.word_map(5)
    for m, has_tags in _decoders(V=5):
        with pytest.raises(ValueError, match="vocab_size"):
            m.sample_batch(6, wm, *_args(m, has_tags))


def test_workspace_query_validates():
    from scnattn import _lib as L
    h = L.lib()
    n = C.c_size_t()
    good = L.Dims(32, 196, 2048, 512, 512, 512, 512, 1000, 10000, 51, 51, 1)
    assert h.scnattn_beam_workspace(C.byref(good), 5, 51, C.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0
    off = (C.c_long * L.BEAM_NOFF)()
    assert h.scnattn_beam_layout(C.byref(good), 5, 51, off) == 0
    assert all(0 <= o < n.value // 4 for o in off) and len(set(off)) == L.BEAM_NOFF
    for dims, K, T, word in [(L.Dims(0, 196, 2048, 512, 512, 512, 512, 1000, 10000, 51, 51, 1), 5, 51, b"positive"),
                             (good, 9, 51, b"beam_size"), (good, 0, 51, b"beam_size"), (good, 5, 0, b"max_steps"),
                             (L.Dims(2, 4, 8, 5, 6, 7, 4, 3, 4, 51, 51, 1), 5, 51, b"vocab_size"),
                             (L.Dims(2, 4, 8, 0, 6, 7, 4, 3, 12, 51, 51, 1), 5, 51, b"attention_dim")]:
        assert h.scnattn_beam_workspace(C.byref(dims), K, T, C.byref(n)) == -1
        assert word in h.scnattn_last_error(), h.scnattn_last_error()
    nat = L.Dims(2, 4, 8, 0, 6, 7, 4, 3, 12, 51, 51, 0)                    # no attention: no alpha record
    assert h.scnattn_beam_layout(C.byref(nat), 3, 51, off) == 0 and off[L.BEAM_NOFF - 1] == -1
    assert h.scnattn_beam_workspace(None, 5, 51, C.byref(n)) == -1


def test_header_declares_every_new_export():
    from scnattn import _lib as L
    header = open(os.path.join(ROOT, "include", "scnattn.h")).read()
    declared = set(re.findall(r"\b(scnattn_[a-z0-9_]+)\s*\(", header))
    h = L.lib()
    for name in NEW:
        assert name in declared and name in L.EXPORTS and hasattr(h, name), name
    assert int(re.search(r"#define SCNATTN_BEAM_NOFF (\d+)", header).group(1)) == L.BEAM_NOFF
    assert h.scnattn_version() == 109
