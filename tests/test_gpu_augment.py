"""GPU tests (``-m gpu``) of the augmentation: scnattn_u8_mean_grey, scnattn_augment_draw and scnattn_u8_gather_augment
through the C ABI, judged per element against fp64 with the bounds of tests/augment_refs.py (nothing is left out near cell
boundaries or clamp kinks), and `DeviceBatchLoader(augment=...)` on a tmp-path split.

Buffers are guarded: the source bytes sit in a flat allocation with a margin on either side, on and one byte off the 16-byte
grid; outputs are the windows of tests/kernel_harness.py (the sentinel around them must survive), on and one element off
it.  Sources of 7 images, random bytes and a smooth ramp with noise, at 3x4x4 (every pixel on a border), 3x8x24 (not square,
W no multiple of 16), 3x32x32 with n = 5 (repeated rows, one index out of range) and 3x256x256 with n = 2 (the real row
size); fp32 and bf16, NCHW and channels-last.  A reference is computed once per (shape, source, table) and shared."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import augment_refs as R
from kernel_harness import GBuf, GBuf16, GBufI, _call, _write_report      # noqa: F401  (_write_report: the report fixture)
from scnattn import augment as A
from scnattn import data as SD
from scnattn import h5lite
from scnattn._lib import AugmentConfig, ptr

pytestmark = pytest.mark.gpu

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
REPORT_TITLE = ("augmentation kernels vs fp64 at the stored parameters: worst |got - ref| / bound over all cases; pixels: counted "
                "roundings + delta x adjacent byte difference x gains / std (bf16: b + 2^-8 (|ref| + b)); parameters: counted "
                "roundings + 4 x CPU-fp32 worst error; grey: 1 fp32 ulp")
ZERO, UNIT = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scnattn import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ---- shared cases and references -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _source(kind, shape):
    N, H, W, n = shape
    src = R.gen_source(kind, N, H, W)
    return src, R.gen_idx(N, n), R.cpu32_grey(src)


@functools.lru_cache(maxsize=None)
def _ref(kind, shape, name, with_grey):
    src, idx, grey = _source(kind, shape)
    params, exact = R.tables(shape[3], shape[1], shape[2])[name]
    return R.batch_ref(src, idx, params, grey if with_grey else None, exact_coords=exact)


class _Bytes:
    """the source images in a flat allocation: 64 bytes of margin on either side, the base `mis` bytes off the 16-byte grid"""

    def __init__(self, dev, src, mis=0):
        host = torch.full((64 + mis + src.numel() + 64,), 0xA5, dtype=torch.uint8)
        host[64 + mis:64 + mis + src.numel()] = src.reshape(-1)
        self.flat = host.to(dev)
        assert self.flat.data_ptr() % 64 == 0
        self.ptr = C.c_void_p(self.flat.data_ptr() + 64 + mis)


def _floats(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _gather(dev, src, idx, params, grey, mean=R.MEAN, std=R.STD, bf16=False, nhwc=False, mis_src=0, mis_dst=0):
    """scnattn_u8_gather_augment on guarded windows -> the batch as float32 / bfloat16 [n, 3, H, W] on the host"""
    N, _, H, W = src.shape
    n = params.shape[0]
    count = n * 3 * H * W
    sb = _Bytes(dev, src, mis_src)
    out = GBuf16(dev, 1, count, mis=mis_dst) if bf16 else GBuf(dev, (count,), out=True, mis=mis_dst)
    idx_d = None if idx is None else idx.to(dev)
    par_d = params.to(dev)
    grey_d = None if grey is None else grey.to(dev)
    _call("scnattn_u8_gather_augment", dev, sb.ptr, N, ptr(idx_d), n, H, W, ptr(par_d), ptr(grey_d), _floats(mean), _floats(std),
          out.ptr, int(bf16), int(nhwc))
    got = out.read("gather_augment").reshape(-1)
    return got.view(n, H, W, 3).permute(0, 3, 1, 2) if nhwc else got.view(n, 3, H, W)


_LAYOUTS = [(bf16, nhwc) for bf16 in (False, True) for nhwc in (False, True)]
_LAYOUT_IDS = ["%s-%s" % ("bf16" if b else "fp32", "nhwc" if c else "nchw") for b, c in _LAYOUTS]


# ---- mean grey -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % (s[1], s[2]))
@pytest.mark.parametrize("kind", ["random", "ramp"])
def test_mean_grey(dev, shape, kind):
    src, _, _ = _source(kind, shape)
    N, H, W = shape[:3]
    results = []
    for mis, with_sums in ((0, True), (1, True), (0, False)):
        sb = _Bytes(dev, src, mis)
        sums = GBufI(dev, 3 * N, wide=True) if with_sums else None
        grey = GBuf(dev, (N,), out=True)
        _call("scnattn_u8_mean_grey", dev, sb.ptr, N, H * W, None if sums is None else sums.ptr, grey.ptr)
        g = grey.read("grey")
        R.judge_grey("u8_mean_grey", None if sums is None else sums.read("sums").view(N, 3), g, src)
        results.append(g)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])      # the vector and the byte path agree
    grey, sums = A.mean_grey(src.to(dev), return_sums=True)
    assert torch.equal(grey.cpu(), results[0]) and torch.equal(sums.cpu(), R.mean_grey_ref(src)[0])


# ---- hand-made tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", _LAYOUTS, ids=_LAYOUT_IDS)
@pytest.mark.parametrize("kind", ["random", "ramp"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % (s[1], s[2]))
def test_tables_against_fp64(dev, shape, kind, layout):
    """identity, flip, dyadic half crop (delta = 0: only the counted roundings remain), a crop flush with the right and bottom
    edges, the smallest legal crop, two colour records and a table that mixes them, with the grey table and with grey =
    NULL; the mixed and the identity table also from bases off the 16-byte grid"""
    bf16, nhwc = layout
    src, idx, grey = _source(kind, shape)
    for name, (params, exact) in R.tables(shape[3], shape[1], shape[2]).items():
        for with_grey in (True, False):
            forms = [(0, 0)] + ([(1, 1)] if name in ("mixed", "identity") and with_grey else [])
            for mis_src, mis_dst in forms:
                got = _gather(dev, src, idx, params, grey if with_grey else None, bf16=bf16, nhwc=nhwc, mis_src=mis_src,
                              mis_dst=mis_dst)
                R.judge_pixels("u8_gather_augment", got, src, idx, params, grey if with_grey else None, exact_coords=exact,
                               bf16=bf16, ref=_ref(kind, shape, name, with_grey))


@pytest.mark.parametrize("layout", _LAYOUTS, ids=_LAYOUT_IDS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % (s[1], s[2]))
def test_identity_and_flip_are_exact(dev, shape, layout):
    """identity: fx = fy = 0 exactly, the result is the three-rounding value of ((b / 255) - mean) / std and lies within 2 ulp
    of gather_normalize with the matching table; flip only: bit-equal to the mirrored identity output"""
    bf16, nhwc = layout
    src, idx, grey = _source("random", shape)
    N, H, W, n = shape
    t = R.tables(n, H, W)
    valid = [i for i in range(n) if 0 <= int(idx[i]) < N]
    want = R.identity_value(src, idx[valid])
    for g in (None, grey):               # contr = 1: the contrast step adds 0 * m
        ident = _gather(dev, src, idx, t["identity"][0], g, bf16=bf16, nhwc=nhwc)
        assert torch.equal(ident[valid], want.to(BF) if bf16 else want)
        assert all(bool(ident[i].isnan().all()) for i in range(n) if i not in valid)
        flipped = _gather(dev, src, idx, t["flip"][0], g, bf16=bf16, nhwc=nhwc)
        assert torch.equal(flipped[valid], ident[valid].flip(3))
    lut = torch.from_numpy(SD.normalize_lut(R.MEAN, R.STD)).to(dev)
    plain = SD.gather_normalize(src.to(dev), idx.to(dev), lut, dtype=F32).cpu()[valid]
    ulp = torch.from_numpy(np.spacing(np.abs(plain.numpy())))
    assert bool(((want - plain).abs() <= 2 * ulp).all())
    # through the Python surface: the same bits, in the memory format asked for
    dt = BF if bf16 else F32
    api = A.gather_augment(src.to(dev), idx.to(dev), A.identity_params(n, H, W, dev), R.MEAN, R.STD, dtype=dt, channels_last=nhwc)
    assert api.is_contiguous(memory_format=torch.channels_last if nhwc else torch.contiguous_format) and api.dtype == dt
    assert torch.equal(api.cpu()[valid], ident[valid])


@pytest.mark.parametrize("shape", R.SHAPES[:3], ids=lambda s: "%dx%d" % (s[1], s[2]))
def test_colour_special_cases(dev, shape):
    """bright = 0: every output is (0 - mean_c) / std_c; sat = 0: the three channels are equal before normalisation; contr = 0:
    every pixel equals m = min(1, bright grey[row])"""
    src, idx, grey = _source("ramp", shape)
    N, H, W, n = shape
    valid = [i for i in range(n) if 0 <= int(idx[i]) < N]
    crop = dict(x0=0.2 * W, y0=0.1 * H, w=0.7 * W, h=0.8 * H)
    m32 = torch.tensor(R.MEAN, dtype=F32).view(1, 3, 1, 1)
    s32 = torch.tensor(R.STD, dtype=F32).view(1, 3, 1, 1)
    for nhwc in (False, True):
        got = _gather(dev, src, idx, R.table(n, H, W, bright=0.0, contr=0.7, sat=1.3, **crop), grey, nhwc=nhwc)[valid]
        assert torch.equal(got, ((0.0 - m32) / s32).expand_as(got))
        got = _gather(dev, src, idx, R.table(n, H, W, sat=0.0, bright=1.2, contr=0.7, **crop), grey, ZERO, UNIT, nhwc=nhwc)[valid]
        assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 1], got[:, 2]) and float(got.std()) > 0
        params = R.table(n, H, W, contr=0.0, bright=1.3, **crop)
        got = _gather(dev, src, idx, params, grey, ZERO, UNIT, nhwc=nhwc)[valid]
        want = torch.minimum(torch.tensor(1.0), params[0, 5] * grey[idx[valid]]).view(-1, 1, 1, 1)
        assert torch.equal(got, want.expand_as(got))
        R.judge_pixels("u8_gather_augment", _gather(dev, src, idx, params, grey, ZERO, UNIT, nhwc=nhwc), src, idx, params, grey,
                       ZERO, UNIT)


# ---- drawn tables ----------------------------------------------------------------------------------------------------------
def _draw(dev, cfg, seed, epoch, sid, H, W):
    n = len(sid)
    sid_d = torch.tensor(sid, dtype=torch.int64, device=dev)
    out = GBuf(dev, (n * 8,), out=True)
    c = AugmentConfig(*cfg)
    _call("scnattn_augment_draw", dev, n, ptr(sid_d), epoch, seed, C.byref(c), H, W, out.ptr)
    return out.read("params").view(n, 8)


@pytest.mark.parametrize("cfg", sorted(R.CONFIGS))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % (s[1], s[2]))
def test_drawn_tables(dev, shape, cfg):
    """the records of scnattn_augment_draw judged as drawn parameters; (seed, epoch, sid) repeats them bit for bit whatever
    the batch they are drawn in; the pixels made from them judged against fp64 at the stored records"""
    N, H, W, n = shape
    c = R.CONFIGS[cfg]
    seed, epoch = 0x123456789ABCDEF, 3
    sid = [0, 1, 2, 77, (1 << 40) + 3, -1] + list(range(1000, 1300))
    got = _draw(dev, c, seed, epoch, sid, H, W)
    R.judge_params("augment_draw", got, c, seed, epoch, sid, H, W)
    again = _draw(dev, c, seed, epoch, sid[::-1][:17], H, W)
    assert torch.equal(again, got.flip(0)[:17])
    if cfg != "narrow":
        assert not torch.equal(_draw(dev, c, seed, epoch + 1, sid[:8], H, W), got[:8])
        assert not torch.equal(_draw(dev, c, seed + (1 << 32), epoch, sid[:8], H, W), got[:8])
        assert not torch.equal(_draw(dev, c, seed + 1, epoch, sid[:8], H, W), got[:8])
    aug = A.Augment(scale=c[:2], ratio=c[2:4], flip=c[4], brightness=c[5], contrast=c[6], saturation=c[7], seed=seed)
    api = aug.draw(torch.tensor(sid, dtype=torch.int64, device=dev), epoch, H, W)
    assert torch.equal(api.cpu(), got)
    src, idx, grey = _source("random", shape)
    params = got[3:3 + n].contiguous()
    want = R.batch_ref(src, idx, params, grey)
    for bf16, nhwc in _LAYOUTS:
        R.judge_pixels("u8_gather_augment", _gather(dev, src, idx, params, grey, bf16=bf16, nhwc=nhwc), src, idx, params, grey,
                       bf16=bf16, ref=want)


# ---- the loader ----------------------------------------------------------------------------------------------------------
BASE = "aug_2_cap_per_img_0_min_word_freq"
NIMG, CPI, LCAP, SIDE = 11, 2, 7, 32


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    d = tmp_path_factory.mktemp("augment_split")
    rng = np.random.RandomState(5)
    u8 = R.gen_source("ramp", NIMG, SIDE, SIDE, seed=3).numpy()
    caps = rng.randint(1, 20, size=(NIMG * CPI, LCAP)).tolist()
    lens = rng.randint(3, LCAP + 1, size=NIMG * CPI).tolist()
    for name in ("TRAIN", "VAL"):
        h5lite.write_arrays(str(d / ("%s_IMAGES_%s.hdf5" % (name, BASE))), {"images": u8}, {"captions_per_image": CPI})
        json.dump(caps, open(str(d / ("%s_CAPTIONS_%s.json" % (name, BASE))), "w"))
        json.dump(lens, open(str(d / ("%s_CAPLENS_%s.json" % (name, BASE))), "w"))
    return str(d), torch.from_numpy(u8)


def _loader(split, dev, augment, batch=5, **kw):
    return SD.DeviceBatchLoader(split[0], BASE, kw.pop("name", "TRAIN"), batch, dev, cpi=CPI, shuffle=True, seed=4, augment=augment, **kw)


def _epoch(ld, epoch):
    ld.set_epoch(epoch)
    return [b[0].clone() for b in ld]


def test_loader_modes_epochs_seeds_and_ranks(dev, split):
    aug = A.Augment(seed=11)
    res = _loader(split, dev, aug, resident=True)
    stg = _loader(split, dev, aug, resident=False)
    assert res.resident and not stg.resident and res.grey is not None and stg.grey is None
    e0 = _epoch(res, 0)
    assert len(e0) == len(res) == 5 and [int(b.shape[0]) for b in e0] == [5, 5, 5, 5, 2]
    for a, b in zip(e0, _epoch(stg, 0)):                      # resident equals staged, bitwise
        assert torch.equal(a, b) and a.is_contiguous(memory_format=torch.channels_last)
    for a, b in zip(e0, _epoch(res, 0)):                      # the same (seed, epoch) repeats the epoch
        assert torch.equal(a, b)
    # the pixels are the reference's for the sample ids of the batch: judged at the records the device draws
    order = SD.epoch_order(NIMG * CPI, 0, 4, True)
    sel = torch.from_numpy(order[:5])
    params = aug.draw(sel.to(dev), 0, SIDE, SIDE).cpu()
    R.judge_params("augment_draw", params, R.CFG_DEFAULT, 11, 0, sel.tolist(), SIDE, SIDE)
    grey = res.grey.cpu()                                     # the table the kernel read
    R.judge_grey("u8_mean_grey", None, grey, split[1])
    R.judge_pixels("u8_gather_augment", e0[0], split[1], sel // CPI, params, grey)
    # another epoch: the same sample gets another view (compare per sample id, not per batch position)
    e1 = torch.cat(_epoch(res, 1))
    order1 = SD.epoch_order(NIMG * CPI, 1, 4, True)
    by0 = torch.cat(e0)[torch.from_numpy(np.argsort(order))]
    by1 = e1[torch.from_numpy(np.argsort(order1))]
    assert all(not torch.equal(by0[s], by1[s]) for s in range(NIMG * CPI))
    other = torch.cat(_epoch(_loader(split, dev, A.Augment(seed=12), resident=True), 0))       # another seed
    assert all(not torch.equal(by0[s], other[torch.from_numpy(np.argsort(order))][s]) for s in range(NIMG * CPI))
    # the captions of one image see different views
    assert not torch.equal(by0[0], by0[1])
    # another batch size and two ranks: the same pixels for the same sample ids
    big = torch.cat(_epoch(_loader(split, dev, aug, batch=7, resident=True), 0))
    assert torch.equal(big, torch.cat(e0))
    for rank in (0, 1):
        for resident in (True, False):
            ld = _loader(split, dev, aug, batch=4, resident=resident, rank=rank, world=2)
            mine = SD.epoch_order(NIMG * CPI, 0, 4, True, rank, 2)
            got = torch.cat(_epoch(ld, 0))
            assert got.shape[0] == len(mine) and torch.equal(got, by0[torch.from_numpy(mine)])
    # bf16 and NCHW go through the same records
    b16 = _epoch(_loader(split, dev, aug, resident=True, dtype=BF, channels_last=False), 0)[0]
    assert b16.dtype == BF and b16.is_contiguous()
    R.judge_pixels("u8_gather_augment", b16, split[1], sel // CPI, params, grey, bf16=True)
    # without contrast no grey table is made, resident or staged, and the batches still agree
    nc = A.Augment(contrast=0.0, seed=11)
    r2, s2 = _loader(split, dev, nc, resident=True), _loader(split, dev, nc, resident=False)
    assert r2.grey is None
    for a, b in zip(_epoch(r2, 0), _epoch(s2, 0)):
        assert torch.equal(a, b)


def test_loader_without_augment_is_the_plain_kernel_and_launches_nothing_else(dev, split, monkeypatch):
    names = []

    def spy(real):
        def call(name, *args):
            names.append(name)
            return real(name, *args)
        return call

    monkeypatch.setattr(SD, "call", spy(SD.call))
    monkeypatch.setattr(A, "call", spy(A.call))
    ident = A.Augment(scale=(1, 1), ratio=(1, 1), flip=0, brightness=0, contrast=0, saturation=0)
    lut = torch.from_numpy(SD.normalize_lut()).to(dev)
    src = split[1].to(dev)
    order = torch.from_numpy(SD.epoch_order(NIMG * CPI, 0, 4, True))
    for augment in (None, ident):
        for resident in (True, False):
            ld = _loader(split, dev, augment, resident=resident)
            assert ld.augment is None and ld.grey is None
            del names[:]
            got = torch.cat(_epoch(ld, 0))
            assert names == ["scnattn_u8_gather_normalize"] * len(ld)
            want = SD.gather_normalize(src, (order // CPI).to(dev), lut, channels_last=True)
            assert torch.equal(got, want)
    del names[:]
    ld = _loader(split, dev, A.Augment(), resident=True)
    assert names == ["scnattn_u8_mean_grey"]
    _epoch(ld, 0)
    assert names == ["scnattn_u8_mean_grey"] + ["scnattn_augment_draw", "scnattn_u8_gather_augment"] * len(ld)      # two launches per batch


def test_loader_refuses_augment_outside_train(dev, split):
    with pytest.raises(ValueError) as e:
        _loader(split, dev, A.Augment(), name="VAL")
    assert "TRAIN split only" in str(e.value)
    assert _loader(split, dev, None, name="VAL").augment is None


def test_train_step_on_an_augmented_batch(dev, tmp_path):
    """one TrainStep step (fine-tuned 1-1-1-1 trunk, channels-last) on an augmented batch of 8, the batch of the suite's
    end-to-end test of the loader: the loss is finite"""
    from models.encoders.caption import EncoderCaption
    from scnattn.resnet import resnet152_trunk
    from trains.harness import TrainStep
    from utils.optimizer import FusedClampAdam
    rng = np.random.RandomState(3)
    base = "augstep_1_cap_per_img_0_min_word_freq"
    V, L, N = 30, 9, 8
    imgs = rng.randint(0, 256, size=(N, 3, 64, 64)).astype(np.uint8)
    h5lite.write_arrays(str(tmp_path / ("TRAIN_IMAGES_%s.hdf5" % base)), {"images": imgs}, {"captions_per_image": 1})
    caps, lens = [], []
    for _ in range(N):
        k = rng.randint(3, L - 1)
        caps.append([V - 2] + rng.randint(1, V - 4, size=k).tolist() + [V - 1] + [0] * (L - 2 - k))
        lens.append(k + 2)
    json.dump(caps, open(str(tmp_path / ("TRAIN_CAPTIONS_%s.json" % base)), "w"))
    json.dump(lens, open(str(tmp_path / ("TRAIN_CAPLENS_%s.json" % base)), "w"))
    torch.manual_seed(0)
    ts = TrainStep(kind="attention_scn", fine_tune_encoder=True, device=dev, encoder=False, seed=0, emb_dim=32,
                   attention_dim=32, decoder_dim=48, factored_dim=32, semantic_dim=10, vocab_size=V, dropout=0.0,
                   max_len=L - 2, decoder_lr=4e-3)
    enc = EncoderCaption(channels_last=True)
    enc.resnet = resnet152_trunk(depths=(1, 1, 1, 1))
    enc = enc.to(dev).train()
    enc.fine_tune(True)
    enc_opt = FusedClampAdam([p for p in enc.parameters() if p.requires_grad], lr=1e-4, grad_clip=5.0)
    loader = SD.DeviceBatchLoader(str(tmp_path), base, "TRAIN", 8, dev, cpi=1, shuffle=True, seed=0, augment=A.Augment(seed=2))
    batch, caps_d, caplens = next(iter(loader))
    assert batch.shape == (8, 3, 64, 64) and bool(torch.isfinite(batch).all())
    enc_opt.zero_grad()
    loss = ts.step(None, torch.rand(N, 10, device=dev), caps_d, caplens, None, enc(batch, pooled=False))
    enc_opt.step()
    assert np.isfinite(float(loss.detach()))
