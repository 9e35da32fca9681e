"""Device-side input pipeline for the caption train/validation loops.

Reference: `CaptionDataset` (datasets/caption.py:19-65) behind a `torch.utils.data.DataLoader`
(trains/attention_scn.py:121-130, `shuffle=True`, `workers = 1  # only 1 works with h5py`): every sample
is a float image made on the host (`imgs[i // cpi] / 255.`, then `Normalize(mean, std)`), collated and
copied to the GPU as fp32.

MI355X-first shape of the same thing:
  * the uint8 image rows are memory-mapped straight out of the HDF5 file (`h5lite`, no h5py);
  * `resident=True` (default whenever the dataset fits the HBM budget — 118k COCO images are 23 GB of
    288): the whole uint8 dataset, all captions and lengths are uploaded once; a step's batch is ONE
    launch of `scnattn_u8_gather_normalize` (gather rows by index + /255 + Normalize + layout/type the
    encoder wants) plus two index_selects for the captions — no host work and no PCIe traffic per step;
  * otherwise batches are staged: a producer thread gathers the batch rows into pinned uint8 buffers
    (4x less PCIe traffic than the reference's fp32 tensors), copies them on a side stream ahead of the
    consumer, and the same kernel normalises them on the consumer's stream;
  * data parallel: every rank draws the same per-epoch permutation and takes a strided slice of it
    (wrap-padded to equal length, as DistributedSampler does), so ranks stay in lock-step.
The arithmetic is bit-identical to the reference's (table lookup of its own per-value results,
`normalize_lut`).  There is no CPU fallback: batches are produced on the GPU.
"""
import functools
import json
import math
import os
import queue
import threading

import numpy as np
import torch

from . import h5lite
from .augment import gather_augment, mean_grey
from ._lib import RESIZE_MAX_DIM, ImageDesc, call, ptr, require_cuda, stream_of

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # trains/attention_scn.py:121-122
IMAGENET_STD = (0.229, 0.224, 0.225)


def normalize_lut(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """lut[c][v] = the reference's value for pixel byte v in channel c: `torch.FloatTensor(v / 255.)`
    (numpy float64 divide, rounded to float32; datasets/caption.py:51) then torchvision Normalize
    `(t - mean[c]) / std[c]` with float32 mean/std tensors (float32 subtract, float32 IEEE divide)."""
    v = (np.arange(256, dtype=np.uint8) / 255.).astype(np.float32)
    m = np.asarray(mean, dtype=np.float32)
    s = np.asarray(std, dtype=np.float32)
    if m.ndim != 1 or m.shape != s.shape:
        raise ValueError("mean/std must be per-channel sequences of equal length")
    if (s == 0).any():
        raise ValueError("std evaluated to zero after conversion to torch.float32, leading to division by zero.")
    return ((v[None, :] - m[:, None]) / s[:, None]).astype(np.float32)


def identity_lut(channels=3):
    """Only the `/ 255.` of datasets/caption.py:51 (transform=None)."""
    v = (np.arange(256, dtype=np.uint8) / 255.).astype(np.float32)
    return np.repeat(v[None, :], channels, axis=0).copy()


def gather_normalize(src, idx, lut, n_out=None, dtype=torch.float32, channels_last=False, out=None):
    """src: uint8 [N, C, H, W] on the GPU; idx: int64 [n] rows to take (None: rows 0..n_out-1);
    lut: float32 [C, 256] on the GPU.  Returns the normalised batch [n, C, H, W] (`channels_last` selects
    the memory format, not the logical shape — what `EncoderCaption(channels_last=True)` consumes)."""
    require_cuda(src, idx, lut)
    if src.dtype != torch.uint8 or src.dim() != 4 or not src.is_contiguous():
        raise RuntimeError("gather_normalize: src must be a contiguous uint8 [N, C, H, W] tensor")
    N, Cn, H, W = src.shape
    if lut.dtype != torch.float32 or tuple(lut.shape) != (Cn, 256) or not lut.is_contiguous():
        raise RuntimeError("gather_normalize: lut must be float32 [C, 256]")
    if idx is not None:
        if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
            raise RuntimeError("gather_normalize: idx must be a contiguous int64 vector")
        n_out = idx.numel()
    elif n_out is None:
        n_out = N
    if n_out > N and idx is None:
        raise RuntimeError("gather_normalize: n_out exceeds the source rows")
    if dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("gather_normalize: dtype must be float32 or bfloat16")
    if out is None:
        out = torch.empty((n_out, Cn, H, W), device=src.device, dtype=dtype,
                          memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    call("scnattn_u8_gather_normalize", stream_of(src), ptr(src), N, ptr(idx), n_out, Cn, H * W, ptr(lut), ptr(out),
         int(dtype == torch.bfloat16), int(bool(channels_last)))
    return out


# ---- raw images -> the rows above: `scipy.misc.imresize(img, size)` of inference.py:33-38 and utils/dataset.py:368-373 ----
FILTERS = ("bilinear", "lanczos")
_libm_sin = np.frompyfunc(math.sin, 1, 1)      # Pillow calls libm's sin; numpy's own may differ in the last bit


def _sinc(x):                                   # Pillow's sinc_filter: 1 at 0, else sin(x * pi) / (x * pi)
    xp = x * np.float64(math.pi)
    s = _libm_sin(xp).astype(np.float64)
    return np.divide(s, xp, out=np.ones_like(xp), where=x != 0.0)


def resize_taps(in_size, out_size, filter="bilinear"):
    """Pillow's coefficient table of one axis (`precompute_coeffs` + `normalize_coeffs_8bpc`), the same float64
    operations in the same order, in numpy so that no compiler contracts a multiply-add:
    `(xmin int32[out], n int32[out], coeff int32[out, ksize])`; output i of the 8-bit pass is
    clip8((2^21 + sum_{k < n[i]} coeff[i, k] * in[xmin[i] + k]) >> 22).  filter: "bilinear" (`bilinear_filter`, support
    1, ksize = 2 * ceil(max(in / out, 1)) + 1) or "lanczos" (`lanczos_filter`, support 3, negative weights, ksize =
    2 * ceil(3 * max(in / out, 1)) + 1 evaluated in double as Pillow does).  Cached per (in, out, filter); the arrays
    are read-only.  An axis with in == out has no pass in Pillow -- `pack_images` leaves it out, it does not apply this
    table."""
    return _resize_taps(int(in_size), int(out_size), filter)


@functools.lru_cache(maxsize=1024)
def _resize_taps(in_size, out_size, filter):
    if filter not in FILTERS:
        raise ValueError("resize_taps: filter must be one of %r (got %r)" % (FILTERS, filter))
    if not (1 <= in_size <= RESIZE_MAX_DIM and 1 <= out_size <= RESIZE_MAX_DIM):
        raise ValueError("resize_taps: sizes must be in [1, %d] (got %d -> %d)" % (RESIZE_MAX_DIM, in_size, out_size))
    scale = np.float64(in_size) / np.float64(out_size)
    filterscale = max(scale, np.float64(1.0))
    support = np.float64(1.0 if filter == "bilinear" else 3.0) * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = np.float64(1.0) / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    if filter == "bilinear":
        a = np.abs(a)
        w = np.where((a < 1.0) & (x < n[:, None]), 1.0 - a, 0.0)
    else:
        w = np.where((a >= -3.0) & (a < 3.0) & (x < n[:, None]), _sinc(a) * _sinc(a / np.float64(3.0)), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                       # Pillow adds the weights one by one, left to right
    w = np.divide(w, ww, out=w.copy(), where=ww != 0.0)
    w = w * np.float64(1 << 22)
    coeff = np.trunc(np.where(w < 0, -0.5, 0.5) + w).astype(np.int32)      # a negative weight rounds with -0.5
    out = (xmin.astype(np.int32), n.astype(np.int32), coeff)
    for arr in out:
        arr.setflags(write=False)
    return out


class PackedImages:
    """A batch of decoded images in ONE pinned byte buffer -- descriptors, then the tap tables, then the pixels -- so
    that the batch is one host-to-device copy.  `desc` (ctypes array of `ImageDesc`) and `taps` (int32) are views of it."""

    def __init__(self, buffer, n, size, desc_bytes, taps_len, src_off, filter="bilinear"):
        self.buffer, self.n, self.size, self.filter = buffer, n, size, filter
        self.taps_off, self.taps_len, self.src_off = desc_bytes, taps_len, src_off
        self.src_bytes = buffer.numel() - src_off
        raw = buffer.numpy()
        self.desc = (ImageDesc * n).from_buffer(raw[:desc_bytes])
        self.taps = raw[desc_bytes:desc_bytes + 4 * taps_len].view(np.int32)


def pack_images(images, size=(256, 256), filter="bilinear"):
    """images: numpy uint8 arrays, each H x W x 3 or H x W (grey), as a decoder hands them over; size: (OH, OW).
    Returns the `PackedImages` `resize_u8` / `resize_normalize` upload: per image a descriptor (byte offset, H, W, C,
    the offsets of its two axis tables), one table per distinct (in, out) pair of the batch (none for an axis that
    keeps its size), and the pixels, each image 16-byte aligned.  filter "bilinear": the tables of
    `scnattn_u8_resize_bilinear`; any other filter of `resize_taps`: those of `scnattn_u8_resize_taps`, each led by a
    header word holding its row length ksize."""
    OH, OW = int(size[0]), int(size[1])
    if filter not in FILTERS:
        raise ValueError("pack_images: filter must be one of %r (got %r)" % (FILTERS, filter))
    if not (1 <= OH <= RESIZE_MAX_DIM and 1 <= OW <= RESIZE_MAX_DIM):
        raise ValueError("pack_images: target size must be in [1, %d]" % RESIZE_MAX_DIM)
    images = list(images)
    if not images:
        raise ValueError("pack_images: no images")
    tables, tab_off, taps_len = [], {}, 0
    metas, nbytes = [], 0
    for k, im in enumerate(images):
        if not isinstance(im, np.ndarray) or im.dtype != np.uint8:
            raise ValueError("pack_images: image %d is not a numpy uint8 array" % k)
        if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3):
            raise ValueError("pack_images: image %d has shape %r; H x W or H x W x 3 is required" % (k, im.shape))
        H, W = im.shape[:2]
        if not (1 <= H <= RESIZE_MAX_DIM and 1 <= W <= RESIZE_MAX_DIM):
            raise ValueError("pack_images: image %d has shape %r; sides must be in [1, %d]" % (k, im.shape, RESIZE_MAX_DIM))
        offs = []
        for pair in ((W, OW), (H, OH)):
            if pair[0] != pair[1] and pair not in tab_off:
                xmin, n, coeff = resize_taps(*pair, filter=filter)
                tab_off[pair] = taps_len
                if filter != "bilinear":
                    tables.append(np.asarray([coeff.shape[1]], np.int32))
                    taps_len += 1
                tables += [xmin, n, coeff.ravel()]
                taps_len += xmin.size + n.size + coeff.size
            offs.append(tab_off.get(pair, -1))
        metas.append((nbytes, H, W, 1 if im.ndim == 2 else im.shape[2], offs[0], offs[1]))
        nbytes += -(-im.size // 16) * 16
    desc_bytes = len(images) * 32
    src_off = -(-(desc_bytes + 4 * taps_len) // 16) * 16
    buffer = torch.empty(src_off + nbytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    packed = PackedImages(buffer, len(images), (OH, OW), desc_bytes, taps_len, src_off, filter)
    if tables:
        np.concatenate(tables, out=packed.taps)
    pixels = buffer.numpy()[src_off:]
    for k, (im, m) in enumerate(zip(images, metas)):
        packed.desc[k] = ImageDesc(*m, 0)
        pixels[m[0]:m[0] + im.size] = im.reshape(-1)
    return packed


def upload_images(packed, device):
    """The packed batch on the device: descriptors, tables and pixels in one (asynchronous) copy."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("scnattn: images are resized on an MI355X device (got %s); there is no CPU fallback" % device)
    return packed.buffer.to(device, non_blocking=True)


def resize_uploaded(packed, dev_buffer, lut=None, dtype=torch.float32, channels_last=False):
    """One launch of `scnattn_u8_resize_bilinear` (`scnattn_u8_resize_taps` for a batch packed with another filter)
    on `upload_images(packed, device)`: the uint8 rows (lut None) or the normalised batch."""
    require_cuda(dev_buffer, lut)
    if dev_buffer.dtype != torch.uint8 or dev_buffer.numel() != packed.buffer.numel() or not dev_buffer.is_contiguous():
        raise RuntimeError("resize_uploaded: dev_buffer is not the upload of this batch")
    OH, OW = packed.size
    if lut is None:
        out = torch.empty((packed.n, 3, OH, OW), device=dev_buffer.device, dtype=torch.uint8)
        kind = 0
    else:
        if lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256) or not lut.is_contiguous():
            raise RuntimeError("resize_normalize: lut must be float32 [3, 256]")
        if dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError("resize_normalize: dtype must be float32 or bfloat16")
        out = torch.empty((packed.n, 3, OH, OW), device=dev_buffer.device, dtype=dtype,
                          memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        kind = 1 if dtype == torch.float32 else 2
    base = dev_buffer.data_ptr()
    if packed.filter == "bilinear":
        call("scnattn_u8_resize_bilinear", stream_of(out), base + packed.src_off, packed.src_bytes, packed.desc, base,
             packed.n, base + packed.taps_off, packed.taps_len, OH, OW, ptr(lut), ptr(out), kind,
             int(bool(channels_last) and kind != 0))
    else:       # the tables carry their row length; the entry point checks the host copy of them before the launch
        call("scnattn_u8_resize_taps", stream_of(out), base + packed.src_off, packed.src_bytes, packed.desc, base,
             packed.n, packed.taps.ctypes.data, base + packed.taps_off, packed.taps_len, OH, OW, ptr(lut), ptr(out), kind,
             int(bool(channels_last) and kind != 0))
    return out


def _resize(images, size, device, lut, dtype, channels_last, filter):
    if torch.device(device).type != "cuda":
        raise RuntimeError("scnattn: images are resized on an MI355X device (got %s); there is no CPU fallback" % device)
    packed = images if isinstance(images, PackedImages) else pack_images(images, size, filter)
    return resize_uploaded(packed, upload_images(packed, device), lut, dtype, channels_last)


def resize_u8(images, size=(256, 256), device="cuda", filter="bilinear"):
    """`imresize(img, size).transpose(2, 0, 1)` of every image (a grey one replicated to three planes first), on the
    device, byte for byte what Pillow gives: uint8 [N, 3, OH, OW] -- the rows utils/dataset.py:373-379 stores and
    `gather_normalize` reads.  images: a list for `pack_images`, or its result (which carries its own filter).
    filter "lanczos": `Image.resize(..., LANCZOS)`, what utils/vizualize.py:22 shows.  One copy, one launch."""
    return _resize(images, size, device, None, None, False, filter)


def resize_normalize(images, lut, size=(256, 256), dtype=torch.float32, channels_last=False, filter="bilinear"):
    """The batch the encoders consume, straight from decoded images: equals
    `gather_normalize(resize_u8(images, size), None, lut, dtype=dtype, channels_last=channels_last)` bit for bit
    without the uint8 rows ever being written.  lut: float32 [3, 256] on the device (`normalize_lut`)."""
    if lut is None:
        raise RuntimeError("resize_normalize: lut is required (normalize_lut / identity_lut)")
    return _resize(images, size, lut.device, lut, dtype, channels_last, filter)


class CaptionFiles:
    """The on-disk artefacts of one split, as written by utils/dataset.py:303-414."""

    def __init__(self, data_folder, data_name, split, cpi=5):
        assert split in {"TRAIN", "VAL", "TEST"}
        self.split = split
        self.h = h5lite.File(os.path.join(data_folder, split + "_IMAGES_" + data_name + ".hdf5"))
        ds = self.h["images"]
        if ds.dtype != np.uint8 or len(ds.shape) != 4:
            raise RuntimeError("'images' must be a uint8 (N, C, H, W) dataset, found %r" % (ds,))
        self.imgs = ds.array                       # zero-copy view of the file
        self.cpi = cpi if cpi else int(self.h.attrs["captions_per_image"])   # datasets/caption.py:32
        with open(os.path.join(data_folder, split + "_CAPTIONS_" + data_name + ".json")) as j:
            self.captions = np.asarray(json.load(j), dtype=np.int64)
        with open(os.path.join(data_folder, split + "_CAPLENS_" + data_name + ".json")) as j:
            self.caplens = np.asarray(json.load(j), dtype=np.int64)
        if self.captions.ndim != 2 or self.caplens.shape != (self.captions.shape[0],):
            raise RuntimeError("captions / caplens files are inconsistent")
        if (len(self.captions) - 1) // self.cpi >= self.imgs.shape[0]:
            raise RuntimeError("%d captions at %d per image need more than the %d stored images"
                               % (len(self.captions), self.cpi, self.imgs.shape[0]))

    def __len__(self):
        return len(self.captions)      # datasets/caption.py:48


def epoch_order(n, epoch, seed, shuffle, rank=0, world=1):
    """Sample indices this rank visits in `epoch`: one global permutation (same on every rank), wrap-padded
    to a multiple of `world`, rank r takes positions r, r+world, ..."""
    if shuffle:
        order = np.random.RandomState((seed * 1000003 + epoch) % (2 ** 31)).permutation(n)
    else:
        order = np.arange(n)
    if world > 1:
        total = -(-n // world) * world
        if total > n:
            order = np.concatenate([order, order[:total - n]])
        order = order[rank::world]
    return order.astype(np.int64)


class DeviceBatchLoader:
    """Iterable of device batches `(imgs, caps, caplens)` for TRAIN or `(imgs, caps, caplens, allcaps)`
    otherwise — the tuples the reference's loops unpack (trains/attention_scn.py:205, 304)."""

    def __init__(self, data_folder, data_name, split, batch_size, device, cpi=5, shuffle=True, seed=0, rank=0,
                 world=1, dtype=torch.float32, channels_last=True, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                 resident=None, hbm_budget_bytes=64 << 30, prefetch=2, drop_last=False, augment=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceBatchLoader produces batches on an MI355X device; there is no CPU fallback "
                               "(datasets.caption.CaptionDataset is the host-side reader)")
        self.files = CaptionFiles(data_folder, data_name, split, cpi)
        self.split, self.batch_size, self.shuffle, self.seed = split, int(batch_size), shuffle, seed
        self.rank, self.world, self.dtype, self.channels_last = rank, world, dtype, channels_last
        self.drop_last, self.prefetch, self.epoch = drop_last, max(1, int(prefetch)), 0
        lut = identity_lut(self.files.imgs.shape[1]) if mean is None else normalize_lut(mean, std)
        if lut.shape[0] != self.files.imgs.shape[1]:
            raise ValueError("mean/std have %d channels, the images %d" % (lut.shape[0], self.files.imgs.shape[1]))
        self.lut = torch.from_numpy(lut).to(self.device)
        self.caps_dev = torch.from_numpy(self.files.captions).to(self.device)
        self.caplens_dev = torch.from_numpy(self.files.caplens).to(self.device)
        nbytes = self.files.imgs.nbytes
        self.resident = (nbytes <= hbm_budget_bytes) if resident is None else bool(resident)
        self.imgs_dev = self._upload() if self.resident else None
        # augment: a scnattn.augment.Augment -- crop, flip and colour jitter inside the gather (two launches per batch
        # instead of one); None, or one whose every draw is the identity, leaves the plain kernel in place
        if augment is not None and split != "TRAIN":
            raise ValueError("augment is for the TRAIN split only (got %s): validation sees the images as they are" % split)
        self.augment = None if augment is None or augment.is_identity else augment
        self.grey = None
        if self.augment is not None:
            if self.files.imgs.shape[1] != 3:
                raise ValueError("augment needs images of 3 planes, found %d" % self.files.imgs.shape[1])
            self.norm = (None, None) if mean is None else (tuple(mean), tuple(std))
            if self.resident and self.augment.contrast != 0.0:
                self.grey = mean_grey(self.imgs_dev)              # once: the contrast step reads the SOURCE image's mean

    # ---- one-off upload of the uint8 dataset ---------------------------------------------------------------
    def _upload(self, chunk_rows=256):
        src = self.files.imgs
        N = src.shape[0]
        dev = torch.empty(src.shape, dtype=torch.uint8, device=self.device)
        stage = [torch.empty((min(chunk_rows, N),) + src.shape[1:], dtype=torch.uint8).pin_memory() for _ in range(2)]
        evs = [None, None]
        for k, a in enumerate(range(0, N, chunk_rows)):
            b = min(a + chunk_rows, N)
            s = k & 1
            if evs[s] is not None:
                evs[s].synchronize()
            np.copyto(stage[s].numpy()[:b - a], src[a:b])
            dev[a:b].copy_(stage[s][:b - a], non_blocking=True)
            evs[s] = torch.cuda.Event()
            evs[s].record(torch.cuda.current_stream(self.device))
        torch.cuda.current_stream(self.device).synchronize()
        return dev

    # ---- epoch bookkeeping --------------------------------------------------------------------------
    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _order(self):
        return epoch_order(len(self.files), self.epoch, self.seed, self.shuffle, self.rank, self.world)

    def __len__(self):
        n = -(-len(self.files) // self.world) if self.world > 1 else len(self.files)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _images(self, src, rows, n, sel, grey):
        """the batch of `n` images: rows `rows` of src (None: the first n), augmented as samples `sel` when asked for"""
        if self.augment is None:
            return gather_normalize(src, rows, self.lut, n_out=n, dtype=self.dtype, channels_last=self.channels_last)
        params = self.augment.draw(sel, self.epoch, src.shape[2], src.shape[3])
        return gather_augment(src, rows, params, self.norm[0], self.norm[1], grey=grey, dtype=self.dtype,
                              channels_last=self.channels_last)

    def _tuple(self, imgs, sel):
        caps = self.caps_dev.index_select(0, sel)
        caplens = self.caplens_dev.index_select(0, sel).unsqueeze(1)          # LongTensor([caplen]) per sample
        if self.split == "TRAIN":
            return imgs, caps, caplens
        cpi = self.files.cpi                                                    # datasets/caption.py:62-63
        first = torch.div(sel, cpi, rounding_mode="floor") * cpi
        rows = first.unsqueeze(1) + torch.arange(cpi, device=self.device)
        return imgs, caps, caplens, self.caps_dev[rows]

    def __iter__(self):
        order = self._order()
        nb = len(self)
        if self.resident:
            order_dev = torch.from_numpy(order).to(self.device)              # once per epoch
            img_rows = torch.div(order_dev, self.files.cpi, rounding_mode="floor")
            for b in range(nb):
                sl = slice(b * self.batch_size, min((b + 1) * self.batch_size, len(order)))
                sel = order_dev[sl]
                imgs = self._images(self.imgs_dev, img_rows[sl].contiguous(), None, sel, self.grey)
                yield self._tuple(imgs, sel)
            return
        yield from self._iter_staged(order, nb)

    # ---- staged mode: pinned uint8 batches copied ahead on a side stream ------------------------------
    def _iter_staged(self, order, nb):
        B = self.batch_size
        src = self.files.imgs
        nslots = self.prefetch + 2
        pinned = [torch.empty((B,) + src.shape[1:], dtype=torch.uint8).pin_memory() for _ in range(nslots)]
        staged = [torch.empty((B,) + src.shape[1:], dtype=torch.uint8, device=self.device) for _ in range(nslots)]
        copied = [None] * nslots          # event: H2D of the slot finished (side stream)
        released = [None] * nslots        # event: consumer's kernel has read the slot (consumer stream)
        q = queue.Queue(maxsize=self.prefetch)
        side = torch.cuda.Stream(device=self.device)
        stop = threading.Event()
        rows_all = order // self.files.cpi

        def produce():
            try:
                torch.cuda.set_device(self.device)
                for b in range(nb):
                    if stop.is_set():
                        return
                    s = b % nslots
                    rows = rows_all[b * B:(b + 1) * B]
                    if copied[s] is not None:
                        copied[s].synchronize()                    # pinned[s] is free again
                    np.take(src, rows, axis=0, out=pinned[s].numpy()[:len(rows)], mode="clip")   # unbuffered; rows are valid by construction
                    with torch.cuda.stream(side):
                        if released[s] is not None:
                            side.wait_event(released[s])           # staged[s] no longer being read
                        staged[s][:len(rows)].copy_(pinned[s][:len(rows)], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    copied[s] = ev
                    q.put((b, s, len(rows), ev))
                q.put(None)
            except BaseException as e:      # surface producer failures in the consumer
                q.put(e)

        th = threading.Thread(target=produce, name="scnattn-batch-stager", daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                b, s, n, ev = item
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)
                sel = None
                if self.augment is None:
                    imgs = self._images(staged[s], None, n, None, None)
                else:                                             # the draw needs the sample ids before the gather
                    sel = torch.from_numpy(order[b * B:b * B + n]).to(self.device, non_blocking=True)
                    # the grey table of this staged batch: the same values as the resident table's rows
                    grey = mean_grey(staged[s][:n]) if self.augment.contrast != 0.0 else None
                    imgs = self._images(staged[s][:n], None, n, sel, grey)
                rel = torch.cuda.Event()
                rel.record(cur)
                released[s] = rel
                if sel is None:
                    sel = torch.from_numpy(order[b * B:b * B + n]).to(self.device, non_blocking=True)
                yield self._tuple(imgs, sel)
        finally:
            stop.set()
            while th.is_alive():            # unblock a producer waiting on a full queue
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)
            torch.cuda.current_stream(self.device).synchronize()
