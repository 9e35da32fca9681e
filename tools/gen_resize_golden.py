"""Writes tests/golden/resize_pillow.npz: inputs and the outputs of `PIL.Image.resize((OW, OH), resample=BILINEAR)` --
what the reference's `scipy.misc.imresize(img, (OH, OW))` computes (inference.py:37, utils/dataset.py:372) -- for the
small shapes of tests/resize_refs.py, a random and a 0/255 checkerboard input each, RGB and grey.  Needs Pillow; the
committed file was written with Pillow 12.2.0.  The 257x255 source is left out to keep the file small (it is compared
with Pillow directly where Pillow is installed).

    python tools/gen_resize_golden.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resize_refs as RR  # noqa: E402

GOLDEN_MAX_SIDE = 64      # larger sources stay out of the file


def main():
    out = {"pillow_version": np.asarray(PIL.__version__)}
    k = 0
    for src, dst in RR.SMALL_SHAPES:
        if max(src) > GOLDEN_MAX_SIDE and src[0] * src[1] > 4096:
            continue
        for grey in (False, True):
            for img in (RR.random_image(src, 100 + k, grey), RR.checker_image(src, grey)):
                res = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), resample=2))
                out["in_%02d" % k], out["out_%02d" % k] = img, res
                k += 1
    path = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes -> %s" % (k, os.path.getsize(path), path))


if __name__ == "__main__":
    main()
