"""Writes tests/golden/lanczos_pillow.npz: inputs and the outputs of `PIL.Image.resize((OW, OH), resample=LANCZOS)` --
the photograph of the reference's utils/vizualize.py:26 -- for the small shapes of tests/overlay_refs.py, a random and a
0/255 checkerboard input each, RGB and grey.  Needs Pillow; the committed file was written with Pillow 12.2.0.  The
257x255 and the 336x336 shapes stay out to keep the file small (they are compared with Pillow directly where Pillow is
installed).

    python tools/gen_lanczos_golden.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlay_refs as OR  # noqa: E402
import resize_refs as RR  # noqa: E402


def main():
    out = {"pillow_version": np.asarray(PIL.__version__)}
    k = 0
    for src, dst in OR.GOLDEN_SHAPES:
        for grey in (False, True):
            for img in (RR.random_image(src, 200 + k, grey), RR.checker_image(src, grey)):
                res = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), resample=Image.LANCZOS))
                out["in_%02d" % k], out["out_%02d" % k] = img, res
                k += 1
    path = os.path.join(ROOT, "tests", "golden", "lanczos_pillow.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes -> %s" % (k, os.path.getsize(path), path))


if __name__ == "__main__":
    main()
