#!/usr/bin/env python3
"""Fixture G22: Pillow's own `Image.resize(wh, Image.LANCZOS)` of the sources of tests/resample_ref.py (`cases()`: the shape
list, RGB and RGBA, noise and a ramp with alpha 0 / 255 / mixed, and an (F = 2) stack).  The sources are an integer hash and
are not stored: the fixture keeps their CRC-32 and Pillow's outputs.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resample.py"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

from make_golden import save  # noqa: E402
from tests import resample_ref as RR  # noqa: E402


def main():
    import PIL
    from PIL import Image
    outs, crcs = {}, {}
    for name, src, wh in RR.cases():
        mode = "RGB" if src.shape[3] == 3 else "RGBA"
        outs[name] = np.stack([np.asarray(Image.fromarray(f, mode).resize(wh, Image.LANCZOS)) for f in src])
        crcs[name] = zlib.crc32(src.tobytes())
    save("g22_resample", dict(pillow=PIL.__version__, source_crc32=crcs), {}, outs)


if __name__ == "__main__":
    main()
