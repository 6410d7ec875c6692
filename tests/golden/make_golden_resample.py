#!/usr/bin/env python3
"""Fixture G22: Pillow's own `Image.resize(wh, Image.LANCZOS)` of the sources of tests/resample_ref.py (`cases()`: the shape
list, RGB and RGBA, noise and a ramp with alpha 0 / 255 / mixed, and an (F = 2) stack).  The sources are an integer hash and
are not stored: the fixture keeps their CRC-32 and Pillow's outputs.
Fixture g22_resample_edges: the same for `edge_cases()`, the shapes past one x-block of the device kernels and the 3000-frame
stack whose rows pass the grid's 65535; of the stack it keeps the CRC-32 of Pillow's output instead of its 1.9 MB.
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


def pillow(cases):
    from PIL import Image
    outs, crcs = {}, {}
    for name, src, wh in cases:
        mode = "RGB" if src.shape[3] == 3 else "RGBA"
        outs[name] = np.stack([np.asarray(Image.fromarray(f, mode).resize(wh, Image.LANCZOS)) for f in src])
        crcs[name] = zlib.crc32(src.tobytes())
    return outs, crcs


def main():
    import PIL
    outs, crcs = pillow(RR.cases())
    save("g22_resample", dict(pillow=PIL.__version__, source_crc32=crcs), {}, outs)
    outs, crcs = pillow(RR.edge_cases())
    stack = outs.pop(RR.EDGE_STACK)
    save("g22_resample_edges", dict(pillow=PIL.__version__, source_crc32=crcs,
                                    output_crc32={RR.EDGE_STACK: zlib.crc32(stack.tobytes())}), {}, outs)


if __name__ == "__main__":
    main()
