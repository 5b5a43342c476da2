"""Writes the PNG fixtures beside this file: files as PIL's encoder (zlib) writes them, and pixels.npz with what PIL's decoder
makes of each, for tests/test_png_cpu.py and tests/test_png_gpu.py (which need no PIL).

    python tests/golden/png/make_png_golden.py

Sources: tests/png_streams.pattern(h, w, channels, seed) at 40 x 33 (grey, 'L'), 33 x 40 (RGB) and 29 x 64 (RGBA), seeds 1..3.
Each is written five times: compress_level 0, 1, 6 and 9, and optimize=True.  PIL picks the row filters itself (its adaptive
choice mixes the types).  pixels.npz: `names`, and rgb_<name> uint8 (H, W, 3) = Image.open(file).convert('RGB') (grey replicated,
alpha dropped).  The recipe asserts that clips.png_decode_host gives those pixels.  Recorded with PIL 12.2 (zlib 1.3).
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import istvt_pkg                                                   # noqa: E402
import png_streams                                                 # noqa: E402

istvt_pkg.load()
from istvt_amd import clips                                        # noqa: E402

SOURCES = (('grey', 40, 33, 1, 'L'), ('rgb', 33, 40, 3, 'RGB'), ('rgba', 29, 64, 4, 'RGBA'))
SETTINGS = (('l0', dict(compress_level=0)), ('l1', dict(compress_level=1)), ('l6', dict(compress_level=6)),
            ('l9', dict(compress_level=9)), ('opt', dict(optimize=True)))


def main():
    names, pixels = [], {}
    for seed, (kind, h, w, ch, mode) in enumerate(SOURCES, 1):
        image = Image.fromarray(png_streams.pattern(h, w, ch, seed), mode)
        for tag, kw in SETTINGS:
            name = '%s_%dx%d_%s' % (kind, h, w, tag)
            buf = io.BytesIO()
            image.save(buf, 'PNG', **kw)
            data = buf.getvalue()
            rgb = np.array(Image.open(io.BytesIO(data)).convert('RGB'))
            got, status = clips.png_decode_host(data, return_status=True)
            assert status == 0 and np.array_equal(got.numpy(), rgb), name
            with open(os.path.join(HERE, name + '.png'), 'wb') as fh:
                fh.write(data)
            names.append(name)
            pixels['rgb_' + name] = rgb
    np.savez_compressed(os.path.join(HERE, 'pixels.npz'), names=np.array(names), **pixels)
    print('%d files' % len(names))


if __name__ == '__main__':
    main()
