"""Writes tests/golden/J1_jpeg_pil.npz: what PIL's JPEG codec (libjpeg-turbo) hands back for seeded synthetic images.

    python tests/golden/make_jpeg_golden.py

Sources: smooth sinusoids plus Gaussian noise of sigma 12 (many coefficients survive the quantisation), 16 x 16, 24 x 40,
17 x 33 and 48 x 48.  Round trips: subsampling=2 (4:2:0) at q in {30, 50, 75, 90} and at q - 10 and q + 10, subsampling=0
(4:4:4) at q = 75 and at 65 and 85.  Keys: src_{H}x{W} and pil_{H}x{W}_s{subsampling}_q{q}, uint8 (H, W, 3).  Recorded with
PIL 12.2 (libjpeg-turbo); tests/test_jpeg_cpu.py reads the file and needs no PIL.
"""
import io
import os

import numpy as np
from PIL import Image

SIZES = ((16, 16), (24, 40), (17, 33), (48, 48))
QUALITIES = {2: (30, 50, 75, 90), 0: (75,)}
SIGMA = 12.0


def smooth_image(h: int, w: int, seed: int) -> np.ndarray:
    """uint8 (h, w, 3): a sinusoid of its own frequency and phase per channel around 128, plus N(0, SIGMA) noise"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, SIGMA, (h, w, 3))), 0, 255).astype(np.uint8)


def pil_roundtrip(img: np.ndarray, q: int, subsampling: int) -> np.ndarray:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=q, subsampling=subsampling)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))


def main():
    out = {}
    for h, w in SIZES:
        src = smooth_image(h, w, 100 * h + w)
        out['src_%dx%d' % (h, w)] = src
        for sub, qs in QUALITIES.items():
            for q in sorted({v + d for v in qs for d in (-10, 0, 10)}):
                out['pil_%dx%d_s%d_q%d' % (h, w, sub, q)] = pil_roundtrip(src, q, sub)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'J1_jpeg_pil.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))


if __name__ == '__main__':
    main()
