"""Writes tests/golden/J4_jpeg_optimize.npz and J4_jpeg_optimize_vectors.txt: what PIL's encoder (libjpeg-turbo) writes with
optimize=True, for the optimised Huffman tables of clips.jpeg_encode_host(optimize=True) (DESIGN.md "JPEG files out,
optimised tables").

    python tests/golden/make_jpeg_optimize_golden.py

Sources: make_jpeg_golden.smooth_image at 8 x 8, 17 x 33 and 24 x 40 with `subsampling` 0 (4:4:4) and at 1 x 1, 16 x 16 and
32 x 48 with `subsampling` 2 (4:2:0) -- the sizes at which libjpeg codes the blocks this project codes: at 4:2:0 it writes a
dummy block (the previous DC, no AC) where a luma block of an MCU lies wholly outside the frame, this project the DCT of the
replicated edge, so the symbol counts differ there and only the host definition is the yardstick.  Qualities 30, 75, 95 and
100, without restart markers and with restart_marker_rows=1.  One 224 x 224 4:4:4 frame (smooth_image(224, 224, 7000) plus
Gaussian noise of sigma 8, quality 95) whose chroma AC table has unlimited code lengths up to 17 and so runs the length
limiting of T.81 K.2; it was found by searching sizes, noise levels and qualities for max(clips.jpeg_code_lengths) > 16.
Keys: `names`; frame_<name> uint8 (H, W, 3); file_<name> uint8 (PIL's bytes); `limit`: the name of the limited frame.
The histogram-to-table vectors: vec_counts int64 (N, 256), vec_bits (N, 16), vec_total (N,), vec_values (N, 256) as
clips.jpeg_optimal_table gives them (values padded with zeros): the four histograms of every file above, random counts,
equal counts, one symbol, 256 symbols, Fibonacci-like counts to depths past 16 and past 32, counts near 2^31, all zeros.  The
text file holds the same for tools/jpeg_entropy_opt_check.cpp: N, then per vector 256 counts, 16 length counts, the number of
values, the values.

The recipe asserts, for every file: the four tables of the definition equal PIL's; the scan bytes equal PIL's; and, on these
sizes and on the dummy-block sizes 8 x 8, 17 x 33 and 48 x 72 at 4:2:0, that PIL decodes every jpeg_encode_host(optimize=True)
file to the bytes it decodes the standard-table file to.  Recorded with PIL 12.2 (libjpeg-turbo); the tests read the files and
need no PIL.
"""
import io
import os
import sys

import numpy as np
import torch
from PIL import Image, ImageFile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import istvt_pkg  # noqa: E402
from make_jpeg_golden import smooth_image  # noqa: E402

CASES = ((0, '444', ((8, 8), (17, 33), (24, 40))), (2, '420', ((1, 1), (16, 16), (32, 48))))
QUALITIES = (30, 75, 95, 100)
DUMMY_BLOCK_SIZES = ((8, 8), (17, 33), (48, 72))
ImageFile.MAXBLOCK = 1 << 22                # PIL's buffer for an optimize=True file: large frames fail with the default


def pil_file(img: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).copy()


def limit_frame() -> np.ndarray:
    base = smooth_image(224, 224, 7000).astype(np.float64)
    return np.clip(np.round(base + np.random.default_rng(0).normal(0, 8.0, base.shape)), 0, 255).astype(np.uint8)


def histograms(clips, x, q, sub, ri):
    """clips.jpeg_symbol_counts of the coefficients jpeg_encode_host codes"""
    step = clips.JPEG_SUBSAMPLINGS[sub]
    qt, zz = clips.jpeg_quant_tables(q), torch.tensor(clips.JPEG_ZIGZAG)
    coef = []
    for c, p in enumerate(clips._jpeg_planes_in(x[None], step)):
        k = clips._jpeg_quantise(p, qt[min(c, 1)][None])[0].permute(0, 2, 1, 3)
        coef.append(k.reshape(k.shape[0], k.shape[1], 64)[:, :, zz].tolist())
    my, mx = -(-x.shape[0] // (8 * step)), -(-x.shape[1] // (8 * step))
    return clips.jpeg_symbol_counts(coef, [(step, step), (1, 1), (1, 1)], my, mx, clips.jpeg_restart_interval(ri, x.shape[1], sub))


def synthetic_counts():
    g = np.random.default_rng(29)
    out = []
    for i in range(12):                                           # random
        c = np.zeros(256, dtype=np.int64)
        idx = g.choice(256, int(g.integers(1, 257)), replace=False)
        c[idx] = g.integers(1, 1 << int(g.integers(1, 25)), len(idx))
        out.append(c.tolist())
    for k in (2, 3, 100, 255, 256):                               # all equal
        out.append([7 if s < k else 0 for s in range(256)])
    for s in (0, 0xF0, 255):                                      # one symbol
        out.append([1000 if t == s else 0 for t in range(256)])
    out.append([1] * 256)                                         # 256 symbols
    out.append(g.integers(1, 1 << 20, 256).tolist())
    for depth in (17, 24, 33, 40, 47):                            # Fibonacci-like: lengths past 16 and past 32
        c, a, b = [0] * 256, 1, 1
        for k in range(depth):
            c[(k * 5 + depth) & 255] = min(a, 0xFFFFFFFF)
            a, b = b, a + b
        out.append(c)
    for top in (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):              # near 2^31
        out.append([top - (s % 3) if s % 5 == 0 else 0 for s in range(256)])
        out.append([top] * 256)
    out.append([0] * 256)
    return out


def main():
    istvt_pkg.load()
    from istvt_amd import clips
    out, names, vectors = {}, [], []

    def record(name, img, sub, q, rows, **kw):
        x = torch.from_numpy(img)
        ri = 'row' if rows else 0
        pil = pil_file(img, quality=q, subsampling={'444': 0, '420': 2}[sub], optimize=True, **kw)
        ours, std = clips.jpeg_encode_host(x, q, sub, ri, optimize=True), clips.jpeg_encode_host(x, q, sub, ri)
        hp, ho = clips.jpeg_parse(pil), clips.jpeg_parse(ours)
        assert hp.huffman == ho.huffman, name
        assert hp.restart_interval == ho.restart_interval, name
        assert [hp.data[b:e] for b, e in hp.segments] == [ho.data[b:e] for b, e in ho.segments], name
        assert np.array_equal(pil_decode(ours), pil_decode(std)), name
        names.append(name)
        out['frame_' + name] = img
        out['file_' + name] = np.frombuffer(pil, dtype=np.uint8)
        vectors.extend(histograms(clips, x, q, sub, ri))

    for pil_sub, sub, sizes in CASES:
        for h, w in sizes:
            img = smooth_image(h, w, 100 * h + w)
            for q in QUALITIES:
                record('%dx%d_s%d_q%d' % (h, w, pil_sub, q), img, sub, q, False)
                record('%dx%d_s%d_q%d_rr1' % (h, w, pil_sub, q), img, sub, q, True, restart_marker_rows=1)
    img = limit_frame()
    lengths = [max(clips.jpeg_code_lengths(c)[0]) for c in histograms(clips, torch.from_numpy(img), 95, '444', 0)]
    assert max(lengths) > 16, lengths
    record('limit_224x224_s0_q95', img, '444', 95, False)
    assert len(out['file_limit_224x224_s0_q95']) < 65536
    out['limit'] = np.array('limit_224x224_s0_q95')
    out['names'] = np.array(names)
    for h, w in DUMMY_BLOCK_SIZES:                                # other counts than libjpeg's, the same pixels
        x = torch.from_numpy(smooth_image(h, w, 100 * h + w))
        for q in QUALITIES:
            for ri in (0, 'row'):
                a, b = clips.jpeg_encode_host(x, q, '420', ri, optimize=True), clips.jpeg_encode_host(x, q, '420', ri)
                assert np.array_equal(pil_decode(a), pil_decode(b)) and len(a) < len(b), (h, w, q, ri)

    vectors.extend(synthetic_counts())
    tables = [clips.jpeg_optimal_table(c) for c in vectors]
    out['vec_counts'] = np.array(vectors, dtype=np.int64)
    out['vec_bits'] = np.array([t[0] for t in tables], dtype=np.uint8)
    out['vec_total'] = np.array([len(t[1]) for t in tables], dtype=np.int32)
    out['vec_values'] = np.array([list(t[1]) + [0] * (256 - len(t[1])) for t in tables], dtype=np.uint8)
    with open(os.path.join(HERE, 'J4_jpeg_optimize_vectors.txt'), 'w') as fh:
        fh.write('%d\n' % len(vectors))
        for c, (bits, values) in zip(vectors, tables):
            fh.write(' '.join(map(str, c)) + '\n' + ' '.join(map(str, bits)) + '\n')
            fh.write(' '.join(map(str, (len(values),) + tuple(values))) + '\n')
    path = os.path.join(HERE, 'J4_jpeg_optimize.npz')
    np.savez_compressed(path, **out)
    print('%s: %d files, %d vectors, %d bytes' % (path, len(names), len(vectors), os.path.getsize(path)))


if __name__ == '__main__':
    main()
