"""Writes tests/golden/J5_jpeg_encode_layouts.npz and J5_jpeg_encode_layouts_scans.txt: the files of
clips.jpeg_encode_host(layout='422' | 'grey') (DESIGN.md "JPEG files out, 4:2:2 and greyscale"), checked against what PIL's
encoder (libjpeg-turbo) writes for the same frames.

    python tests/golden/make_jpeg_encode_layouts_golden.py

Sources: make_jpeg_golden.smooth_image(h, w, 100 h + w) at the sizes below; PIL writes 4:2:2 with subsampling=1 and greyscale
from Image.convert('L'), whose luma is the Y of this project's colour-in.  Qualities 30, 75, 95 and 100, standard and
optimised tables, without restart markers and with restart_marker_rows=1.

The recipe asserts, for every such file:
  - at the sizes in PIL_EQUAL the scan bytes of the definition are PIL's, and with optimize=True so are the tables of the
    same class and id (PIL writes only those of the components it has);
  - at the other sizes (4:2:2 with 0 < W % 16 <= 8: libjpeg writes a dummy block -- the previous DC, no AC -- where the second
    luma block of the last MCU lies wholly outside the frame, this project the DCT of the replicated edge) PIL decodes the
    definition's file to the pixels of its own file;
  - PIL decodes every optimised file to the pixels of the standard file, the greyscale ones with their two empty id-1 tables
    included.

Recorded (RECORDED_QUALITIES only, to stay small): `names`; frame_<h>x<w> uint8 (H, W, 3); file_<name> uint8, the definition's
bytes, name = <h>x<w>_<layout>_q<quality>[_rr1][_opt]; `pil_equal`: the names whose scans are PIL's.  The text file is for
tools/jpeg_entropy_layout_check.cpp: the number of cases, then per case layout code (1: 4:2:2, 2: greyscale), MCU columns, MCU
rows, restart interval in MCUs, optimised (0 / 1), the number of blocks, 64 coefficients per block in the order of the
device's scratch (Y row by row of the padded plane, then Cb, then Cr; zig-zag), the number of scan bytes and the scan (all
restart intervals, markers and EOI included).  Recorded with PIL 12.2 (libjpeg-turbo); the tests read the files and need no PIL.
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

SIZES = {'422': ((1, 1), (8, 8), (8, 16), (9, 47), (16, 32), (17, 33), (23, 31), (24, 40), (33, 70), (40, 25)),
         'grey': ((1, 1), (8, 8), (8, 16), (9, 47), (16, 32), (17, 33), (23, 31), (24, 40), (33, 70), (40, 25))}
PIL_EQUAL = {'422': ((1, 1), (8, 16), (9, 47), (16, 32), (23, 31), (40, 25)), 'grey': SIZES['grey']}
QUALITIES = (30, 75, 95, 100)
RECORDED_QUALITIES = (75, 100)
SCAN_SIZES = ((9, 47), (17, 33))             # the cases of the text file: these sizes at quality 75
ImageFile.MAXBLOCK = 1 << 22


def pil_file(img: np.ndarray, layout: str, **kw) -> bytes:
    buf = io.BytesIO()
    if layout == 'grey':
        Image.fromarray(img).convert('L').save(buf, 'JPEG', **kw)
    else:
        Image.fromarray(img).save(buf, 'JPEG', subsampling=1, **kw)
    return buf.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).copy()


def scratch_blocks(clips, data: bytes):
    """the coefficients of a file in the order of the device's scratch, zig-zag within a block"""
    hd = clips.jpeg_parse(data, layouts='all')
    coef = clips._jpeg_coefficients(hd)[0]
    zz = torch.tensor(clips.JPEG_ZIGZAG)
    return hd, [blk for plane in coef for blk in plane.permute(0, 2, 1, 3).reshape(-1, 64)[:, zz].tolist()]


def main():
    istvt_pkg.load()
    from istvt_amd import clips
    out, names, pil_equal, cases = {}, [], [], []
    for layout in ('422', 'grey'):
        for h, w in SIZES[layout]:
            img = smooth_image(h, w, 100 * h + w)
            x = torch.from_numpy(img)
            out['frame_%dx%d' % (h, w)] = img
            for q in QUALITIES:
                for rows in (False, True):
                    kw = dict(quality=q, **({'restart_marker_rows': 1} if rows else {}))
                    ri = 'row' if rows else 0
                    std = clips.jpeg_encode_host(x, q, restart_interval=ri, layout=layout)
                    assert std == clips.jpeg_encode_layout_host(x, q, layout, clips.jpeg_restart_interval(ri, w, layout=layout))
                    for optimize in (False, True):
                        name = '%dx%d_%s_q%d%s%s' % (h, w, layout, q, '_rr1' if rows else '', '_opt' if optimize else '')
                        ours = clips.jpeg_encode_host(x, q, restart_interval=ri, optimize=True, layout=layout) if optimize else std
                        pil = pil_file(img, layout, optimize=optimize, **kw)
                        hp, ho = clips.jpeg_parse(pil, layouts='all'), clips.jpeg_parse(ours, layouts='all')
                        assert hp.restart_interval == ho.restart_interval and hp.layout == ho.layout == layout, name
                        if (h, w) in PIL_EQUAL[layout]:
                            assert [hp.data[b:e] for b, e in hp.segments] == [ho.data[b:e] for b, e in ho.segments], name
                            assert hp.huffman == ho.huffman, name      # per component the file has
                            pil_equal.append(name)
                        else:
                            assert np.array_equal(pil_decode(ours), pil_decode(pil)), name
                        assert np.array_equal(pil_decode(ours), pil_decode(std)) and len(ours) <= len(std), name
                        if q in RECORDED_QUALITIES:
                            names.append(name)
                            out['file_' + name] = np.frombuffer(ours, dtype=np.uint8)
                        if q == 75 and (h, w) in SCAN_SIZES:
                            hd, blocks = scratch_blocks(clips, ours)
                            scan = hd.data[hd.segments[0][0]:]
                            cases.append((clips.JPEG_LAYOUT_CODES[layout], hd.mcus[1], hd.mcus[0], hd.restart_interval,
                                          int(optimize), blocks, scan))
    out['names'] = np.array(names)
    out['pil_equal'] = np.array([n for n in pil_equal if n in set(names)])
    with open(os.path.join(HERE, 'J5_jpeg_encode_layouts_scans.txt'), 'w') as fh:
        fh.write('%d\n' % len(cases))
        for code, mx, my, ri, optimize, blocks, scan in cases:
            fh.write('%d %d %d %d %d %d\n' % (code, mx, my, ri, optimize, len(blocks)))
            for blk in blocks:
                fh.write(' '.join(map(str, blk)) + '\n')
            fh.write('%d\n' % len(scan) + ' '.join(map(str, scan)) + '\n')
    path = os.path.join(HERE, 'J5_jpeg_encode_layouts.npz')
    np.savez_compressed(path, **out)
    print('%s: %d files (%d with PIL\'s scan), %d scan cases, %d bytes' % (path, len(names), len(out['pil_equal']), len(cases),
                                                                          os.path.getsize(path)))


if __name__ == '__main__':
    main()
