"""Writes tests/golden/J2_jpeg_files.npz: baseline JPEG files as PIL's encoder (libjpeg-turbo) writes them, with what PIL's
decoder makes of each.

    python tests/golden/make_jpeg_files_golden.py [directory to write the sound and damaged files into as .jpg]

Sources: make_jpeg_golden.smooth_image at 1 x 1, 8 x 8, 16 x 16, 17 x 33, 24 x 40, 33 x 70 and 48 x 48, `subsampling` 2 (4:2:0)
and 0 (4:4:4); qualities 30, 75, 95 and 100 with default tables and, at quality 75, optimize=True, restart_marker_blocks=1
and restart_marker_rows=1; one 40 x 56 uniform-noise image at quality 50 and 100.  Keys: `names` (the sound files, in
order), file_<name> uint8 (the bytes) and rgb_<name> uint8 (H, W, 3) (PIL's decode).

Three damaged copies of 24x40_s2_q75: damaged_cut (cut in the middle of its scan; status 1), damaged_code and damaged_run
(one byte of the scan replaced so that clips.jpeg_decode_host reports status 2 and 3; the first such byte and value in file
order); `damaged` lists their names, damaged_status their statuses, damaged_edit (byte, value) per file (the cut: length, 0).
Three files PIL can write and the decoder refuses: refused_progressive, refused_422, refused_grey.

The recipe also checks what the tests do not need PIL for: that PIL decodes every clips.jpeg_encode_host file to the bytes of
clips.jpeg_roundtrip_host, and that PIL's default Huffman tables are clips.JPEG_STD_HUFFMAN.  Recorded with PIL 12.2
(libjpeg-turbo); tests/test_jpeg_decode_cpu.py and tests/test_jpeg_decode_gpu.py read the file and need no PIL.
"""
import io
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import istvt_pkg  # noqa: E402
from make_jpeg_golden import smooth_image  # noqa: E402

SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (24, 40), (33, 70), (48, 48))
VARIANTS = (('q30', dict(quality=30)), ('q75', dict(quality=75)), ('q95', dict(quality=95)), ('q100', dict(quality=100)),
            ('q75_opt', dict(quality=75, optimize=True)), ('q75_rb1', dict(quality=75, restart_marker_blocks=1)),
            ('q75_rr1', dict(quality=75, restart_marker_rows=1)))


def pil_file(img: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).copy()


def main():
    istvt_pkg.load()
    from istvt_amd import clips
    out, names = {}, []

    def sound(name, data):
        names.append(name)
        out['file_' + name] = np.frombuffer(data, dtype=np.uint8)
        out['rgb_' + name] = pil_decode(data)

    for h, w in SIZES:
        src = smooth_image(h, w, 100 * h + w)
        for sub in (2, 0):
            for tag, kw in VARIANTS:
                sound('%dx%d_s%d_%s' % (h, w, sub, tag), pil_file(src, subsampling=sub, **kw))
    noise = np.random.default_rng(4056).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    for sub in (2, 0):
        for q in (50, 100):
            sound('noise40x56_s%d_q%d' % (sub, q), pil_file(noise, subsampling=sub, quality=q))
    out['names'] = np.array(names)

    base = bytes(out['file_24x40_s2_q75'])
    hd = clips.jpeg_parse(base)
    lo, hi = hd.segments[0][0], hd.segments[-1][1]
    cut = (lo + hi) // 2
    damaged = {'damaged_cut': (base[:cut], 1, (cut, 0))}
    for name, want in (('damaged_code', 2), ('damaged_run', 3)):
        for at in range(lo, hi):
            for value in range(256):
                if value in (0xFF, base[at]) or (at > lo and base[at - 1] == 0xFF):
                    continue                              # no new marker, no new stuffed pair
                data = base[:at] + bytes([value]) + base[at + 1:]
                try:
                    status = clips.jpeg_decode_host(data, True)[1]
                except ValueError:
                    continue
                if status == want:
                    damaged[name] = (data, want, (at, value))
                    break
            if name in damaged:
                break
    assert len(damaged) == 3, sorted(damaged)
    assert clips.jpeg_decode_host(damaged['damaged_cut'][0], True)[1] == 1
    out['damaged'] = np.array(sorted(damaged))
    out['damaged_status'] = np.array([damaged[k][1] for k in sorted(damaged)], dtype=np.int32)
    out['damaged_edit'] = np.array([damaged[k][2] for k in sorted(damaged)], dtype=np.int32)
    for k, v in damaged.items():
        out['file_' + k] = np.frombuffer(v[0], dtype=np.uint8)

    src = smooth_image(24, 40, 2440)
    out['file_refused_progressive'] = np.frombuffer(pil_file(src, quality=75, progressive=True), dtype=np.uint8)
    out['file_refused_422'] = np.frombuffer(pil_file(src, quality=75, subsampling=1), dtype=np.uint8)
    out['file_refused_grey'] = np.frombuffer(pil_file(src[..., 0].copy(), quality=75), dtype=np.uint8)

    # the host definition on every sound file, and what the tests leave to this recipe
    for name in names:
        got, status = clips.jpeg_decode_host(bytes(out['file_' + name]), True)
        assert status == 0 and np.array_equal(got.numpy(), out['rgb_' + name]), name
    std = clips.JPEG_STD_HUFFMAN
    assert clips.jpeg_parse(bytes(out['file_16x16_s2_q75'])).huffman[:2] == ((std[(0, 0)], std[(1, 0)]), (std[(0, 1)], std[(1, 1)]))
    for h, w in ((16, 16), (17, 33), (24, 40)):
        x = torch.from_numpy(smooth_image(h, w, 100 * h + w))
        for s in ('420', '444'):
            for q in (30, 90):
                for ri in (0, 2):
                    data = clips.jpeg_encode_host(x, q, s, ri)
                    assert np.array_equal(pil_decode(data), clips.jpeg_roundtrip_host(x[None], q, s)[0].numpy()), (h, w, s, q, ri)

    path = os.path.join(HERE, 'J2_jpeg_files.npz')
    np.savez_compressed(path, **out)
    print('%s: %d sound files, %d arrays, %d bytes' % (path, len(names), len(out), os.path.getsize(path)))
    if len(sys.argv) > 1:
        os.makedirs(sys.argv[1], exist_ok=True)
        for name in names + sorted(damaged):
            with open(os.path.join(sys.argv[1], name + '.jpg'), 'wb') as fh:
                fh.write(bytes(out['file_' + name]))


if __name__ == '__main__':
    main()
