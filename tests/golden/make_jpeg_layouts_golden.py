"""Writes tests/golden/J3_jpeg_layouts.npz: baseline JPEG files in the 4:2:2 and greyscale layouts as PIL's encoder
(libjpeg-turbo) writes them, with what PIL's decoder makes of each.  The scheme of make_jpeg_files_golden.py (J2).

    python tests/golden/make_jpeg_layouts_golden.py [directory to write the sound and damaged files into as .jpg]

Sources: make_jpeg_golden.smooth_image at 1 x 1, 8 x 8, 16 x 16, 17 x 33, 24 x 40, 33 x 70, 48 x 48, 9 x 15 (two MCU rows
where 4:2:0 has one) and 8 x 17 (an odd width whose last chroma column lies in the second MCU); each as 4:2:2 (`subsampling`
1) and as greyscale (channel 1 saved as mode L); qualities 30, 75, 95 and 100 with default tables and, at quality 75,
optimize=True, restart_marker_blocks=1 and restart_marker_rows=1; one 40 x 56 uniform-noise image at quality 50 and 100 in
both layouts; grey_f22_24x40_q75, the greyscale 24 x 40 quality-75 file with the sampling factors of its SOF0 set to 2x2,
which PIL decodes to the pixels of the 1x1 file.  Keys: `names` (the sound files, in order), file_<name> uint8 (the bytes)
and rgb_<name> uint8 (H, W, 3) (PIL's decode, .convert('RGB')).

Three damaged copies of 24x40_422_q75: damaged422_cut (cut in the middle of its scan; status 1), damaged422_code and
damaged422_run (one byte of the scan replaced so that clips.jpeg_decode_host(..., layouts='all') reports status 2 and 3; the
first such byte and value in file order); `damaged` lists their names, damaged_status their statuses, damaged_edit (byte,
value) per file (the cut: length, 0).

The recipe also checks what the tests do not need PIL for: that the definition gives PIL's bytes on every sound file, and
that PIL decodes every clips.jpeg_encode_layout_host file to the bytes of clips.jpeg_decode_host.  Recorded with PIL 12.2
(libjpeg-turbo); tests/test_jpeg_layouts_cpu.py and tests/test_jpeg_layouts_gpu.py read the file and need no PIL.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import istvt_pkg  # noqa: E402
from make_jpeg_files_golden import VARIANTS, pil_decode, pil_file  # noqa: E402
from make_jpeg_golden import smooth_image  # noqa: E402

SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (24, 40), (33, 70), (48, 48), (9, 15), (8, 17))


def layout_file(img: np.ndarray, layout: str, **kw) -> bytes:
    return pil_file(img, subsampling=1, **kw) if layout == '422' else pil_file(img[..., 1].copy(), **kw)


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
        for layout in ('422', 'grey'):
            for tag, kw in VARIANTS:
                sound('%dx%d_%s_%s' % (h, w, layout, tag), layout_file(src, layout, **kw))
    noise = np.random.default_rng(4056).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    for layout in ('422', 'grey'):
        for q in (50, 100):
            sound('noise40x56_%s_q%d' % (layout, q), layout_file(noise, layout, quality=q))
    patched = bytearray(out['file_24x40_grey_q75'].tobytes())
    sof = bytes(patched).index(b'\xff\xc0')
    assert patched[sof + 9] == 1 and patched[sof + 11] == 0x11
    patched[sof + 11] = 0x22
    sound('grey_f22_24x40_q75', bytes(patched))
    assert np.array_equal(out['rgb_grey_f22_24x40_q75'], out['rgb_24x40_grey_q75'])
    out['names'] = np.array(names)

    base = bytes(out['file_24x40_422_q75'])
    hd = clips.jpeg_parse(base, 'all')
    lo, hi = hd.segments[0][0], hd.segments[-1][1]
    cut = (lo + hi) // 2
    damaged = {'damaged422_cut': (base[:cut], 1, (cut, 0))}
    for name, want in (('damaged422_code', 2), ('damaged422_run', 3)):
        for at in range(lo, hi):
            for value in range(256):
                if value in (0xFF, base[at]) or (at > lo and base[at - 1] == 0xFF):
                    continue                              # no new marker, no new stuffed pair
                data = base[:at] + bytes([value]) + base[at + 1:]
                try:
                    status = clips.jpeg_decode_host(data, True, 'all')[1]
                except ValueError:
                    continue
                if status == want:
                    damaged[name] = (data, want, (at, value))
                    break
            if name in damaged:
                break
    assert len(damaged) == 3, sorted(damaged)
    assert clips.jpeg_decode_host(damaged['damaged422_cut'][0], True, 'all')[1] == 1
    out['damaged'] = np.array(sorted(damaged))
    out['damaged_status'] = np.array([damaged[k][1] for k in sorted(damaged)], dtype=np.int32)
    out['damaged_edit'] = np.array([damaged[k][2] for k in sorted(damaged)], dtype=np.int32)
    for k, v in damaged.items():
        out['file_' + k] = np.frombuffer(v[0], dtype=np.uint8)

    # the host definition on every sound file, and what the tests leave to this recipe
    for name in names:
        got, status = clips.jpeg_decode_host(bytes(out['file_' + name]), True, layouts='all')
        assert status == 0 and np.array_equal(got.numpy(), out['rgb_' + name]), name
    for h, w in ((16, 16), (17, 33), (24, 40)):
        x = torch.from_numpy(smooth_image(h, w, 100 * h + w))
        for layout in ('422', 'grey'):
            for q in (30, 90):
                for ri in (0, 2):
                    data = clips.jpeg_encode_layout_host(x, q, layout, ri)
                    got, status = clips.jpeg_decode_host(data, True, layouts='all')
                    assert status == 0 and np.array_equal(pil_decode(data), got.numpy()), (h, w, layout, q, ri)

    path = os.path.join(HERE, 'J3_jpeg_layouts.npz')
    np.savez_compressed(path, **out)
    print('%s: %d sound files, %d arrays, %d bytes' % (path, len(names), len(out), os.path.getsize(path)))
    if len(sys.argv) > 1:
        os.makedirs(sys.argv[1], exist_ok=True)
        for name in names + sorted(damaged):
            with open(os.path.join(sys.argv[1], name + '.jpg'), 'wb') as fh:
                fh.write(bytes(out['file_' + name]))


if __name__ == '__main__':
    main()
