"""Files, batches, banks and vectors for the tests of PNG bands that stand alone (test_png_alone_cpu.py,
test_png_alone_gpu.py; no tests in here): flagged files of ours at the sizes where a band edge can go wrong, files whose flag
lies, a damaged band under the flag, the doctored band rows, and the vectors of tools/png_alone_check.cpp written from the
definition.  Only files and rows that program has walked go to a device: the GPU tests take them from here and nowhere else."""
import zlib

import numpy as np
import torch

import png_bands_cases as B
import png_streams as P

FLAG = 0x80000000
_CACHE = {}

# (H, W, channels, band_rows) of the flagged files of the mixed batch: R of 1, 5, 8, 16, 64 and 100; H no multiple of R; H < R,
# a single band; 130 rows in bands of 100, a band longer than the 64 rows a wave holds at once; H = 1; W of 1, 31 and 70;
# grey, RGB and RGBA
ALONE = ((130, 9, 3, 100), (20, 31, 3, 8), (5, 9, 1, 16), (1, 70, 4, 16), (64, 70, 4, 1), (33, 1, 1, 5), (17, 31, 3, 5),
         (130, 7, 4, 64), (40, 12, 1, 16), (9, 33, 3, 64))
DEVICE_WRITER = ((20, 31, 3, 8), (5, 9, 1, 16), (64, 70, 4, 1))   # (H, W, channels, band_rows) of the device writer's test


def set_flag(data):
    """a file of ours with an index: bit 31 of the chunk's R word set by hand, the chunk's CRC-32 redone"""
    length = int.from_bytes(data[33:37], 'big')
    assert data[37:41] == b'baND'
    body = bytearray(data[41:41 + length])
    body[0] |= 0x80
    return data[:33] + B.chunk(b'baND', bytes(body)) + data[33 + 12 + length:]


def alone_files(clips):
    """[(name, flagged file of ours)]"""
    if 'alone' not in _CACHE:
        _CACHE['alone'] = [('%dx%dx%d_r%d' % (h, w, ch, R),
                            clips.png_encode_banded_host(P.pattern(h, w, ch, 140 + i), R, 'adaptive', index=True, alone=True))
                           for i, (h, w, ch, R) in enumerate(ALONE)]
    return _CACHE['alone']


def _flagged(clips, rows, ch, R, **how):
    """rows with their filter bytes -> a flagged file whose bands zlib wrote with a flush at every band edge"""
    stream, off = B.banded_stream(rows, R, **how)
    return B.wrap(clips, rows, ch, stream, R | FLAG, off), stream, off


def lying_files(clips):
    """[(name, file, status)]: 36 x 25 RGB in bands of 8 rows.  Files written with a fixed filter 2, 3 and 4 and index=True
    whose flag is set by hand (status 10); the same lie under a damaged band (the band's status) and under a filter byte 5
    (status 6); a file whose row 0 alone has type 2 (sound: PNG defines row 0 with a zero row above)."""
    if 'lying' in _CACHE:
        return _CACHE['lying']
    H, W, ch, R = 36, 25, 3, 8
    frame = P.pattern(H, W, ch, 191)
    out = [('fixed_%d_flagged' % ft, set_flag(clips.png_encode_banded_host(frame, R, ft, index=True)), 10) for ft in (2, 3, 4)]
    up = clips.png_filter_rows_host(frame, 2)
    f, stream, off = _flagged(clips, up, ch, R, level=9)
    bad = bytearray(stream)
    bad[off[1] + 9] ^= 0x10                                        # a bit inside the second band's first block
    broken = B.wrap(clips, up, ch, bytes(bad), R | FLAG, off)
    out.append(('damaged_band_and_lying_row', broken, clips.png_decode_bands_host(broken, return_status=True)[1]))
    five = clips.png_filter_rows_host(frame, 4).copy()
    five[3, 0] = 5
    out.append(('filter_5_and_lying_row', _flagged(clips, five, ch, R)[0], 6))
    first = clips.png_filter_rows_host(frame, 'adaptive', R).copy()
    assert first[0, 0] in (0, 1)
    first[0] = clips.png_filter_rows_host(frame, 2)[0]             # row 0 as Up against the zero row
    out.append(('row_0_alone_has_type_2', _flagged(clips, first, ch, R)[0], 0))
    assert out[3][2] not in (0, 6, 10)
    _CACHE['lying'] = out
    return out


def damaged_file(clips):
    """a true flagged file whose second band has a flipped bit"""
    rows = clips.png_filter_rows_host(P.pattern(36, 25, 3, 192), 'adaptive', 8)
    _, stream, off = _flagged(clips, rows, 3, 8, level=9)
    bad = bytearray(stream)
    bad[off[1] + 9] ^= 0x10
    return B.wrap(clips, rows, 3, bytes(bad), 8 | FLAG, off)


def mixed_files(clips, golden_dir):
    """[(name, file)] of the one mixed batch: the flagged files, an indexed file without the flag, a PIL file without an
    index, the lying files and a damaged band"""
    plain = clips.png_encode_banded_host(P.pattern(37, 29, 3, 150), 8, 'adaptive', index=True)
    return (alone_files(clips) + [('indexed_without_the_flag', plain)] + B.pil_files(golden_dir, 1)
            + [(n, f) for n, f, _ in lying_files(clips)] + [('damaged_band', damaged_file(clips))])


def reference(clips, files):
    """[(frame, status)] of png_decode_alone_host: computed once per list, shared, never changed"""
    key = ('ref',) + tuple(n for n, _ in files)
    if key not in _CACHE:
        _CACHE[key] = [clips.png_decode_alone_host(f, return_status=True) for _, f in files]
    return _CACHE[key]


def bank_files(clips):
    """the files of the alone bank: png_bank_cases' index shapes run over them"""
    plain = clips.png_encode_banded_host(P.pattern(37, 29, 3, 150), 8, 'adaptive', index=True)
    return [f for _, f in alone_files(clips)] + [plain, clips.png_encode_host(P.pattern(23, 31, 3, 7), level=6)]


def alone_bank(clips, first_byte=0):
    key = ('bank', first_byte)
    if key not in _CACHE:
        _CACHE[key] = clips.png_bank(bank_files(clips), first_byte=first_byte, alone=True)
    return _CACHE[key]


def doctored(clips, bank):
    """[(name, the doctored bank, the place whose band rows were changed)]: a wrong `out`, an `out_bytes` that is no multiple
    of the stride, and a wrong count; each gives status 9 at that place and leaves every other place as it was"""
    import png_bank_cases as K
    images, bands = bank.images, bank.bands
    a = next(i for i, r in enumerate(images.tolist()) if r[9] & 1 and 3 <= r[8] <= 16)
    first, stride = int(images[a, 7]), 1 + int(images[a, 1]) * int(images[a, 3])
    out = []
    t = bands.clone()
    t[first + 1, 3] += stride                                      # band 1 starts a row late
    out.append(('wrong_out', K.with_rows(clips, bank, bands=t), a))
    t = bands.clone()
    t[first + 1, 4] -= 1
    out.append(('out_bytes_no_multiple_of_the_stride', K.with_rows(clips, bank, bands=t), a))
    t = images.clone()
    t[a, 8] -= 1
    out.append(('wrong_count', K.with_rows(clips, bank, images=t), a))
    return out


def file_line(clips, name, H, W, bpp, rows, waves, raw, statuses):
    """an F line of tools/png_alone_check.cpp from the band rows, the filtered rows and the band statuses of one flagged file:
    the status, R and the waves' rows are the definition's (clips._png_alone_band_rows, clips._png_alone_rows)"""
    stride = 1 + W * bpp
    R = clips._png_alone_band_rows(H, stride, rows)
    status = 9 if R == 0 else clips._png_alone_rows(raw, statuses, H, W, bpp, R)[1]
    spans = '-' if R == 0 else ','.join('%d:%d' % (k * R, min(H, (k + 1) * R)) for k in range(len(rows)))
    csv = lambda v: ','.join(str(int(x)) for x in v)
    filters = [raw[r * stride] for r in range(H)]
    return 'F %s %d %d %d %d %d %s %s %s %d %d %s' % (name, H, W, bpp, len(rows), waves, csv(sum(rows, [])), csv(filters), csv(statuses),
                                                       status, R, spans), status


def write_vectors(path, clips, golden_dir):
    """Every flagged file the GPU tests hand to a device, as the vectors of tools/png_alone_check.cpp: the mixed batch's, the
    bank's at its band_max waves, and the doctored banks' -> (lines, the set of statuses)"""
    lines, seen = [], set()
    for name, f in mixed_files(clips, golden_dir):
        hd = clips.png_parse(f)
        if not hd.alone:
            continue
        raw, statuses = clips.png_inflate_bands_host(hd)
        line, status = file_line(clips, name, hd.H, hd.W, hd.bpp, clips.png_band_table(hd), len(statuses), raw, statuses)
        assert status == clips.png_decode_alone_host(hd, return_status=True)[1], name
        lines.append(line)
        seen.add(status)
    bank = alone_bank(clips)
    for tag, b, places in [('bank', bank, range(bank.n))] + [('doctored_' + n, d, [p]) for n, d, p in doctored(clips, bank)]:
        for i in places:
            im = b.images[i].tolist()
            if not im[9] & 1:
                continue
            hd = bank.headers[i]
            raw, statuses = clips.png_inflate_bands_host(hd)
            rows = [b.bands[im[7] + k].tolist() for k in range(im[8])]
            line, status = file_line(clips, '%s_f%d' % (tag, i), im[0], im[1], im[3], rows, b.band_max, raw, statuses[:im[8]])
            assert status == int(clips.png_bank_decode_host(b, [i])[2][0]), (tag, i)
            lines.append(line)
            seen.add(status)
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return lines, seen
