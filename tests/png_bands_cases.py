"""Files for the tests of the banded PNG decoder (test_png_bands_cpu.py, test_png_bands_gpu.py; no tests in here): our own
indexed files at the sizes where a band edge can go wrong, files zlib wrote with a flush at every band edge and a hand-made
index, indexes that are malformed (and so ignored) and indexes that are well-formed and lie, and the vectors of
tools/png_bands_check.cpp written from the definition."""
import os
import zlib

import numpy as np

import png_encode_cases as C
import png_streams as P

# (H, W, channels, band_rows): H of 1, below R, equal to R, one above a multiple of R, and 130 (the unfilter's groups of 64 rows
# and the bands disagree); grey, RGB and RGBA; band_rows 1, 8, 16 and 64; the widest is 111
MIXED = ((1, 70, 1, 16), (5, 33, 3, 8), (16, 21, 4, 16), (17, 9, 3, 8), (33, 40, 1, 16), (130, 9, 4, 64), (130, 11, 3, 1),
         (40, 111, 3, 8), (64, 5, 1, 64), (65, 67, 4, 16), (9, 3, 1, 1), (129, 2, 3, 64))


def chunk(kind, body):
    return len(body).to_bytes(4, 'big') + kind + body + zlib.crc32(kind + body).to_bytes(4, 'big')


def splice(data, extra, at=33):
    """whole chunks `extra` put into a file behind its IHDR (at=33), or at another chunk boundary"""
    return data[:at] + extra + data[at:]


def index_body(R, offsets, nb=None):
    return b''.join(int(v).to_bytes(4, 'big') for v in [R, len(offsets) - 1 if nb is None else nb] + list(offsets))


def mixed_files(clips):
    """[(name, indexed file of ours)]"""
    return [('%dx%dx%d_r%d' % (h, w, ch, R), clips.png_encode_banded_host(P.pattern(h, w, ch, 40 + i), R, 'adaptive', index=True))
            for i, (h, w, ch, R) in enumerate(MIXED)]


def ignored_index_file(clips):
    """a file of ours whose chunk has a wrong last offset: the index is ignored and the file is one band"""
    frame = P.pattern(20, 31, 3, 77)
    plain, bands, _ = clips.png_encode_banded_host(frame, 8, 'adaptive', return_bands=True)
    off = [b for b, _ in bands] + [bands[-1][1] + 1]
    return splice(plain, chunk(b'baND', index_body(8, off)))


def banded_stream(rows, R, level=6, strategy=0, edge=zlib.Z_FULL_FLUSH, inner=None, shared=True, final=True):
    """rows uint8 (H, stride) -> (the zlib stream, [off[0] .. off[nb]]): zlib's own blocks with a flush of kind `edge` behind
    every band but the last (an empty stored block on a byte boundary; Z_FULL_FLUSH also forgets the window), inner: a flush
    of that kind in the middle of every band (several blocks per band, and a stored block that does not end the band).
    shared=False: a compressor of its own per band, each finished (BFINAL in every band).  final=False: the last band is
    flushed like the others, so no block has BFINAL."""
    H = rows.shape[0]
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    stream, off = bytearray(b'\x78\x01'), []
    for r0 in range(0, H, R):
        off.append(len(stream))
        band = rows[r0:r0 + R].tobytes()
        last = r0 + R >= H
        if not shared:
            z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        if inner is not None:
            stream += z.compress(band[:len(band) // 2]) + z.flush(inner)
            band = band[len(band) // 2:]
        stream += z.compress(band)
        stream += z.flush(zlib.Z_FINISH if (last and final) or not shared else edge)
    off.append(len(stream))
    return bytes(stream + zlib.adler32(rows.tobytes()).to_bytes(4, 'big')), off


def wrap(clips, rows, ch, stream, R, off):
    H, W = rows.shape[0], (rows.shape[1] - 1) // ch
    return clips.png_wrap(H, W, {1: 0, 3: 2, 4: 6}[ch], stream, extra=chunk(b'baND', index_body(R, off)))


def periodic(H, W, ch, seed):
    """every row is the first: with filter 0 a compressor finds each row in the row above, at distance 1 + W ch"""
    row = np.random.default_rng(seed).integers(0, 256, (1, W, ch), dtype=np.uint8)
    x = np.repeat(row, H, 0)
    return x[:, :, 0] if ch == 1 else x


def flush_files(clips):
    """[(name, file)]: Z_FULL_FLUSH at every band edge and a hand-made index; the five stream kinds of png_streams.KINDS
    (stored, fixed and dynamic blocks), a flush inside every band too (several blocks per band), long matches inside a band
    (periodic rows)"""
    out = []
    for i, ((level, strategy), (H, W, ch, R)) in enumerate(zip(P.KINDS + ((6, 0), (9, 0)),
                                                               ((37, 50, 3, 8), (20, 45, 1, 16), (66, 30, 4, 16), (33, 64, 3, 4),
                                                                (19, 27, 1, 5), (48, 100, 3, 16), (130, 20, 4, 64)))):
        frame = periodic(H, W, ch, i) if i >= 5 else P.pattern(H, W, ch, 60 + i)
        rows = clips.png_filter_rows_host(frame, 0 if i >= 5 else 'adaptive')
        stream, off = banded_stream(rows, R, level, strategy, inner=zlib.Z_SYNC_FLUSH if i % 2 == 0 else zlib.Z_FULL_FLUSH)
        out.append(('flush_%d_%dx%dx%d_r%d_l%d_s%d' % (i, H, W, ch, R, level, strategy), wrap(clips, rows, ch, stream, R, off)))
    return out


def lying_files(clips):
    """[(name, file, the status the issue names or None)]: indexes that png_parse takes and that do not say where the bands
    are, and bands that are damaged.  36 x 25 RGB in bands of 8 rows unless said otherwise."""
    H, W, ch, R = 36, 25, 3, 8
    frame = P.pattern(H, W, ch, 91)
    rows = clips.png_filter_rows_host(frame, 'adaptive')
    out = []
    stream, off = banded_stream(rows, R)
    out.append(('offset_plus_1', wrap(clips, rows, ch, stream, R, off[:2] + [off[2] + 1] + off[3:]), None))
    prows = clips.png_filter_rows_host(periodic(H, W, ch, 5), 0)
    stream, off = banded_stream(prows, R, edge=zlib.Z_SYNC_FLUSH)
    out.append(('sync_flush', wrap(clips, prows, ch, stream, R, off), 4))
    stream, off = banded_stream(rows, R, shared=False)
    out.append(('bfinal_in_a_middle_band', wrap(clips, rows, ch, stream, R, off), 7))
    stream, off = banded_stream(rows, R, final=False)
    out.append(('bfinal_missing_in_the_last_band', wrap(clips, rows, ch, stream, R, off), 1))
    stream, off = banded_stream(rows, 9)                          # four bands of 9 rows, and an index that says 4 x 10 (the last: 6)
    out.append(('band_rows_wrong', wrap(clips, rows, ch, stream, 10, off), 5))
    stream, off = banded_stream(rows, R, level=9)
    bad = bytearray(stream)
    bad[off[1] + 9] ^= 0x10                                        # a bit inside the second band's first block
    out.append(('bit_flipped_in_a_band', wrap(clips, rows, ch, bytes(bad), R, off), None))
    stream, off = banded_stream(rows, R)
    cut = stream[:off[2] - 7] + stream[off[2]:]                    # the second band loses its last coded bytes; the index follows
    out.append(('band_cut_short', wrap(clips, rows, ch, cut, R, off[:2] + [v - 7 for v in off[2:]]), None))
    return out


def pil_files(golden_dir, k=3):
    d = os.path.join(golden_dir, 'png')
    names = np.load(os.path.join(d, 'pixels.npz'))['names'].tolist()
    return [(n, open(os.path.join(d, n + '.png'), 'rb').read()) for n in names[:k]]


def write_vectors(path, clips, files):
    """the vectors of tools/png_bands_check.cpp from the definition, clips.png_inflate_bands_host's rules band by band: every
    band of every file of `files` [(name, file)] at the offset mod 4 it has in a batch -> [(band name, status)]"""
    done = []
    with open(path, 'w') as fh:
        for name, f in files:
            hd = clips.png_parse(f)
            table = clips.png_band_table(hd)
            for k, (_, begin, end, _, nbytes) in enumerate(table):
                middle = k < len(table) - 1
                out, status = clips._png_inflate(hd.data[begin:end], nbytes, middle=middle)
                fh.write('%s_b%d %d %d %d %d %s %s\n' % (name, k, status, int(middle), begin % 4, nbytes, hd.data[begin:end].hex() or '-',
                                                        bytes(out).hex() if status == 0 and out else '-'))
                done.append(('%s_b%d' % (name, k), status))
    return done


def device_files(clips, golden_dir):
    """every file the GPU tests decode by bands, as [(name, file)]: what the host check decodes first"""
    return (mixed_files(clips) + [('ignored_index', ignored_index_file(clips))] + pil_files(golden_dir) + flush_files(clips)
            + [(n, f) for n, f, _ in lying_files(clips)] + encoder_files(clips))


ENCODER = ((1, 16), (17, 16), (40, 8), (33, 1))                   # (H, band_rows) of the device encoder's test, W = 29


def encoder_frames(ch):
    return [(H, R, np.stack([C.smooth(H, 29, ch, 10 * ch + j) for j in range(3)]).reshape(3, H, 29, ch)) for H, R in ENCODER]


def encoder_files(clips):
    out = []
    for ch in C.CHANNELS:
        for H, R, frames in encoder_frames(ch):
            out += [('enc_c%d_%d_r%d_%d' % (ch, H, R, j), f) for j, f in enumerate(clips.png_encode_files_host(frames, R, index=True))]
    return out
