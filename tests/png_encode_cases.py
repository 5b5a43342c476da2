"""Frames for the PNG writer's tests (test_png_encode_cpu.py, test_png_encode_gpu.py): the shapes, filters, runs and tables at
which a rule of clips.png_encode_banded_host can go wrong, as (name, frame uint8, band_rows, filters), and the vectors of
tools/png_deflate_check.cpp written from the definition."""
import numpy as np

CHANNELS = (1, 3, 4)
FILTERS = (0, 1, 2, 3, 4, 'adaptive')
RUN_RESTS = (1, 2, 3, 257, 258, 259, 260, 261, 516, 517)      # what is left of a run behind its leading literal


def noise(H, W, ch, seed):
    x = np.random.default_rng(seed).integers(0, 256, (H, W, ch), dtype=np.uint8)
    return x[:, :, 0] if ch == 1 else x


def smooth(H, W, ch, seed):
    """a gradient with a little noise: every filter type wins some row"""
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * yy + 2 * xx + 40 * c) % 256 for c in range(ch)], 2)
    x = np.clip(base + np.random.default_rng(seed).integers(-2, 3, base.shape), 0, 255).astype(np.uint8)
    return x[:, :, 0] if ch == 1 else x


def spread(counts, values):
    """a row in which value k stands counts[k] times and no two neighbours are equal (the largest count is at most half)"""
    seq = [v for c, v in sorted(zip(counts, values), reverse=True) for _ in range(c)]
    out = [0] * len(seq)
    half = (len(seq) + 1) // 2
    out[0::2], out[1::2] = seq[:half], seq[half:]
    return np.array(out, np.uint8)[None, :]


def fibonacci_row(k=17):
    """the filter byte 0 and the end-of-block once each, k values 2, 3, 5, 8, ... times: an unlimited Huffman code has k + 1 bits"""
    fib = [2, 3]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    return spread(fib, [3 + 7 * i for i in range(k)])


def cl_limit_lengths():
    """literal/length code lengths of symbols 0..256 whose code-length code would be 8 bits deep: 144 symbols of 13 bits in
    groups of three (a run of three is sent as three lengths, not as a repeat), between them 13 of 4 bits, 1 of 5, 8 of 6, 1 of 9,
    3 of 10, 1 of 11, 34 of 12 and zero runs of 36, 8 and 8, no two equal ones side by side.  The Kraft sum is 1; the
    code-length symbols are then used 144, 34, 13, 8, 3, 2, 1, 1, 1, 1, 1 times (the distance code's 1 among them)."""
    seps = [4] * 13 + [5] + [6] * 8 + [9] + [10] * 3 + [11] + [12] * 34 + [(0, 36), (0, 8), (0, 8)]
    kinds = {}
    for v in seps:
        kinds.setdefault(v, []).append(v)
    pools, order = sorted(kinds.values(), key=len, reverse=True), []
    while any(pools):                          # dealt round-robin by value: equal separators never meet in the first rounds
        order += [p.pop() for p in pools if p]
    lens, at, double = [], 0, len(order) - 47  # 47 gaps between 48 groups; the first `double` gaps take two separators
    for g in range(48):
        lens += [13] * 3
        for v in order[at:at + (0 if g == 47 else 2 if g < double else 1)]:
            lens += [0] * v[1] if isinstance(v, tuple) else [v]
        at += 0 if g == 47 else 2 if g < double else 1
    return lens


def cl_limit_row():
    """one grey row of 8190 bytes for filter 0 whose literal/length code is cl_limit_lengths(): byte v stands 2^(13 - length)
    times (the filter byte is the one 0, the end-of-block the 8192nd count), no two neighbours equal"""
    lens = cl_limit_lengths()
    values = [v for v in range(1, 256) if lens[v]]
    return spread([1 << (13 - lens[v]) for v in values], values)


def tie_frame():
    """two rows on which filter types tie: a constant first row (types 0 and 2 see the same bytes; 1, 3 and 4 tie at a lower
    sum: 1 wins), and a copy of the row above (2 and 4 give all zeros: 2 wins)"""
    return np.array([[9] * 6, [9] * 6], np.uint8)


def mixed_frame(ch, W=23, seed=8):
    """seven rows built so that the adaptive rule picks a known type on most: noise; a copy of the row above (2); bytes near zero
    under noise (0); the mean of left and above (3); a ramp (1); noise; the Paeth predictor itself (4)"""
    g = np.random.default_rng(seed)
    n = W * ch
    rows = [g.integers(0, 256, n)]
    rows.append(rows[0].copy())
    rows.append(g.integers(-1, 2, n) & 255)
    up, cur = rows[-1], np.zeros(n, np.int64)
    for i in range(n):
        cur[i] = ((cur[i - ch] if i >= ch else 0) + up[i]) >> 1
    rows.append(cur)
    rows.append((40 + 3 * (np.arange(n) // ch) + 50 * (np.arange(n) % ch)) & 255)
    rows.append(g.integers(0, 256, n))
    up, cur = rows[-1], np.zeros(n, np.int64)
    cur[:ch] = 100                             # a first pixel of its own, or every pixel would copy the row above
    for i in range(ch, n):
        a, b, c = cur[i - ch], up[i], up[i - ch]
        pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
        cur[i] = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
    rows.append(cur)
    x = np.stack(rows).astype(np.uint8).reshape(7, W, ch)
    return x[:, :, 0] if ch == 1 else x


def shape_cases():
    out = []
    for ch in CHANNELS:
        out.append(('1x1_c%d' % ch, noise(1, 1, ch, 1), 16, 'adaptive'))
        out.append(('5x3_c%d' % ch, noise(5, 3, ch, 2), 16, 'adaptive'))
        out.append(('17x9_c%d' % ch, smooth(17, 9, ch, 3), 16, 'adaptive'))
        for R in (1, 8, 16, 64):
            out.append(('33x40_c%d_r%d' % (ch, R), smooth(33, 40, ch, 4), R, 'adaptive'))
    out.append(('1x300_zeros', np.zeros((1, 300), np.uint8), 16, 0))
    return out


def filter_cases():
    out = [('filter_%s_c%d' % (f, ch), smooth(9, 11, ch, 5 + ch), 4, f) for ch in CHANNELS for f in FILTERS]
    out.append(('filter_tie', tie_frame(), 16, 'adaptive'))
    out += [('filter_mixed_c%d' % ch, mixed_frame(ch), 4, 'adaptive') for ch in CHANNELS]
    return out


def run_cases():
    """constant grey rows with filter 0: the filter byte 0, then a run of rest + 1 bytes of 7; and a run that crosses a row
    boundary inside a band (rows of zeros: the filter byte joins the run)"""
    out = [('run_%d' % m, np.full((1, m + 1), 7, np.uint8), 16, 0) for m in RUN_RESTS]
    out.append(('run_rows', np.zeros((3, 100), np.uint8), 16, 0))
    out.append(('run_rows_bands', np.zeros((5, 130), np.uint8), 2, 0))
    return out


def table_cases():
    two = np.random.default_rng(7).integers(0, 2, (4, 64), dtype=np.uint8) * 200 + 5
    return [('uniform_noise', noise(16, 255, 1, 6), 16, 0), ('two_values', two, 16, 0), ('fibonacci', fibonacci_row(), 16, 0),
            ('cl_limit', cl_limit_row(), 16, 0)]


def all_cases():
    return shape_cases() + filter_cases() + run_cases() + table_cases()


def band_rows_of(clips, frame, R, filters):
    rows = clips.png_filter_rows_host(frame, filters)
    return [rows[r0:r0 + R].tobytes() for r0 in range(0, rows.shape[0], R)]


def write_vectors(path, clips):
    """-> the names written: every band of every case (at the byte offset mod 4 it has in its file), and every small case as a
    whole file"""
    done = []
    with open(path, 'w') as fh:
        for name, frame, R, filters in all_cases():
            data, bands, _ = clips.png_encode_banded_host(frame, R, filters, return_bands=True)
            body = data[41:]
            rows = clips.png_filter_rows_host(frame, filters)
            parts = band_rows_of(clips, frame, R, filters)
            for k, ((b, e), raw) in enumerate(zip(bands, parts)):
                fh.write('band %s_b%d %d %d %s %s\n' % (name, k, int(k == len(bands) - 1), (41 + b) % 4, raw.hex(), body[b:e].hex()))
                done.append('%s_b%d' % (name, k))
            if rows.size <= 4096:
                bpp = 1 if frame.ndim == 2 else frame.shape[2]
                fh.write('file %s %d %d %d %d %s %s\n' % (name, frame.shape[0], frame.shape[1], bpp, R, rows.tobytes().hex(), data.hex()))
                done.append(name)
    return done
