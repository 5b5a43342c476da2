"""PNG files out (DESIGN.md "PNG files out") without a device: the definition clips.png_encode_banded_host read back four ways
on the shapes, filters, runs and tables of tests/png_encode_cases.py; its token, table and size rules; the plain build of
tools/png_deflate_check.cpp on the vectors the definition writes; the ABI row and the refusals that need no device."""
import ctypes
import io
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_encode_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def _four_ways(clips, frame, R, filters):
    """-> (file, bands, filter types) after PIL, zlib, png_decode_host and every band inflated alone have read it back"""
    from PIL import Image
    data, bands, types = clips.png_encode_banded_host(frame, R, filters, return_bands=True)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frame)
    rows = clips.png_filter_rows_host(frame, filters)
    assert data[:8] == clips.PNG_SIGNATURE and data[37:41] == b'IDAT' and data.count(b'IDAT') == 1
    body = data[41:41 + int.from_bytes(data[33:37], 'big')]
    assert body[:2] == b'\x78\x01' and zlib.decompress(body) == rows.tobytes()          # and so the Adler-32
    got, status = clips.png_decode_host(data, return_status=True)
    want = np.repeat(frame[:, :, None], 3, 2) if frame.ndim == 2 else frame[:, :, :3]
    assert status == 0 and np.array_equal(got.numpy(), want)
    assert len(bands) == -(-frame.shape[0] // R) and bands[0][0] == 2 and bands[-1][1] == len(body) - 4
    for k, (b, e) in enumerate(bands):
        z = zlib.decompressobj(-15)
        alone = z.decompress(body[b:e])
        assert alone == rows[k * R:(k + 1) * R].tobytes() and z.eof == (k == len(bands) - 1) and z.unused_data == b''
        assert body[e - 4:e] == b'\x00\x00\xff\xff' and (k == 0 or bands[k - 1][1] == b)
    assert types == rows[:, 0].tolist()
    return data, bands, types


@pytest.mark.parametrize('case', C.shape_cases() + C.filter_cases(), ids=lambda c: c[0])
def test_shapes_and_filters_read_back_four_ways(clips, case):
    name, frame, R, filters = case
    data, bands, types = _four_ways(clips, frame, R, filters)
    if filters != 'adaptive':
        assert types == [filters] * frame.shape[0]
    if frame.ndim == 2:                       # (H, W, 1) is the same file
        assert clips.png_encode_banded_host(frame[:, :, None], R, filters) == data


def test_adaptive_filter_and_its_ties(clips):
    data, bands, types = _four_ways(clips, C.tie_frame(), 16, 'adaptive')
    assert types == [1, 2]                    # row 0: types 1, 3 and 4 tie below 0 and 2; row 1: 2 and 4 give all zeros
    rows = [clips.png_filter_rows_host(C.tie_frame(), f) for f in range(5)]
    cost = [[int(np.minimum(r[y, 1:].astype(int), 256 - r[y, 1:].astype(int)).sum()) for r in rows] for y in range(2)]
    assert cost[0][1] == cost[0][4] < cost[0][0] == cost[0][2] and cost[0][3] >= cost[0][1]
    assert cost[1][2] == cost[1][4] == 0 < min(cost[1][0], cost[1][1], cost[1][3])
    for ch in C.CHANNELS:                     # the choice is the per-row minimum, and every type is chosen
        frame = C.mixed_frame(ch)
        types = clips.png_encode_banded_host(frame, 4, 'adaptive', return_bands=True)[2]
        assert types[1:5] == [2, 0, 3, 1] and (ch == 1 or types[6] == 4)
        all_rows = np.stack([clips.png_filter_rows_host(frame, f)[:, 1:].astype(int) for f in range(5)])
        costs = np.minimum(all_rows, 256 - all_rows).sum(axis=2)
        assert types == np.argmin(costs, axis=0).tolist()


def _greedy(band):
    """the token rule restated left to right: a literal, then as many 258s as fit, then the rest as one match or literals"""
    out, i = [], 0
    while i < len(band):
        out.append(band[i])
        j = i + 1
        while j < len(band) and band[j] == band[i]:
            j += 1
        rest = j - i - 1
        while rest >= 258:
            out.append(-258)
            rest -= 258
        out += [-rest] if rest >= 3 else [band[i]] * rest
        i = j
    return out


@pytest.mark.parametrize('case', C.run_cases(), ids=lambda c: c[0])
def test_runs(clips, case):
    name, frame, R, filters = case
    _four_ways(clips, frame, R, filters)
    for band in C.band_rows_of(clips, frame, R, filters):
        assert clips._png_band_tokens(band) == _greedy(band)
    if name.startswith('run_') and name[4:].isdigit():
        m = int(name[4:])
        want = {1: [0, 7, 7], 2: [0, 7, 7, 7], 3: [0, 7, -3], 257: [0, 7, -257], 258: [0, 7, -258], 259: [0, 7, -258, 7],
                260: [0, 7, -258, 7, 7], 261: [0, 7, -258, -3], 516: [0, 7, -258, -258], 517: [0, 7, -258, -258, 7]}[m]
        assert clips._png_band_tokens(C.band_rows_of(clips, frame, R, filters)[0]) == want
    if name == 'run_rows':                    # 3 rows of 101 zeros are one run: the filter bytes join it
        assert clips._png_band_tokens(C.band_rows_of(clips, frame, R, filters)[0]) == [0, -258, -44]
    if name == 'run_rows_bands':              # and no run leaves its band: 2 rows of 131, 2 rows, 1 row
        assert [clips._png_band_tokens(b) for b in C.band_rows_of(clips, frame, R, filters)] == [[0, -258, -3], [0, -258, -3], [0, -130]]


def _kraft(lens):
    return sum(2.0 ** -v for v in lens if v)


def test_tables(clips):
    for name, frame, R, filters in C.table_cases():
        _four_ways(clips, frame, R, filters)
        tokens = clips._png_band_tokens(C.band_rows_of(clips, frame, R, filters)[0])
        lit, hlit, cltok, cl, hclen = clips._png_band_tables(tokens)
        assert _kraft(lit) == 1.0 and _kraft(cl) == 1.0 and clips._png_code(lit) is not None and clips._png_code(cl) is not None
        assert max(lit) <= 15 and max(cl) <= 7 and lit[256] > 0
        if name == 'uniform_noise':
            assert min(tokens) >= 0 and all(lit[:256]) and hlit == 257
        if name == 'two_values':
            assert sorted(set(t for t in tokens if t >= 0)) == [0, 5, 205] and hlit >= 257
        if name == 'fibonacci':
            # 17 values 2, 3, 5, ... times, the filter byte and the end-of-block once: 19 symbols, an unlimited code of 18 bits
            counts = [0] * 286
            for t in tokens:
                counts[t] += 1
            counts[256] = 1
            assert min(tokens) >= 0 and sorted(c for c in counts if c)[:6] == [1, 1, 2, 3, 5, 8] and sum(1 for c in counts if c) == 19
            assert max(clips._png_code_lengths(counts, 64)) == 18 and max(lit) == 15
        if name == 'cl_limit':
            # the literal/length code is the planned one, and its lengths use the code-length symbols 144, 34, 13, 8, 3, 2, 1, ...
            # times: an unlimited code-length code has 8 bits, so the 7-bit limit decides what the header carries
            assert min(tokens) >= 0 and lit[:257] == C.cl_limit_lengths() and hlit == 257
            clcounts = [0] * 19
            for s, _, _ in cltok:
                clcounts[s] += 1
            assert clcounts == [0, 1, 0, 0, 13, 1, 8, 0, 0, 1, 3, 1, 34, 144, 0, 0, 0, 2, 1]
            assert max(clips._png_code_lengths(clcounts, 64)) == 8 > 7 and max(cl) == 7
            assert cl != clips._png_code_lengths(clcounts, 64)
    # equal counts: the larger symbol is merged first, so it is never the shorter code
    assert clips._png_code_lengths([1, 1, 1], 15) == [1, 2, 2]
    assert clips._png_code_lengths([5, 0, 5, 5, 5, 0], 15) == [2, 0, 2, 2, 2, 0]
    assert clips._png_code_lengths([0, 9, 0], 15) == [0, 1, 0] and clips._png_code_lengths([0, 0], 15) == [0, 0]


def test_code_length_code_limit(clips):
    """The code-length code's limit of 7 bits on the construction itself: counts 1, 1, 2, 3, ... over 10 of its 19 symbols give
    an unlimited code of 9 bits.  End to end the limit is reached by the band `cl_limit` of png_encode_cases.table_cases (an
    unlimited code of 8 bits), which test_tables, the host tool's vectors and the GPU byte comparison run.  Then the greedy
    rule that sends the lengths."""
    counts = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55] + [0] * 9
    assert max(clips._png_code_lengths(counts, 15)) == 9
    lens = clips._png_code_lengths(counts, 7)
    assert max(lens) == 7 and _kraft(lens) == 1.0 and clips._png_code(lens) is not None
    assert lens == [7, 7, 7, 7, 6, 6, 4, 3, 2, 1] + [0] * 9
    # the greedy rule for sending lengths
    T = clips._png_length_tokens
    assert T([0] * 2) == [(0, 0, 0)] * 2 and T([0] * 3) == [(17, 0, 3)] and T([0] * 10) == [(17, 7, 3)] and T([0] * 11) == [(18, 0, 7)]
    assert T([0] * 138) == [(18, 127, 7)] and T([0] * 140) == [(18, 127, 7), (0, 0, 0), (0, 0, 0)] and T([0] * 149) == [(18, 127, 7), (18, 0, 7)]
    assert T([5] * 3) == [(5, 0, 0)] * 3 and T([5] * 4) == [(5, 0, 0), (16, 0, 2)] and T([5] * 7) == [(5, 0, 0), (16, 3, 2)]
    assert T([5] * 9) == [(5, 0, 0), (16, 3, 2), (5, 0, 0), (5, 0, 0)] and T([5] * 10) == [(5, 0, 0), (16, 3, 2), (16, 0, 2)]
    assert T([3, 0, 0, 0, 3]) == [(3, 0, 0), (17, 0, 3), (3, 0, 0)]


def test_size_bound(clips):
    for H, W in ((1, 1), (5, 3), (64, 64)):
        for ch in C.CHANNELS:
            for R in (1, 16):
                frame = C.noise(H, W, ch, 30 + ch)
                raw = H * (1 + W * ch)
                bands = -(-H // min(R, H))
                bound = clips.png_encoded_bound(H, W, ch, R)
                for filters in (0, 'adaptive'):
                    assert len(clips.png_encode_banded_host(frame, R, filters)) <= bound, (H, W, ch, R)
                # raw + raw / 8 + a constant per band (the largest header, the end-of-block, the stored block) and per file
                assert bound <= raw + raw / 8 + bands * ((clips.PNG_BAND_HEADER_BITS + 15 + 3 + 7) / 8 + 4 + 1) + clips.PNG_CONTAINER_BYTES
    assert clips.PNG_CONTAINER_BYTES == 63 and clips.PNG_BAND_HEADER_BITS == 17 + 57 + 7 * 287
    for name, frame, R, filters in C.table_cases():          # and where the length limits act
        bpp = 1 if frame.ndim == 2 else frame.shape[2]
        assert len(clips.png_encode_banded_host(frame, R, filters)) <= clips.png_encoded_bound(frame.shape[0], frame.shape[1], bpp, R), name


def test_files_of_a_batch_and_refusals(clips):
    frames = np.stack([C.smooth(9, 11, 3, i) for i in range(4)])
    want = [clips.png_encode_banded_host(f, 4, 'adaptive') for f in frames]
    assert clips.png_encode_files_host(frames, 4) == want == clips.png_encode_files_host(torch.from_numpy(frames).reshape(2, 2, 9, 11, 3), 4)
    assert clips.png_encode_banded_host(torch.from_numpy(frames[0]), 4) == want[0]
    assert clips.png_encode_banded_host(frames[0], 9) == clips.png_encode_banded_host(frames[0], 64)     # one band either way
    with pytest.raises(ValueError, match=r'png_encode_banded_host: a uint8 \(H, W\), \(H, W, 1\), \(H, W, 3\) or \(H, W, 4\) frame'):
        clips.png_encode_banded_host(frames[0].astype(np.float32))
    with pytest.raises(ValueError, match='png_encode_banded_host: a uint8'):
        clips.png_encode_banded_host(frames[0][:, :, :2])
    with pytest.raises(ValueError, match='png_encode_banded_host: band_rows is a count of rows of at least 1, got 0'):
        clips.png_encode_banded_host(frames[0], 0)
    with pytest.raises(ValueError, match=r"png_encode_banded_host: filters is 'adaptive' or one type 0..4 for every row, got 5"):
        clips.png_encode_banded_host(frames[0], 4, 5)


def test_png_files_shares_jpeg_files_code(clips):
    data, offsets = torch.arange(10, dtype=torch.uint8), torch.tensor([0, 4, 12], dtype=torch.int64)
    for cls, who in ((clips.PngFiles, 'png_encode'), (clips.JpegFiles, 'jpeg_encode')):
        assert cls.files is clips._EncodedFiles.files and cls.nbytes is clips._EncodedFiles.nbytes
        f = cls(data, offsets, torch.tensor([0, 1], dtype=torch.int32))
        assert len(f) == 2 and f.nbytes() == 12 and f.files(check=False) == [bytes(range(4)), b'']
        with pytest.raises(ValueError, match=r'%s: file 1 has status 1 \(the file does not fit in data' % who):
            f.files()
        with pytest.raises(ValueError, match='%s: data uint8' % cls.__name__):
            cls(data, offsets, torch.tensor([0], dtype=torch.int32))


def test_the_checker_built_plain(clips, tmp_path):
    """csrc/png_deflate.h on the host, one lane, against the definition: every band of every case and every small file;
    DESIGN.md "PNG files out" records the same program's run under AddressSanitizer and UBSan"""
    from istvt_amd import build
    vectors = tmp_path / 'png_encode_vectors.txt'
    done = C.write_vectors(str(vectors), clips)
    assert len(done) == 272
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    exe = tmp_path / 'png_deflate_check'
    r = subprocess.run([clang, '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(ROOT, 'tools', 'png_deflate_check.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'png_deflate_check: 272 cases agree', r.stdout + r.stderr
    # the check can fail: one byte of a band's expected bytes changed, one of a file's
    lines = vectors.read_text().splitlines()
    band = next(l for l in lines if l.startswith('band 5x3_c3_b0 '))
    file = next(l for l in lines if l.startswith('file 5x3_c3 '))
    for k, line in enumerate((band, file)):
        flipped = line[:-9] + ('0' if line[-9] != '0' else '1') + line[-8:]
        (tmp_path / 'wrong.txt').write_text(flipped + '\n')
        r = subprocess.run([str(exe), str(tmp_path / 'wrong.txt')], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'png_deflate_check: 1 of 1 cases disagree' in r.stdout and '5x3_c3' in r.stdout, r.stdout


def test_entry_point_declared_and_bound(clips):
    import abi_header as H
    from istvt_amd import _lib, frames, ops
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        text = fh.read()
    assert H.defines(text)['ISTVT_PNG_BAND_ROW_BYTES'] == frames.PNG_BAND_ROW_BYTES == 1728
    assert H.prototypes(text)['istvt_png_encode_u8'] == [('const istvt_jpeg_encode_args*', 'a'), ('int', 'bpp'), ('int', 'band_rows'),
                                                         ('int', 'filter'), ('int', 'raw_stride')]
    assert _lib.SIGNATURES['istvt_png_encode_u8'] == [ctypes.POINTER(_lib.JpegEncodeArgs)] + [ctypes.c_int] * 4
    assert ops.png_encode_u8 is frames.png_encode_u8 and ops.encode_frames is frames.encode_frames
    fn = _lib.lib().istvt_png_encode_u8
    assert fn(None, 3, 16, 5, 16) == -3                                       # no block: refused, nothing launched
    assert fn(ctypes.byref(_lib.JpegEncodeArgs(n=1, H=4, W=4)), 3, 16, 5, 64) == -3      # null pointers
    # bad scalars with every pointer set: host memory, never touched because the call is refused first
    buf = (ctypes.c_char * 4096)()
    at = ctypes.addressof(buf)
    at += -at % 16

    def call(bpp=3, band_rows=16, filt=5, raw_stride=64, **kw):
        a = dict(frames=at, total=48, scratch=at + 256, scratch_bytes=64 + 1728, data=at + 2304, capacity=1024, offsets=at + 3400,
                 status=at + 3500, n=1, H=4, W=4)
        a.update(kw)
        return fn(ctypes.byref(_lib.JpegEncodeArgs(**a)), bpp, band_rows, filt, raw_stride)
    for kw in (dict(bpp=2), dict(band_rows=0), dict(filt=6), dict(filt=-1), dict(raw_stride=48), dict(raw_stride=56), dict(n=0), dict(H=0),
               dict(W=16385), dict(total=47), dict(scratch=at + 257), dict(scratch_bytes=64 + 1727), dict(capacity=0), dict(data=at + 40),
               dict(band_rows=2, scratch_bytes=64 + 2 * 1728 - 1)):
        assert call(**kw) == -3, kw
    # the refusals of the wrapper that need no device
    with pytest.raises(TypeError, match='png_encode_u8: frames must be a uint8 tensor, got list'):
        ops.png_encode_u8([1, 2])
    with pytest.raises(TypeError, match='png_encode_u8: frames must be uint8, got torch.int32'):
        ops.png_encode_u8(torch.zeros((1, 4, 4, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match='png_encode_u8: band_rows is a count of rows of at least 1, got 0'):
        ops.png_encode_u8(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), 0)
    for q in (50, 90):                        # given is given, the default's value too
        with pytest.raises(ValueError, match="encode_frames: quality= goes with format='jpeg'"):
            ops.encode_frames(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), 4, boxes=torch.zeros((1, 4), dtype=torch.int32), quality=q, format='png')
