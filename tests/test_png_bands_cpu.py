"""PNG files by their bands (DESIGN.md "PNG files by their bands") without a device: the baND chunk our writer adds and
clips.png_parse reads; clips.png_decode_bands_host against clips.png_decode_host on every file whose index is true; indexes
that are malformed (ignored) and indexes that lie (a status, the definition's); the plain build of tools/png_bands_check.cpp on
the vectors the definition writes for every band the GPU tests decode; the batch's band table; the ABI rows; the refusals that
need no device."""
import ctypes
import io
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_bands_cases as B
import png_encode_cases as C
import png_streams as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def _same(clips, f):
    """the band-wise and the sequential definition agree on f, bytes and status -> the status"""
    got, s1 = clips.png_decode_bands_host(f, return_status=True)
    ref, s0 = clips.png_decode_host(f, return_status=True)
    assert s1 == s0 and torch.equal(got, ref)
    return s0


def test_the_chunk(clips):
    from PIL import Image
    cases = C.shape_cases() + C.filter_cases()
    assert len(cases) == 44
    for name, frame, R, filters in cases:
        plain = clips.png_encode_banded_host(frame, R, filters)
        data, bands, _ = clips.png_encode_banded_host(frame, R, filters, return_bands=True, index=True)
        H, W = frame.shape[:2]
        bpp = 1 if frame.ndim == 2 else frame.shape[2]
        nb = -(-H // R)
        extra = 12 + 8 + 4 * (nb + 1)
        assert len(bands) == nb and clips.png_band_chunk_bytes(H, R) == extra, name
        assert len(data) == len(plain) + extra and data[:33] + data[33 + extra:] == plain, name
        assert data[37:41] == b'baND' and int.from_bytes(data[33:37], 'big') == extra - 12, name
        assert np.array_equal(np.array(Image.open(io.BytesIO(data))), frame), name
        hd, hp = clips.png_parse(data), clips.png_parse(plain)
        assert hd.data == hp.data and hp.bands is None, name
        assert hd.bands == (min(R, H), [b for b, _ in bands] + [bands[-1][1]]), name
        assert hd.bands[1][0] == 2 and hd.bands[1][-1] == len(hd.data) + 2, name
        assert len(data) <= clips.png_encoded_bound(H, W, bpp, R, index=True) == clips.png_encoded_bound(H, W, bpp, R) + extra, name
        assert clips.png_encode_files_host(frame[None], R, filters, index=True) == [data], name
        assert clips.png_encode_files_host(frame[None], R, filters) == [plain], name
    with pytest.raises(ValueError, match='png_encode_banded_host: index is True or False'):
        clips.png_encode_banded_host(cases[0][1], index=1)


def test_equivalence(clips, golden_dir):
    """a true index: the band-wise definition is the sequential one"""
    for name, frame, R, filters in C.shape_cases() + C.filter_cases():
        f = clips.png_encode_banded_host(frame, R, filters, index=True)
        assert _same(clips, f) == 0, name
        got = clips.png_decode_bands_host(clips.png_parse(f)).numpy()        # a parsed file is taken as it is
        assert np.array_equal(got, np.repeat(frame[:, :, None], 3, 2) if frame.ndim == 2 else frame[:, :, :3]), name
    for name, f in B.mixed_files(clips):
        assert clips.png_parse(f).bands is not None and _same(clips, f) == 0, name
    for name, f in B.pil_files(golden_dir, 15):                               # no index: one band, the sequential decoder
        assert clips.png_parse(f).bands is None and _same(clips, f) == 0, name
    kinds = set()
    for name, f in B.flush_files(clips):
        hd = clips.png_parse(f)
        assert hd.bands is not None and _same(clips, f) == 0, name
        for _, begin, _, _, _ in clips.png_band_table(hd):                     # the type of every band's first block
            kinds.add((hd.data[begin] >> 1) & 3)
    assert kinds == {0, 1, 2}
    # the damaged streams of the sequential tests have no index: the same status from both
    for name, raw, want in P.damaged_streams():
        assert _same(clips, clips.png_wrap(P.H, P.W, 2, P.zlib_wrap(raw))) == want, name


def test_bands_inflate_alone(clips):
    """every band of a flush file is a stream zlib inflates on its own once BFINAL is put behind it, to the band's rows"""
    for name, f in B.flush_files(clips):
        hd = clips.png_parse(f)
        whole = zlib.decompress(hd.data, -15)
        table = clips.png_band_table(hd)
        assert len(table) > 1 and sum(r[4] for r in table) == len(whole) == hd.raw_bytes, name
        for k, (_, begin, end, at, nbytes) in enumerate(table):
            tail = b'' if k == len(table) - 1 else b'\x01\x00\x00\xff\xff'
            assert zlib.decompress(hd.data[begin:end] + tail, -15) == whole[at:at + nbytes], (name, k)
            assert hd.data[end - 4:end] == b'\x00\x00\xff\xff' or k == len(table) - 1, (name, k)


def test_a_malformed_index_is_ignored(clips):
    frame = P.pattern(20, 31, 3, 77)
    plain, bands, _ = clips.png_encode_banded_host(frame, 8, 'adaptive', return_bands=True)
    off = [b for b, _ in bands] + [bands[-1][1]]
    good = B.chunk(b'baND', B.index_body(8, off))
    assert clips.png_parse(B.splice(plain, good)).bands == (8, off)
    idat = plain.index(b'IDAT') - 4
    after = len(plain) - 12                                                   # in front of IEND
    cases = {
        'a wrong length': B.splice(plain, B.chunk(b'baND', B.index_body(8, off) + bytes(4))),
        'a length that is no multiple of 4': B.splice(plain, B.chunk(b'baND', B.index_body(8, off) + bytes(1))),
        'an empty chunk': B.splice(plain, B.chunk(b'baND', b'')),
        'nb off by one': B.splice(plain, B.chunk(b'baND', B.index_body(8, off, nb=len(off)))),
        'nb of another R': B.splice(plain, B.chunk(b'baND', B.index_body(4, off))),
        'R = 0': B.splice(plain, B.chunk(b'baND', B.index_body(0, off))),
        'off[0] != 2': B.splice(plain, B.chunk(b'baND', B.index_body(8, [3] + off[1:]))),
        'a non-increasing offset': B.splice(plain, B.chunk(b'baND', B.index_body(8, off[:1] + [off[2], off[2]] + off[3:]))),
        'a wrong last offset': B.ignored_index_file(clips),
        'two chunks': B.splice(plain, good + good),
        'a chunk after IDAT': B.splice(plain, good, after),
        'one before and one after IDAT': B.splice(B.splice(plain, good, after), good),
    }
    assert idat == 33
    ref = clips.png_decode_host(plain)
    for name, f in cases.items():
        hd = clips.png_parse(f)                                               # never a refusal
        assert hd.bands is None and hd.data == clips.png_parse(plain).data, name
        got, status = clips.png_decode_bands_host(f, return_status=True)
        assert status == 0 and torch.equal(got, ref), name
        assert clips.png_band_table(hd) == [[0, 0, len(hd.data), 0, hd.raw_bytes]], name


def test_an_index_that_lies_gets_a_status(clips):
    cases = B.lying_files(clips)
    assert [n for n, _, _ in cases] == ['offset_plus_1', 'sync_flush', 'bfinal_in_a_middle_band', 'bfinal_missing_in_the_last_band',
                                        'band_rows_wrong', 'bit_flipped_in_a_band', 'band_cut_short']
    for name, f, want in cases:
        hd = clips.png_parse(f)
        assert hd.bands is not None, name
        frame, status = clips.png_decode_bands_host(f, return_status=True)
        raw, statuses = clips.png_inflate_bands_host(hd)
        assert status != 0 and status == next(s for s in statuses if s), name
        assert want is None or status == want, (name, status)
        assert tuple(frame.shape) == (hd.H, hd.W, 3) and not bool(frame.any()), name
    by = {n: f for n, f, _ in cases}
    # the stream of the sync-flush file is sound: only the band-wise decoder refuses it, in the second band
    assert clips.png_decode_host(by['sync_flush'], return_status=True)[1] == 0
    assert clips.png_inflate_bands_host(clips.png_parse(by['sync_flush']))[1][:2] == [0, 4]
    assert clips.png_inflate_bands_host(clips.png_parse(by['bfinal_in_a_middle_band']))[1][0] == 7
    assert clips.png_inflate_bands_host(clips.png_parse(by['bfinal_missing_in_the_last_band']))[1] == [0, 0, 0, 0, 1]
    assert clips.png_decode_host(by['bfinal_in_a_middle_band'], return_status=True)[1] == 5     # it stops at the first BFINAL
    # BFINAL is looked at before the block's type in a band that is not the last; in the last band a reserved type is status 2
    assert clips._png_inflate(bytes([0b111]), 0, middle=True)[1] == 7 and clips._png_inflate(bytes([0b111]), 0)[1] == 2
    assert clips.PNG_BAND_STATUS == {7: 'the band index disagrees with the stream'} and 7 not in clips.PNG_STATUS
    with pytest.raises(ValueError, match=r'png_decode: file 1 is damaged \(status 7: the band index disagrees with the stream\)'):
        clips.check_png_status(torch.tensor([0, 7], dtype=torch.int32))


def test_the_checker_built_plain(clips, golden_dir, tmp_path):
    """pi_inflate<true> of csrc/png_inflate.h on the host, one lane, against the definition on every band that the GPU tests
    send to a device; DESIGN.md "PNG files by their bands" records the same program's run under AddressSanitizer and UBSan"""
    from istvt_amd import build
    vectors = tmp_path / 'png_band_vectors.txt'
    done = B.write_vectors(str(vectors), clips, B.device_files(clips, golden_dir))
    assert len(done) > 400 and {s for _, s in done} >= {0, 1, 4, 5, 7}
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    exe = tmp_path / 'png_bands_check'
    r = subprocess.run([clang, '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(ROOT, 'tools', 'png_bands_check.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'png_bands_check: %d bands agree' % len(done), r.stdout + r.stderr
    # the check can fail: a vector with another status, and one with another byte
    lines = vectors.read_text().splitlines()
    name, status, rest = lines[0].split(' ', 2)
    (tmp_path / 'wrong.txt').write_text('%s %d %s\n' % (name, 7, rest))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong.txt')], capture_output=True, text=True, timeout=120)
    assert status == '0' and r.returncode == 1 and 'status 0, the definition has 7' in r.stdout
    head, want = lines[0].rsplit(' ', 1)
    (tmp_path / 'wrong2.txt').write_text('%s %s%02x\n' % (head, want[:-2], int(want[-2:], 16) ^ 1))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong2.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'the bytes differ' in r.stdout


def test_batch_layout(clips, golden_dir):
    files = [f for _, f in B.mixed_files(clips)[:4]] + [B.ignored_index_file(clips)] + [f for _, f in B.pil_files(golden_dir, 1)]
    heads = [clips.png_parse(f) for f in files]
    plain, b = clips.png_batch(files), clips.png_batch(files, bands='index')
    assert plain.bands is None and plain.images[:, 6:].tolist() == [[0, 0]] * 6 and plain.scratch_bytes == 6 * plain.raw_stride
    assert bytes(plain.data.numpy().tobytes()) == bytes(b.data.numpy().tobytes()) and plain.images[:, :6].tolist() == b.images[:, :6].tolist()
    assert b.bands.dtype == torch.int32 and tuple(b.bands.shape) == (sum(len(clips.png_band_table(h)) for h in heads), clips.PNG_BAND_INTS)
    assert b.scratch_bytes == 6 * b.raw_stride + 4 * b.bands.shape[0] and b.raw_stride == plain.raw_stride
    at = 0
    for i, (row, h) in enumerate(zip(b.images.tolist(), heads)):
        table = clips.png_band_table(h, i, row[4])
        assert row[6:] == [at, len(table)] and b.bands[at:at + len(table)].tolist() == table
        assert table[0][1] == row[4] and table[-1][2] == row[5] and sum(r[4] for r in table) == h.raw_bytes
        assert all(p[2] == q[1] and p[3] + p[4] == q[3] for p, q in zip(table, table[1:]))
        at += len(table)
    assert [r[7] for r in b.images.tolist()] == [1, 1, 1, 3, 1, 1]
    with pytest.raises(ValueError, match=r"png_batch: bands is None or 'index', got 'rows'"):
        clips.png_batch(files, bands='rows')


def test_entry_points_declared_and_bound(clips):
    import abi_header as H
    from istvt_amd import _lib, frames, ops
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        text = fh.read()
    assert H.defines(text)['ISTVT_PNG_BAND_INTS'] == clips.PNG_BAND_INTS == 5
    assert H.prototypes(text)['istvt_png_decode_bands_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'raw_stride')]
    assert H.prototypes(text)['istvt_png_encode_indexed_u8'] == H.prototypes(text)['istvt_png_encode_u8']
    assert _lib.SIGNATURES['istvt_png_decode_bands_u8'] == _lib.SIGNATURES['istvt_png_decode_u8']
    assert _lib.SIGNATURES['istvt_png_encode_indexed_u8'] == _lib.SIGNATURES['istvt_png_encode_u8']
    assert ops.png_decode_u8 is frames.png_decode_u8 and ops.png_encode_u8 is frames.png_encode_u8
    lib = _lib.lib()
    assert lib.istvt_png_decode_bands_u8(None, 16) == -3 and lib.istvt_png_encode_indexed_u8(None, 3, 16, 5, 16) == -3
    args = _lib.JpegDecodeArgs(n=1, nseg=1, Hc=8, Wc=8)
    assert lib.istvt_png_decode_bands_u8(ctypes.byref(args), 16) == -3        # null pointers


def _bands_args(clips, batch, bands):
    """the argument block of a call on host memory: the entry refuses it before any launch, or the test is wrong"""
    from istvt_amd import _lib
    keep = [torch.zeros(batch.scratch_bytes + 16, dtype=torch.uint8), torch.zeros(batch.n * 64 * 64 * 3, dtype=torch.uint8),
            torch.zeros((batch.n, 2), dtype=torch.int32), torch.zeros(batch.n, dtype=torch.int32), bands]
    scratch = keep[0][(-keep[0].data_ptr()) % 16:]
    data = batch.data
    assert data.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0
    return keep, _lib.JpegDecodeArgs(
        bytes=data.data_ptr(), nbytes=batch.nbytes, images=batch.images.data_ptr(), images_host=batch.images.data_ptr(),
        segments=bands.data_ptr(), segments_host=bands.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=batch.scratch_bytes,
        out=keep[1].data_ptr(), sizes=keep[2].data_ptr(), status=keep[3].data_ptr(), n=batch.n, nseg=int(bands.shape[0]), Hc=64, Wc=64)


def test_the_entry_checks_the_band_table(clips):
    """every disagreement between the host tables is -3 before any launch: no device is needed to see it"""
    from istvt_amd import _lib
    files = [clips.png_encode_banded_host(P.pattern(20, 31, 3, s), 8, index=True) for s in (1, 2)]
    batch = clips.png_batch(files, bands='index')
    assert batch.bands.shape[0] == 6
    lib = _lib.lib()

    def call(bands, images=None, scratch_bytes=None, nseg=None):
        keep, args = _bands_args(clips, batch, bands.contiguous())
        if images is not None:
            keep.append(images)
            args.images_host = images.data_ptr()
        if scratch_bytes is not None:
            args.scratch_bytes = scratch_bytes
        if nseg is not None:
            args.nseg = nseg
        return lib.istvt_png_decode_bands_u8(ctypes.byref(args), batch.raw_stride)

    def edit(r, c, v):
        t = batch.bands.clone()
        t[r, c] = v
        return t
    stride = 1 + 31 * 3
    cases = {
        'a band that begins in front of its file': edit(3, 1, int(batch.images[1, 4]) - 1),
        'a band that ends behind its file': edit(5, 2, int(batch.images[1, 5]) + 1),
        'a band that ends in front of its begin': edit(1, 2, int(batch.bands[1, 1]) - 1),
        'a band of another file': edit(2, 0, 1),
        'output ranges with a gap': edit(1, 3, 8 * stride + 1),
        'output ranges that overlap': edit(4, 3, 8 * stride - 1),
        'a negative output length': edit(0, 4, -1),
        'output bytes that do not sum to the file': edit(2, 4, 4 * stride + 1),
        'output bytes past the file': edit(5, 4, 5 * stride),
    }
    for name, bands in cases.items():
        assert call(bands) == -3, name
    images = batch.images.clone()
    images[1, 6] = 2
    assert call(batch.bands, images=images) == -3, 'a first band row that does not follow the file before'
    images = batch.images.clone()
    images[0, 7], images[1, 6], images[1, 7] = 2, 2, 4
    assert call(batch.bands, images=images) == -3, 'band counts that cut the files elsewhere'
    images = batch.images.clone()
    images[1, 7] = 0
    assert call(batch.bands, images=images) == -3, 'a file without a band'
    assert call(batch.bands, nseg=7) == -3 and call(batch.bands, nseg=5) == -3, 'a count that is not the table'
    assert call(batch.bands, scratch_bytes=batch.scratch_bytes - 1) == -3, 'a scratch without the status words'
    assert call(batch.bands, scratch_bytes=2 * batch.raw_stride) == -3, 'the scratch of a batch without bands'


def test_refusals_that_need_no_device(clips):
    from istvt_amd import ops
    f = clips.png_encode_banded_host(P.pattern(9, 7, 3, 0), 4, index=True)
    with pytest.raises(ValueError, match=r"png_decode_u8: bands is None or 'index', got 'all'"):
        ops.png_decode_u8([f], bands='all')
    with pytest.raises(ValueError, match=r"png_decode_u8: bands is None or 'index', got True"):
        ops.png_decode_u8(clips.png_batch([f]), checked=True, bands=True)
    with pytest.raises(ValueError, match=r"png_decode_u8: bands='index' with a clips.PngBatch that was packed without bands"):
        ops.png_decode_u8(clips.png_batch([f]), checked=True, bands='index')
    frames = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 16, 16]] * 2, dtype=torch.int32)
    for index in (True, False):
        with pytest.raises(ValueError, match=r"encode_frames: index= goes with format='png' \(the band index of a PNG file\); JPEG "
                                             r"files have none"):
            ops.encode_frames(frames, 8, boxes, index=index)
    with pytest.raises(ValueError, match='png_encode_u8: index is True or False, got 1'):
        ops.png_encode_u8(frames, index=1)
    with pytest.raises(ValueError, match='png_encode_u8: index is True or False'):
        ops.encode_frames(frames, 8, boxes, format='png', index='yes')
