"""PNG bands that stand alone (DESIGN.md "PNG bands that stand alone") without a device: the writer's restricted rows and the
flag in the index; the parser's attribute; the definition clips.png_decode_alone_host with status 10 and its precedence; the
rows and flags clips.png_batch and clips.png_bank pack, their refusals, and clips.png_bank_decode_host on an alone bank; what
the three decode entries refuse before any launch, on host memory; the plain build of tools/png_alone_check.cpp on the vectors
the definition writes for every flagged file the GPU tests hand to a device; the ABI rows.  Everything is exact."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
import torch

import png_alone_cases as A
import png_bands_cases as B
import png_bank_cases as K
import png_encode_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def _chunk_words(data):
    length = int.from_bytes(data[33:37], 'big')
    assert data[37:41] == b'baND'
    return [int.from_bytes(data[41 + i:45 + i], 'big') for i in range(0, length, 4)]


def test_the_writer(clips):
    from PIL import Image
    changed = 0
    for name, frame, R, filters in C.shape_cases() + C.filter_cases():
        indexed = clips.png_encode_banded_host(frame, R, filters, index=True)
        alone, bands, types = clips.png_encode_banded_host(frame, R, filters, return_bands=True, index=True, alone=True)
        assert clips.png_encode_banded_host(frame, R, filters, index=True, alone=False) == indexed, name
        assert clips.png_encode_banded_host(frame, R, filters, alone=False) == clips.png_encode_banded_host(frame, R, filters), name
        H, W = frame.shape[:2]
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        # the rows: every band's first row has type 0 or 1, every other row is the unrestricted writer's, byte for byte
        free, rows = clips.png_filter_rows_host(frame, filters), clips.png_filter_rows_host(frame, filters, alone_rows=R)
        assert rows[:, 0].tolist() == types
        for r in range(H):
            if r % R == 0:
                assert rows[r, 0] in (0, 1), (name, r)
                if filters != 'adaptive':
                    assert rows[r, 0] == (0, 1, 0, 1, 1)[filters], (name, r)
                changed += int(rows[r, 0] != free[r, 0])
            else:
                assert rows[r].tobytes() == free[r].tobytes(), (name, r)
        # the file carries them, and its length differs from the indexed file's by what the stream's differs
        hd, hi = clips.png_parse(alone), clips.png_parse(indexed)
        raw, statuses = clips.png_inflate_bands_host(hd)
        assert bytes(raw) == rows.tobytes() and set(statuses) == {0}, name
        assert len(alone) - len(indexed) == len(hd.data) - len(hi.data), name
        assert len(alone) <= clips.png_encoded_bound(H, W, ch, R, index=True, alone=True) == clips.png_encoded_bound(H, W, ch, R, index=True)
        # the chunk: the R word has bit 31 and nothing else differs in its layout
        wa, wi = _chunk_words(alone), _chunk_words(indexed)
        assert wa[0] == wi[0] | clips.PNG_BAND_ALONE == min(R, H) | 0x80000000 and wa[1] == wi[1] and len(wa) == len(wi), name
        assert wa[2] == 2 and wa[2:-1] == [b for b, _ in bands] and alone[:33] == indexed[:33]
        assert hd.alone is True and hi.alone is False and hd.bands == (min(R, H), wa[2:]) and hi.bands[0] == min(R, H)
        # PIL and the sequential definition give the source pixels
        px = np.asarray(Image.open(io.BytesIO(alone)))
        assert np.array_equal(px, frame), name
        want = torch.from_numpy(np.ascontiguousarray(frame.reshape(H, W, ch)))
        want = want.expand(H, W, 3) if ch == 1 else want[:, :, :3]
        assert torch.equal(clips.png_decode_host(alone), want), name
    assert changed > 20
    frame = C.smooth(9, 11, 3, 5)
    assert clips.png_encode_files_host(frame[None], 4, index=True, alone=True) == [clips.png_encode_banded_host(frame, 4, index=True, alone=True)]
    for call in (lambda: clips.png_encode_banded_host(frame, 4, alone=True), lambda: clips.png_encode_files_host(frame[None], 4, alone=True),
                 lambda: clips.png_encoded_bound(9, 11, 3, 4, alone=True)):
        with pytest.raises(ValueError, match=r'png_enc\w+: alone=True needs index=True \(the flag lives in the band index\)'):
            call()
    with pytest.raises(ValueError, match='png_encode_banded_host: alone is True or False, got 1'):
        clips.png_encode_banded_host(frame, 4, index=True, alone=1)


def test_the_parser(clips):
    for name, f in A.alone_files(clips):
        assert clips.png_parse(f).alone is True, name
    # every indexed and malformed-index case of before parses as before, with alone == False
    old = B.mixed_files(clips) + B.flush_files(clips) + [(n, f) for n, f, _ in B.lying_files(clips)]
    for name, f in old:
        hd = clips.png_parse(f)
        assert hd.alone is False and hd.bands is not None and hd.bands[0] == _chunk_words(f)[0], name
    ignored = B.ignored_index_file(clips)
    hd = clips.png_parse(ignored)
    assert hd.bands is None and hd.alone is False
    # a flagged word whose stripped R fails the checks: no index, no flag, no refusal
    hd = clips.png_parse(A.set_flag(ignored))
    assert hd.bands is None and hd.alone is False
    f = B.mixed_files(clips)[3][1]                                 # 17 rows in bands of 8: three bands, and 9 would give two
    words = _chunk_words(f)
    body = b''.join(v.to_bytes(4, 'big') for v in [(words[0] + 1) | 0x80000000] + words[1:])
    hd = clips.png_parse(f[:33] + B.chunk(b'baND', body) + f[33 + 12 + 4 * len(words):])
    assert hd.bands is None and hd.alone is False
    # the bit by hand on a sound index: the same bands, and the flag
    hd, flagged = clips.png_parse(f), clips.png_parse(A.set_flag(f))
    assert flagged.alone is True and flagged.bands == hd.bands and flagged.data == hd.data
    assert clips.png_parse(clips.png_encode_host(C.smooth(5, 5, 3, 1))).alone is False


def test_the_definition(clips, golden_dir):
    for name, f in A.alone_files(clips):
        got, status = clips.png_decode_alone_host(f, return_status=True)
        want, s = clips.png_decode_host(f, return_status=True)
        assert status == s == 0 and torch.equal(got, want), name
        assert torch.equal(clips.png_decode_alone_host(clips.png_parse(f)), want)
    for name, frame, R, filters in C.filter_cases():
        f = clips.png_encode_banded_host(frame, R, filters, index=True, alone=True)
        assert torch.equal(clips.png_decode_alone_host(f), clips.png_decode_host(f)), name
    # a file without the flag is png_decode_bands_host, bytes and status
    for name, f, _ in B.lying_files(clips)[:4]:
        got, want = clips.png_decode_alone_host(f, return_status=True), clips.png_decode_bands_host(f, return_status=True)
        assert torch.equal(got[0], want[0]) and got[1] == want[1], name
    lying = {name: (f, status) for name, f, status in A.lying_files(clips)}
    for ft in (2, 3, 4):
        f, want = lying['fixed_%d_flagged' % ft]
        got, status = clips.png_decode_alone_host(f, return_status=True)
        assert status == want == 10 and not bool(got.any()) and tuple(got.shape) == (36, 25, 3)
        assert clips.png_decode_host(f, return_status=True)[1] == 0            # the stream is sound: the flag lies
    f, want = lying['row_0_alone_has_type_2']
    got, status = clips.png_decode_alone_host(f, return_status=True)
    assert status == want == 0 and torch.equal(got, clips.png_decode_host(f))
    rows = np.frombuffer(bytes(clips.png_inflate_bands_host(clips.png_parse(f))[0]), np.uint8).reshape(36, -1)
    assert rows[0, 0] == 2 and set(rows[8::8, 0].tolist()) <= {0, 1}
    # precedence: the band's status, then 6, then 10
    f, want = lying['damaged_band_and_lying_row']
    assert clips.png_decode_alone_host(f, return_status=True)[1] == want and want in clips.PNG_STATUS and want != 6
    f, want = lying['filter_5_and_lying_row']
    assert clips.png_decode_alone_host(f, return_status=True)[1] == want == 6
    assert clips.PNG_ALONE_STATUS.keys() == {10}
    with pytest.raises(ValueError, match=r"png_decode: file 1 is damaged \(status 10: the index says its bands stand alone, and a band's "
                                         r"first row is filtered against the row above\)"):
        clips.check_png_status(torch.tensor([0, 10]))


def test_batch_and_bank(clips, golden_dir):
    named = A.mixed_files(clips, golden_dir)
    files = [f for _, f in named]
    flags = [int(clips.png_parse(f).alone) for f in files]
    assert flags == [1] * 10 + [0, 0] + [1] * 7
    batch, plain = clips.png_batch(files, bands='index', alone=True), clips.png_batch(files, bands='index')
    assert batch.alone.dtype == torch.int32 and batch.alone.tolist() == flags and plain.alone is None
    assert clips.png_batch(files).alone is None
    for name in ('data', 'images', 'bands'):
        assert torch.equal(getattr(batch, name), getattr(plain, name)), name
    assert batch.scratch_bytes == plain.scratch_bytes
    with pytest.raises(ValueError, match=r"png_batch: alone=True needs bands='index' \(the flag lives in the band index\)"):
        clips.png_batch(files, alone=True)
    with pytest.raises(ValueError, match=r"png_bank: alone=True needs bands='index' \(the flag lives in the band index\)"):
        clips.png_bank(files, bands=None, alone=True)
    with pytest.raises(ValueError, match='png_batch: alone is True or False, got 1'):
        clips.png_batch(files, bands='index', alone=1)
    with pytest.raises(ValueError, match="png_bank: alone is True or False, got 'yes'"):
        clips.png_bank(files, alone='yes')
    bank, old = clips.png_bank(files, alone=True), clips.png_bank(files)
    assert bank.alone is True and old.alone is False
    assert bank.images[:, 9].tolist() == flags and old.images[:, 9].tolist() == [0] * len(files)
    assert torch.equal(bank.images[:, :9], old.images[:, :9]) and torch.equal(bank.bands, old.bands) and torch.equal(bank.data, old.data)
    assert clips.png_bank_scratch_bytes(bank, 3) == clips.png_bank_scratch_bytes(old, 3)
    # the bank's definition places png_decode_alone_host; status 10 keeps the size and zeroes the frame
    refs = A.reference(clips, named)
    index = list(range(len(files))) + [-1, 3, len(files)]
    frames, sizes, status = clips.png_bank_decode_host(bank, index)
    for j, i in enumerate(index):
        if 0 <= i < len(files):
            f, s = refs[i]
            assert status[j] == s and sizes[j].tolist() == list(f.shape[:2]), named[i][0]
            assert torch.equal(frames[j, :f.shape[0], :f.shape[1]], f) and int(frames[j].sum()) == int(f.sum())
        else:
            assert status[j] == 8 and sizes[j].tolist() == [0, 0] and not bool(frames[j].any())
    assert status.tolist().count(10) == 3 and 6 in status.tolist()
    # without alone=True the flag is not looked at: today's path, the right pixels (a lying file decodes: its stream is sound)
    was = clips.png_bank_decode_host(old, list(range(len(files))))
    for i, f in enumerate(files):
        ref, s = clips.png_decode_bands_host(f, return_status=True)
        assert was[2][i] == s and torch.equal(was[0][i, :ref.shape[0], :ref.shape[1]], ref)
    # doctored band rows of a flagged file: status 9 at its place only
    good = A.alone_bank(clips)
    for name, bad, place in A.doctored(clips, good):
        got = clips.png_bank_decode_host(bad, [place, (place + 1) % good.n])
        assert got[2].tolist() == [9, 0] and got[1][0].tolist() == [0, 0] and not bool(got[0][0].any()), name


def _aligned(t):
    room = torch.zeros(t.numel() * t.element_size() + 16, dtype=torch.uint8)
    room = room[(-room.data_ptr()) % 16:][:t.numel() * t.element_size()]
    room.copy_(t.contiguous().view(torch.uint8).flatten())
    return room


def test_the_batch_entry_refuses_before_any_launch(clips):
    """a valid block on host memory, one thing made wrong per case, -3 back: nothing was launched then, which is why host
    memory will do"""
    from istvt_amd import _lib
    files = [f for _, f in A.alone_files(clips)[:3]] + [B.mixed_files(clips)[1][1]]
    batch = clips.png_batch(files, bands='index', alone=True)
    assert batch.alone.tolist() == [1, 1, 1, 0]
    n, nband, Hc, Wc = batch.n, int(batch.bands.shape[0]), 130, 33
    entry = _lib.lib().istvt_png_decode_alone_u8

    def block(flags=None, bands=None):
        keep = dict(data=_aligned(batch.data), scratch=_aligned(torch.zeros(batch.scratch_bytes, dtype=torch.uint8)),
                    out=torch.zeros(n * Hc * Wc * 3, dtype=torch.uint8), sizes=torch.zeros((n, 2), dtype=torch.int32),
                    status=torch.zeros(n, dtype=torch.int32), images=batch.images.clone(),
                    bands=batch.bands.clone() if bands is None else bands, flags=batch.alone.clone() if flags is None else flags)
        args = _lib.JpegDecodeArgs(bytes=keep['data'].data_ptr(), nbytes=batch.nbytes, images=keep['images'].data_ptr(),
                                   images_host=keep['images'].data_ptr(), segments=keep['bands'].data_ptr(),
                                   segments_host=keep['bands'].data_ptr(), qtabs=keep['flags'].data_ptr(), htabs=keep['flags'].data_ptr(),
                                   scratch=keep['scratch'].data_ptr(), scratch_bytes=batch.scratch_bytes, out=keep['out'].data_ptr(),
                                   sizes=keep['sizes'].data_ptr(), status=keep['status'].data_ptr(), stream=None, n=n, nseg=nband,
                                   nq=n, nh=n, Hc=Hc, Wc=Wc)
        return args, keep

    cases = [('null_' + f, {f: None}) for f in ('bytes', 'images', 'images_host', 'segments', 'segments_host', 'qtabs', 'htabs', 'scratch',
                                                'out', 'sizes', 'status')]
    cases += [('nq_0', dict(nq=0)), ('nq_other', dict(nq=n + 1)), ('nh_other', dict(nh=n - 1)), ('n_0', dict(n=0)),
              ('nseg_short', dict(nseg=nband - 1)), ('scratch_one_byte_short', dict(scratch_bytes=batch.scratch_bytes - 1)),
              ('canvas_small', dict(Hc=129)), ('canvas_wide', dict(Wc=16385)), ('nbytes_negative', dict(nbytes=-1))]
    for name, fields in cases:
        args, keep = block()
        for f, v in fields.items():
            setattr(args, f, v)
        assert entry(ctypes.byref(args), batch.raw_stride) == -3, name
    assert entry(None, batch.raw_stride) == -3
    args, keep = block()
    assert entry(ctypes.byref(args), batch.raw_stride + 8) == -3 and entry(ctypes.byref(args), 0) == -3
    for bad in (2, 3, -1, 0x80000000 - 2 ** 32):                  # a flag word with bits other than bit 0
        flags = batch.alone.clone()
        flags[1] = bad
        args, keep = block(flags=flags)
        assert entry(ctypes.byref(args), batch.raw_stride) == -3, bad
    # band rows of a flagged file that pass the banded entry's checks (ranges that follow one another from 0 to the end) and
    # are not the R-row bands of an index: a band edge moved by a row, and the bands of the unflagged file given the flag
    first, stride = int(batch.images[1, 6]), 1 + 31 * 3
    moved = batch.bands.clone()
    moved[first, 4] += stride
    moved[first + 1, 3] += stride
    moved[first + 1, 4] -= stride
    args, keep = block(bands=moved)
    assert entry(ctypes.byref(args), batch.raw_stride) == -3
    merged = batch.bands.clone()                                   # the last two bands' rows in the last but one: its out_bytes fits no R
    last = first + int(batch.images[1, 7]) - 1
    merged[last - 1, 4] += 1
    merged[last, 3] += 1
    merged[last, 4] -= 1
    args, keep = block(bands=merged)
    assert entry(ctypes.byref(args), batch.raw_stride) == -3


def test_the_bank_entries_refuse_before_any_launch(clips):
    """the table of istvt_png_decode_bank_u8 (tests/test_png_bank_cpu.py) on the two new entries"""
    from istvt_amd import _lib
    bank = clips.png_bank(K.small_files(clips), alone=True)
    M, HC, WC = 3, 12, 14
    assert (bank.n, bank.band_max, bank.Hmax, bank.Wmax) == (3, 3, HC, WC)
    need = clips.png_bank_scratch_bytes(bank, M)
    entry, drawn = _lib.lib().istvt_png_decode_bank_alone_u8, _lib.lib().istvt_png_decode_bank_alone_drawn_u8

    def block():
        keep = dict(data=_aligned(bank.data), scratch=_aligned(torch.zeros(need, dtype=torch.uint8)),
                    out=torch.zeros(M * HC * WC * 3, dtype=torch.uint8), sizes=torch.zeros((M, 2), dtype=torch.int32),
                    status=torch.zeros(M, dtype=torch.int32), index=torch.tensor([2, 0, 2], dtype=torch.int32),
                    images=bank.images.clone(), bands=bank.bands.clone())
        args = _lib.JpegDecodeArgs(bytes=keep['data'].data_ptr(), nbytes=bank.nbytes, images=keep['images'].data_ptr(),
                                   images_host=keep['index'].data_ptr(), segments=keep['bands'].data_ptr(), segments_host=None, qtabs=None,
                                   htabs=None, scratch=keep['scratch'].data_ptr(), scratch_bytes=need, out=keep['out'].data_ptr(),
                                   sizes=keep['sizes'].data_ptr(), status=keep['status'].data_ptr(), stream=None, n=bank.n, nseg=bank.nband,
                                   nq=0, nh=0, Hc=HC, Wc=WC)
        return args, keep

    scalars = dict(m=M, band_max=bank.band_max, raw_stride=bank.raw_stride)
    cases = [('null_' + f, {f: None}, {}) for f in ('bytes', 'images', 'segments', 'images_host', 'scratch', 'out', 'sizes', 'status')]
    cases += [('m_0', {}, dict(m=0)), ('m_negative', {}, dict(m=-1)), ('band_max_0', {}, dict(band_max=0)),
              ('raw_stride_unaligned', {}, dict(raw_stride=bank.raw_stride + 8)), ('raw_stride_small', {}, dict(raw_stride=0)),
              ('m_band_max_beyond_int', {}, dict(m=2 ** 20, band_max=2 ** 11)), ('scratch_one_byte_short', dict(scratch_bytes=need - 1), {}),
              ('canvas_0', dict(Hc=0), {}), ('canvas_wide', dict(Wc=16385), {}), ('n_0', dict(n=0), {}), ('nseg_0', dict(nseg=0), {}),
              ('nbytes_negative', dict(nbytes=-1), {})]
    for name, fields, extra in cases:
        args, keep = block()
        for f, v in fields.items():
            setattr(args, f, v)
        s = dict(scalars, **extra)
        assert entry(ctypes.byref(args), s['m'], s['band_max'], s['raw_stride']) == -3, name
    assert entry(None, M, bank.band_max, bank.raw_stride) == -3
    args, keep = block()
    args.out = args.bytes
    assert entry(ctypes.byref(args), M, bank.band_max, bank.raw_stride) == -3
    args, keep = block()
    for Bc, T, ints in ((0, 3, 64), (1, 0, 64), (1, 3, 36 + 2)):
        assert drawn(ctypes.byref(args), Bc, T, ints, bank.band_max, bank.raw_stride) == -3
    assert drawn(None, 1, 3, 64, bank.band_max, bank.raw_stride) == -3


def test_the_host_check(clips, golden_dir, tmp_path):
    """tools/png_alone_check.cpp, built plain, on the vectors of every flagged file the GPU tests hand to a device; a doctored
    status and a doctored row range fail.  DESIGN.md has its run under AddressSanitizer and UBSan."""
    from istvt_amd import build
    vectors = tmp_path / 'png_alone_vectors.txt'
    lines, statuses = A.write_vectors(str(vectors), clips, golden_dir)
    assert len(lines) == 17 + 10 + 3 and statuses == {0, 3, 6, 9, 10}
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    exe = tmp_path / 'png_alone_check'
    r = subprocess.run([clang, '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(ROOT, 'tools', 'png_alone_check.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith('png_alone_check: %d files and ' % len(lines)) and r.stdout.strip().endswith('waves agree'), \
        r.stdout + r.stderr
    # a file with another status
    line = next(l for l in lines if l.startswith('F fixed_3_flagged '))
    head, status, R, spans = line.rsplit(' ', 3)
    assert status == '10'
    (tmp_path / 'wrong.txt').write_text('%s 0 %s %s\n' % (head, R, spans))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'wave 0 has status 10, the definition has 0' in r.stdout
    # a wave with another row range
    line = next(l for l in lines if l.startswith('F 20x31x3_r8 '))
    head, spans = line.rsplit(' ', 1)
    assert spans == '0:8,8:16,16:20'
    (tmp_path / 'wrong2.txt').write_text('%s 0:8,8:17,17:20\n' % head)
    r = subprocess.run([str(exe), str(tmp_path / 'wrong2.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'wave 1 takes rows 8:16, the definition has 8:17' in r.stdout
    # doctored band rows that claim to fit
    line = next(l for l in lines if l.startswith('F doctored_wrong_out_'))
    head, status, R, spans = line.rsplit(' ', 3)
    assert (status, R, spans) == ('9', '0', '-')
    (tmp_path / 'wrong3.txt').write_text('%s 0 8 0:8,8:16,16:20\n' % head)
    r = subprocess.run([str(exe), str(tmp_path / 'wrong3.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'the file has status 9, the definition has 0' in r.stdout


def test_the_abi_rows(clips):
    from istvt_amd import _lib, ops
    dec, enc = ctypes.POINTER(_lib.JpegDecodeArgs), ctypes.POINTER(_lib.JpegEncodeArgs)
    assert _lib.SIGNATURES['istvt_png_decode_alone_u8'] == [dec, ctypes.c_int]
    assert _lib.SIGNATURES['istvt_png_decode_bank_alone_u8'] == [dec] + [ctypes.c_int] * 3
    assert _lib.SIGNATURES['istvt_png_decode_bank_alone_drawn_u8'] == [dec] + [ctypes.c_int] * 5
    assert _lib.SIGNATURES['istvt_png_encode_alone_u8'] == [enc] + [ctypes.c_int] * 4
    text = open(os.path.join(ROOT, 'include', 'istvt_hip.h')).read()
    assert '#define ISTVT_PNG_BAND_ALONE 0x80000000u' in text and clips.PNG_BAND_ALONE == 0x80000000
    for name in ('istvt_png_decode_alone_u8', 'istvt_png_decode_bank_alone_u8', 'istvt_png_decode_bank_alone_drawn_u8',
                 'istvt_png_encode_alone_u8'):
        assert hasattr(_lib.lib(), name)
    # the front end, before a device is asked for
    x = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r'png_encode_u8: alone=True needs index=True \(the flag lives in the band index\)'):
        ops.png_encode_u8(x, 8, alone=True)
    with pytest.raises(ValueError, match=r"encode_frames: alone= goes with format='png'"):
        ops.encode_frames(x, 8, torch.tensor([[0, 0, 16, 16]] * 2, dtype=torch.int32), alone=True)
