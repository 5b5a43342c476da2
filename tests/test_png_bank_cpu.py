"""PNG bank (DESIGN.md "PNG bank") without a device: the rows clips.png_bank packs against clips.png_batch's; the definition
clips.png_bank_decode_host against the per-file definitions; the refusals that need no device; what the entry refuses before
any launch, on host memory; the plain build of tools/png_bank_check.cpp on the vectors the definition writes for every lookup
and every band the GPU tests hand to a device; a BatchPlan over a PngBank; the ABI rows."""
import ctypes
import os
import subprocess

import pytest
import torch

import png_bank_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def test_the_rows(clips):
    files = K.fixture_files(clips)
    for first in (0, 4096, 2 ** 32 + 16):
        bank, batch = clips.png_bank(files, first_byte=first), clips.png_batch(files, bands='index')
        im, ib = bank.images.tolist(), batch.images.tolist()
        assert bank.images.dtype == torch.int32 and tuple(bank.images.shape) == (len(files), clips.PNG_BANK_IMAGE_INTS) == (13, 10)
        assert [r[:4] for r in im] == [r[:4] for r in ib]                        # the geometry columns
        assert [r[7:] for r in im] == [r[6:8] + [0] for r in ib]                 # first band row, band count, 0
        assert [r[6] for r in im] == [r[5] - r[4] for r in ib]                   # stream bytes
        bases = [K.base_of(r) for r in im]
        assert all(b % 16 == 0 for b in bases) and bases == [r[4] + first for r in ib]
        rebased = [[f, b - ib[f][4], e - ib[f][4], o, nb] for f, b, e, o, nb in batch.bands.tolist()]
        assert bank.bands.tolist() == rebased and bank.nband == len(rebased) and bank.bands.dtype == torch.int32
        assert (bank.raw_stride, bank.Hmax, bank.Wmax) == (batch.raw_stride, 130, 111)
        assert bank.band_max == max(r[7] for r in ib) == 130 and bank.n == len(bank) == 13 and bank.first_byte == first
        assert bank.nbytes == batch.nbytes == int(bank.data.numel()) and bank.sizes == batch.sizes
        assert clips.png_bank_scratch_bytes(bank, 7) == 7 * bank.raw_stride + 4 * 7 * 130
    one = clips.png_bank(files, bands=None)
    assert one.band_max == 1 and one.nband == len(files) and one.bands[:, 1].tolist() == [0] * len(files)
    assert one.bands[:, 2].tolist() == one.images[:, 6].tolist()


def _expect(clips, refs, index, n, canvas):
    frames = torch.zeros((len(index), canvas[0], canvas[1], 3), dtype=torch.uint8)
    sizes, status = torch.zeros((len(index), 2), dtype=torch.int32), torch.zeros(len(index), dtype=torch.int32)
    for j, i in enumerate(index):
        if 0 <= i < n:
            f, s = refs[i]
            frames[j, :f.shape[0], :f.shape[1]] = f
            sizes[j, 0], sizes[j, 1], status[j] = f.shape[0], f.shape[1], s
        else:
            status[j] = 8
    return frames, sizes, status


def test_the_definition(clips):
    files, bank, refs = K.fixture_files(clips), K.fixture_bank(clips), K.reference(clips)
    n = bank.n
    assert [s for _, s in refs] == [0] * n
    for name, index in K.index_shapes(n):
        for dtype in (torch.int32, torch.int64):
            got = clips.png_bank_decode_host(bank, torch.tensor(index, dtype=dtype))
            want = _expect(clips, refs, index, n, (130, 111))
            assert all(torch.equal(g, w) for g, w in zip(got, want)), name
    got = clips.png_bank_decode_host(files, [n - 1, 0], canvas=(131, 120))        # a list of files, a list of ints, a canvas
    assert all(torch.equal(g, w) for g, w in zip(got, _expect(clips, refs, [n - 1, 0], n, (131, 120))))
    plain, s = clips.png_decode_host(files[-1], return_status=True)              # the file without an index: one band
    assert s == 0 and torch.equal(got[0][0, :23, :31], plain) and bank.images[n - 1, 8] == 1
    one = clips.png_bank(files, bands=None)                                        # packed as one band: png_decode_host's result
    got = clips.png_bank_decode_host(one, [5, 6])
    for j, i in enumerate((5, 6)):
        ref = clips.png_decode_host(files[i])
        assert torch.equal(got[0][j, :ref.shape[0], :ref.shape[1]], ref) and got[2][j] == 0
    wide = torch.tensor([0, -1, 1, n, 2 ** 32 + 3, 2], dtype=torch.int64)
    frames, sizes, status = clips.png_bank_decode_host(bank, wide)
    assert status.tolist() == [0, 8, 0, 8, 8, 0] and sizes[[1, 3, 4]].tolist() == [[0, 0]] * 3
    assert not bool(frames[[1, 3, 4]].any()) and torch.equal(frames[2, :5, :33], refs[1][0])
    # damaged and lying files: the statuses of png_decode_bands_host
    dam = K.damaged_files(clips)
    _, _, status = clips.png_bank_decode_host(K.damaged_bank(clips), list(range(len(dam))))
    assert status.tolist() == [clips.png_decode_bands_host(f, return_status=True)[1] for f in dam] and len(set(status.tolist())) >= 5
    assert clips.PNG_BANK_STATUS.keys() == {8, 9} and clips.PNG_BAND_STATUS.keys() == {7}
    for s, text in ((8, 'the index is outside the bank'), (9, "the bank's row for this place"), (7, 'the band index disagrees'),
                    (1, 'the stream ends early')):
        with pytest.raises(ValueError, match=r'png_decode: file 2 is damaged \(status %d: %s' % (s, text)):
            clips.check_png_status(torch.tensor([0, 0, s]))


def test_refusals(clips, monkeypatch):
    from istvt_amd import ops
    files = K.small_files(clips)
    with pytest.raises(ValueError, match='png_bank: an empty bank'):
        clips.png_bank([])
    with pytest.raises(ValueError, match='png_parse: the file does not start with the PNG signature'):
        clips.png_bank([files[0], b'JFIF' * 20])
    with pytest.raises(TypeError, match=r'png_bank expects a sequence of files \(bytes\), got bytes'):
        clips.png_bank(files[0])
    for bad in (-16, 8, 2 ** 31 + 1, 16.0, True):
        with pytest.raises(ValueError, match='png_bank: first_byte is a multiple of 16 and not negative'):
            clips.png_bank(files, first_byte=bad)
    with pytest.raises(ValueError, match=r"png_bank: bands is None or 'index', got 'rows'"):
        clips.png_bank(files, bands='rows')
    hd = clips.png_parse(files[0])
    huge = clips.PngHeader(H=hd.H, W=hd.W, colour_type=hd.colour_type, bpp=hd.bpp, bands=None, data=_Long(clips.PNG_MAX_BYTES))
    with pytest.raises(ValueError, match=r'png_bank: the stream of file 1 holds %d bytes; one file holds fewer' % clips.PNG_MAX_BYTES):
        clips.png_bank([hd, huge])
    bank = clips.png_bank(files)
    # the front end, before a device is asked for
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: pytest.fail('a device was asked for'))
    with pytest.raises(TypeError, match=r'png_decode_bank_u8 expects a clips.PngBank \(clips.png_bank\), got list'):
        ops.png_decode_bank_u8(files, [0])
    with pytest.raises(TypeError, match='png_decode_bank_u8: index is a list of ints or an int32 / int64 tensor'):
        ops.png_decode_bank_u8(bank, 'abc')
    with pytest.raises(ValueError, match='png_decode_bank_u8: an empty index'):
        ops.png_decode_bank_u8(bank, [])
    with pytest.raises(TypeError, match='png_decode_bank_u8: index is int32 or int64 of one dimension'):
        ops.png_decode_bank_u8(bank, torch.zeros(2, dtype=torch.float32))
    with pytest.raises(TypeError, match='png_decode_bank_drawn_u8 expects a clips.PngBank, got NoneType'):
        ops.png_decode_bank_drawn_u8(None, None)
    with pytest.raises(TypeError, match='png_decode_bank_drawn_u8 expects a clips.BatchPlan, got NoneType'):
        ops.png_decode_bank_drawn_u8(bank, None)
    plan = clips.BatchPlan(bank, [(0, 3, 0)], T=2, B=2, jpeg=None, perturb=None)
    with pytest.raises(RuntimeError, match='png_decode_bank_drawn_u8: the plan is drawn from where its draw block lives: upload it first'):
        ops.png_decode_bank_drawn_u8(bank, plan)
    with pytest.raises(RuntimeError, match='draw_clips: the plan is drawn from where its draw block lives: upload it first'):
        ops.draw_clips(None, plan, 16)
    with pytest.raises(RuntimeError, match='draw_clips: .* upload it first'):
        ops.draw_clips(bank, plan, 16)
    with pytest.raises(ValueError, match='decode_frames: a clips.PngBank is decoded through index='):
        ops.decode_frames(bank, 16)
    with pytest.raises(ValueError, match='decode_frames: split= and layouts= go with JPEG files; a clips.PngBank takes neither'):
        ops.decode_frames(bank, 16, index=[0], split=64)
    with pytest.raises(ValueError, match='decode_frames: split= and layouts= go with JPEG files; a clips.PngBank takes neither'):
        ops.decode_frames(bank, 16, index=[0], layouts=('420',))
    with pytest.raises(ValueError, match='index= goes with a clips.JpegBank'):
        ops.decode_frames(files, 16, index=[0])
    with pytest.raises(TypeError, match='jpeg_decode_drawn_u8 expects a clips.JpegBank, got PngBank'):
        ops.jpeg_decode_drawn_u8(bank, plan)
    with pytest.raises(TypeError, match='jpeg_decode_indexed_u8 expects a clips.JpegBank'):
        ops.jpeg_decode_indexed_u8(bank, [0])
    with pytest.raises(ValueError, match='png_bank_decode_host: the canvas 8 x 14 does not hold every image of the bank'):
        clips.png_bank_decode_host(bank, [0], canvas=(8, 14))


class _Long(bytes):
    """stands for a stream of `n` bytes without holding them"""

    def __new__(cls, n):
        self = super().__new__(cls, b'')
        self.n = n
        return self

    def __len__(self):
        return self.n


M, HC, WC = 3, 12, 14


def _block(clips, _lib, bank, scratch_bytes):
    room = torch.zeros(scratch_bytes + 48, dtype=torch.uint8)
    keep = dict(scratch=room[(-room.data_ptr()) % 16:], out=torch.zeros(M * HC * WC * 3, dtype=torch.uint8),
                sizes=torch.zeros((M, 2), dtype=torch.int32), status=torch.zeros(M, dtype=torch.int32),
                index=torch.tensor([2, 0, 2], dtype=torch.int32), images=bank.images.clone(), bands=bank.bands.clone())
    data = bank.data if bank.data.data_ptr() % 16 == 0 else None
    assert data is not None
    args = _lib.JpegDecodeArgs(bytes=data.data_ptr(), nbytes=bank.nbytes, images=keep['images'].data_ptr(),
                               images_host=keep['index'].data_ptr(), segments=keep['bands'].data_ptr(), segments_host=None, qtabs=None,
                               htabs=None, scratch=keep['scratch'].data_ptr(), scratch_bytes=scratch_bytes, out=keep['out'].data_ptr(),
                               sizes=keep['sizes'].data_ptr(), status=keep['status'].data_ptr(), stream=None, n=bank.n, nseg=bank.nband,
                               nq=0, nh=0, Hc=HC, Wc=WC)
    return args, keep


def test_the_entry_refuses_before_any_launch(clips):
    """a valid block on host memory, one thing made wrong per case, -3 back: nothing was launched then, which is why host
    memory will do.  The smallest scratch is written from the entry's own arithmetic."""
    from istvt_amd import _lib
    bank = clips.png_bank(K.small_files(clips))
    assert (bank.n, bank.band_max, bank.Hmax, bank.Wmax) == (3, 3, HC, WC) and bank.raw_stride % 16 == 0
    if bank.data.data_ptr() % 16:                                   # host memory at a multiple of 16, as a device's is
        room = torch.zeros(bank.nbytes + 16, dtype=torch.uint8)
        room = room[(-room.data_ptr()) % 16:][:bank.nbytes]
        room.copy_(bank.data)
        bank.data = room
    need = M * bank.raw_stride + 4 * M * bank.band_max
    assert need == clips.png_bank_scratch_bytes(bank, M)
    entry, drawn = _lib.lib().istvt_png_decode_bank_u8, _lib.lib().istvt_png_decode_bank_drawn_u8
    scalars = dict(m=M, band_max=bank.band_max, raw_stride=bank.raw_stride)
    cases = [('null_' + f, {f: None}, {}) for f in ('bytes', 'images', 'segments', 'images_host', 'scratch', 'out', 'sizes', 'status')]
    cases += [('m_0', {}, dict(m=0)), ('m_negative', {}, dict(m=-1)), ('band_max_0', {}, dict(band_max=0)),
              ('raw_stride_unaligned', {}, dict(raw_stride=bank.raw_stride + 8)), ('raw_stride_small', {}, dict(raw_stride=0)),
              ('raw_stride_8', {}, dict(raw_stride=8)), ('m_band_max_beyond_int', {}, dict(m=2 ** 20, band_max=2 ** 11)),
              ('scratch_one_byte_short', dict(scratch_bytes=need - 1), {}), ('scratch_unaligned', dict(scratch='+8'), {}),
              ('canvas_0', dict(Hc=0), {}), ('canvas_wide', dict(Wc=16385), {}), ('n_0', dict(n=0), {}), ('nseg_0', dict(nseg=0), {}),
              ('nbytes_negative', dict(nbytes=-1), {}), ('bytes_unaligned', dict(bytes='+8'), {})]
    assert len(cases) == 23
    for name, fields, extra in cases:
        args, keep = _block(clips, _lib, bank, need + 16)
        args.scratch_bytes = need
        for f, v in fields.items():
            setattr(args, f, getattr(args, f) + 8 if v == '+8' else v)
        s = dict(scalars, **extra)
        assert entry(ctypes.byref(args), s['m'], s['band_max'], s['raw_stride']) == -3, name
    assert entry(None, M, bank.band_max, bank.raw_stride) == -3
    # out inside the bank's bytes
    args, keep = _block(clips, _lib, bank, need)
    args.out = args.bytes
    assert entry(ctypes.byref(args), M, bank.band_max, bank.raw_stride) == -3
    # the drawn entry asks the draw's scalars first, then the bank decode's: nothing is drawn on a refusal of the first
    args, keep = _block(clips, _lib, bank, need)
    for B, T, ints in ((0, 3, 64), (1, 0, 64), (1, 3, 36 + 2)):
        assert drawn(ctypes.byref(args), B, T, ints, bank.band_max, bank.raw_stride) == -3
    assert drawn(None, 1, 3, 64, bank.band_max, bank.raw_stride) == -3


def test_the_host_check(clips, tmp_path):
    """tools/png_bank_check.cpp, built plain, on the vectors of every lookup and every band the GPU tests hand to a device;
    a doctored status and a doctored byte fail.  DESIGN.md has its run under AddressSanitizer and UBSan."""
    from istvt_amd import build
    vectors = tmp_path / 'png_bank_vectors.txt'
    nlook, nband, statuses, names = K.write_vectors(str(vectors), clips)
    assert nlook == 8 + len(names) and len(names) == 11 and nband == 248 and statuses >= {0, 1, 4, 5, 7}
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    exe = tmp_path / 'png_bank_check'
    r = subprocess.run([clang, '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(ROOT, 'tools', 'png_bank_check.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == 'png_bank_check: %d lookups and %d bands agree' % (nlook, nband), r.stdout + r.stderr
    lines = vectors.read_text().splitlines()
    # a lookup with another status
    at = next(i for i, l in enumerate(lines) if l.startswith('L doctored_count_0 '))
    head, status, bases = lines[at].rsplit(' ', 2)
    assert status.split(',')[0] == '9'
    (tmp_path / 'wrong0.txt').write_text('%s %s %s\n' % (head, ','.join(['0'] + status.split(',')[1:]), bases))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong0.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'place 0 has status 9, the definition has 0' in r.stdout
    # a band with another status, and one with another byte
    first = next(l for l in lines if l.startswith('B '))
    kind, name, status, rest = first.split(' ', 3)
    (tmp_path / 'wrong.txt').write_text('%s %s %d %s\n' % (kind, name, 7, rest))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong.txt')], capture_output=True, text=True, timeout=120)
    assert status == '0' and r.returncode == 1 and 'status 0, the definition has 7' in r.stdout
    head, want = first.rsplit(' ', 1)
    (tmp_path / 'wrong2.txt').write_text('%s %s%02x\n' % (head, want[:-2], int(want[-2:], 16) ^ 1))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong2.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'the bytes differ' in r.stdout


def test_a_plan_over_a_png_bank(clips):
    """BatchPlan reads a bank through .sizes alone: the index batch_draw_host draws, fed to the definition, gives the frames of
    those files"""
    bank, refs = K.fixture_bank(clips), K.reference(clips)
    plan = clips.BatchPlan(bank, [(0, 6, 0), (6, 7, 1)], T=3, B=4, K=16, seed=11)
    assert (plan.N, plan.Hmax, plan.Wmax) == (bank.n, bank.Hmax, bank.Wmax)
    listed = clips.BatchPlan(bank.sizes, [(0, 6, 0), (6, 7, 1)], T=3, B=4, K=16, seed=11)
    d = clips.batch_draw_host(plan, 3)
    assert torch.equal(d.index, clips.batch_draw_host(listed, 3).index) and d.index.numel() == 12
    index = d.index.tolist()
    assert all(0 <= i < bank.n for i in index) and len(set(index)) > 3
    got = clips.png_bank_decode_host(bank, d.index)
    assert all(torch.equal(g, w) for g, w in zip(got, _expect(clips, refs, index, bank.n, (130, 111))))


def test_the_abi_rows(clips):
    """the two entries in the ctypes table as the header declares them (tests/test_abi_cpu.py compares every row): the typed
    block and int scalars, no bare pointer"""
    from istvt_amd import _lib
    block = ctypes.POINTER(_lib.JpegDecodeArgs)
    assert _lib.SIGNATURES['istvt_png_decode_bank_u8'] == [block] + [ctypes.c_int] * 3
    assert _lib.SIGNATURES['istvt_png_decode_bank_drawn_u8'] == [block] + [ctypes.c_int] * 5
    text = open(os.path.join(ROOT, 'include', 'istvt_hip.h')).read()
    assert 'int istvt_png_decode_bank_u8(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride);' in text
    assert '#define ISTVT_PNG_BANK_IMAGE_INTS 10' in text and clips.PNG_BANK_IMAGE_INTS == 10
    for name in ('istvt_png_decode_bank_u8', 'istvt_png_decode_bank_drawn_u8'):
        assert hasattr(_lib.lib(), name)
