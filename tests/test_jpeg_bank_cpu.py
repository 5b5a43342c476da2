"""The JPEG bank (DESIGN.md "JPEG bank") on the CPU: clips.jpeg_bank against clips.jpeg_batch on the recorded files, the
definition clips.jpeg_bank_decode_host against the per-file decoder with the two new statuses, the host definition of the
device's marker scan against the parser's segments, JpegBank.extend with plain tensors, every refusal that needs no device,
the two new entry points against the header, and tools/jpeg_bank_check.cpp built plain."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_jpeg_split_cpu import _smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def recorded(golden_dir):
    """{layouts: [bytes]} of the sound recorded files: J2 by the default layouts, J2 and J3 together by 'all'"""
    j2 = np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))
    j3 = np.load(os.path.join(golden_dir, 'J3_jpeg_layouts.npz'))
    old = [bytes(j2['file_' + n]) for n in j2['names'].tolist()]
    new = [bytes(j3['file_' + n]) for n in j3['names'].tolist()]
    assert len(old) == 102 and len(new) > 100
    return {'default': old, 'all': old + new, 'cut': bytes(j2['file_damaged_cut'])}


def _encoded(clips):
    """jpeg_encode_host files of all four layouts with restart interval 0, 1 and 'row'"""
    x = _smooth(33, 50, 4)
    return [clips.jpeg_encode_host(x, 80, restart_interval=ri, layout=layout)
            for layout in clips.JPEG_LAYOUTS for ri in (0, 1, 'row')]


def test_bank_rows_are_the_batch_rows(clips, recorded):
    for layouts, files in ((clips.JPEG_LAYOUTS_DEFAULT, recorded['default']), ('all', recorded['all'])):
        bank, batch = clips.jpeg_bank(files, layouts), clips.jpeg_batch(files, layouts)
        for name in ('data', 'images', 'segments', 'qtabs', 'htabs'):
            assert torch.equal(getattr(bank, name), getattr(batch, name)), name
        assert bank.sizes == batch.sizes and len(bank) == bank.n == batch.n == len(files) and bank.nbytes == batch.nbytes
        assert (bank.nseg, bank.nq, bank.nh) == (batch.segments.shape[0], batch.qtabs.shape[0], batch.htabs.shape[0])
        headers = [clips.jpeg_parse(f, layouts) for f in files]
        assert bank.seg_max == max(len(h.segments) for h in headers) > 1
        most = max(h.mcus[0] * h.mcus[1] * len(h.mcu_blocks) for h in headers)
        assert bank.block_stride % clips.JPEG_IDCT_BLOCKS == 0 and 0 <= bank.block_stride - most < clips.JPEG_IDCT_BLOCKS
        assert (bank.Hmax, bank.Wmax) == (max(h.H for h in headers), max(h.W for h in headers))
        # the scratch: 192 bytes per block of every place, a status word per segment row and per place, the two planned tables
        for m in (1, 7):
            front = 192 * m * bank.block_stride + 4 * m * (bank.seg_max + 1)
            assert clips.jpeg_bank_scratch_bytes(bank, m) == -(-front // 16) * 16 + 80 * m + 20 * m * bank.seg_max
    assert clips.jpeg_bank(files[:3], 'all').on('cpu').segments.shape[1] == 5


def test_the_definition_is_the_per_file_decoder(clips, recorded):
    files = recorded['all'][::9] + [recorded['cut']]
    bank = clips.jpeg_bank(files, 'all')
    n = len(files)
    index = [n - 1, 0, 3, 3, -1, n, 5, -2 ** 40, 2 ** 31]
    canvas = (bank.Hmax + 3, bank.Wmax + 1)
    frames, sizes, status = clips.jpeg_bank_decode_host(bank, index, canvas)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (len(index),) + canvas + (3,)
    assert sizes.dtype == status.dtype == torch.int32
    seen = set()
    for j, i in enumerate(index):
        if not 0 <= i < n:
            assert status[j] == 4 and sizes[j].tolist() == [0, 0] and int(frames[j].max()) == 0
            continue
        ref, st = clips.jpeg_decode_host(files[i], return_status=True, layouts='all')
        h, w = ref.shape[:2]
        assert status[j] == st and sizes[j].tolist() == [h, w]
        assert torch.equal(frames[j, :h, :w], ref.to(torch.uint8))
        assert int(frames[j, h:].max()) == 0 and int(frames[j, :, w:].max()) == 0
        seen.add(st)
    assert seen == {0, 1}                                         # the cut file reports what the default call reports
    # the same from the files, as tensors of either width; an empty place is status 5
    holes = list(files)
    holes[3], holes[5] = b'', None
    for dtype in (torch.int32, torch.int64):
        idx = torch.tensor([0, 3, 5, n, 2], dtype=dtype)
        f2, s2, st2 = clips.jpeg_bank_decode_host(holes, idx, canvas, layouts='all')
        assert st2.tolist() == [0, 5, 5, 4, 0] and s2[1:4].tolist() == [[0, 0]] * 3 and int(f2[1:4].max()) == 0
        assert torch.equal(f2[0], frames[1]) and torch.equal(f2[4], clips.jpeg_bank_decode_host(bank, [2], canvas)[0][0])
    # the default canvas is the largest image of the set, whatever is drawn
    assert tuple(clips.jpeg_bank_decode_host(bank, [0])[0].shape[1:3]) == (bank.Hmax, bank.Wmax)
    with pytest.raises(ValueError, match='canvas'):
        clips.jpeg_bank_decode_host(bank, list(range(n)), (bank.Hmax - 1, bank.Wmax))


def test_status_names(clips):
    clips.check_jpeg_bank_status(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'place 2 has status 4 \(the index is outside the bank\)'):
        clips.check_jpeg_bank_status(torch.tensor([0, 0, 4, 5], dtype=torch.int32))
    with pytest.raises(ValueError, match=r'place 0 has status 5 \(the bank holds no decodable file at that place\)'):
        clips.check_jpeg_bank_status(torch.tensor([5], dtype=torch.int32))
    with pytest.raises(ValueError, match=r'place 1 is damaged \(status 1: its scan ends early\)'):
        clips.check_jpeg_bank_status(torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match=r'jpeg_decode: file 0 is damaged \(status 4: unknown\)'):   # the pinned text is as it was
        clips.check_jpeg_status(torch.tensor([4], dtype=torch.int32))


def test_marker_scan_gives_the_parsers_segments(clips, recorded):
    files = recorded['all'] + _encoded(clips)
    several = boundaries = 0
    for f in files:
        hd = clips.jpeg_parse(f, 'all')
        assert hd.eoi
        begin, end = hd.segments[0][0], hd.segments[-1][1]
        assert f[end:end + 2] == b'\xff\xd9'
        assert clips.jpeg_scan_segments_host(f, begin, end, len(hd.segments)) == hd.segments
        assert clips.jpeg_scan_segments_host(f, begin, end, len(hd.segments) + 1) is None
        several += len(hd.segments) > 1
        boundaries += any((e - begin) % clips.JPEG_SCAN_LANE_BYTES == clips.JPEG_SCAN_LANE_BYTES - 1 for _, e in hd.segments[:-1])
    assert several > 40 and boundaries > 3                        # files with markers, some of them across a lane's last byte
    # a scan cut short holds fewer intervals than its header promises: no table
    cut = clips.jpeg_parse(recorded['cut'])
    if len(cut.segments) > 1:
        assert clips.jpeg_scan_segments_host(cut.data, cut.segments[0][0], len(cut.data), len(cut.segments)) is None


def test_extend_rebases_the_second_bank(clips, recorded):
    one, two = recorded['all'][:40:3], recorded['all'][100:160:4]
    joined = clips.jpeg_bank(one, 'all').extend(clips.jpeg_bank(two, 'all'), device='cpu')
    whole = clips.jpeg_bank(one + two, 'all')
    a, b = joined.on('cpu'), whole.on('cpu')
    assert joined.data is None and joined.headers is None and str(joined.device) == 'cpu'
    assert (joined.n, joined.nbytes, joined.nseg, joined.seg_max, joined.block_stride, joined.Hmax, joined.Wmax, joined.sizes) == \
           (whole.n, whole.nbytes, whole.nseg, whole.seg_max, whole.block_stride, whole.Hmax, whole.Wmax, whole.sizes)
    assert torch.equal(a.data[:joined.nbytes], b.data[:whole.nbytes]) and torch.equal(a.segments, b.segments)
    # every column but the table slots is the packed one; the slots name equal tables (extend does not merge equal tables)
    cols = [0, 1, 2, 3, 4, 14, 15, 16, 17, 18, 19]
    assert torch.equal(a.images[:, cols], b.images[:, cols])
    assert torch.equal(a.qtabs[a.images[:, 5:8].long()], b.qtabs[b.images[:, 5:8].long()])
    assert torch.equal(a.htabs[a.images[:, 8:14].long()], b.htabs[b.images[:, 8:14].long()])
    assert joined.nq == a.qtabs.shape[0] and joined.nh == a.htabs.shape[0]
    with pytest.raises(ValueError, match='no host copy'):
        clips.jpeg_bank_decode_host(joined, [0])
    with pytest.raises(RuntimeError, match='no host copy to upload'):
        joined.on('meta')
    with pytest.raises(ValueError, match='joined on the `device`'):
        clips.jpeg_bank(one, 'all').extend(clips.jpeg_bank(two, 'all'))
    # an uploaded bank can let its host copies go: the uploaded tensors stay what a decode reads
    kept = clips.jpeg_bank(one, 'all')
    with pytest.raises(RuntimeError, match='upload the bank first'):
        kept.release_host()
    up = kept.on('cpu')
    kept.release_host()
    assert kept.data is None and kept.headers is None and kept.on('cpu') is up and str(kept.device) == 'cpu'


def test_refusals(clips, recorded):
    from istvt_amd import ops
    files = recorded['default'][:6]
    with pytest.raises(ValueError, match='jpeg_bank: an empty bank'):
        clips.jpeg_bank([])
    with pytest.raises(TypeError, match='sequence of files'):
        clips.jpeg_bank(files[0])
    with pytest.raises(ValueError, match=r'jpeg_parse: sampling 2x1/1x1/1x1'):          # the parser's text, not a new one
        clips.jpeg_bank([recorded['all'][102]])
    # 2^31 bytes through a faked length: a parsed file that claims a scan of 2^31 - 1 bytes, the most a bank holds, beside
    # real ones
    hd = clips.jpeg_parse(files[0])
    lo = hd.segments[0][0]
    fake = clips.JpegHeader(**dict(hd.__dict__, segments=[(lo, lo + 2 ** 31 - 1)]))
    with pytest.raises(ValueError, match=r'jpeg_bank: \d+ bytes; a bank holds fewer than 2\^31 .* use several banks'):
        clips.jpeg_bank(files + [fake])
    assert clips._bank_bytes(2 ** 31 - 1, 'x') == 2 ** 31 - 1
    small = clips.jpeg_bank(files)
    small.nbytes = 2 ** 31 - 1
    with pytest.raises(ValueError, match='JpegBank.extend: .* use several banks'):
        clips.jpeg_bank(files).extend(small, device='cpu')
    bank = clips.jpeg_bank(files)
    # the front end: what is wrong with the arguments is said before a device is asked for
    for split in (64, 'auto'):
        with pytest.raises(ValueError, match='split= is not available for a bank'):
            ops.jpeg_decode_indexed_u8(bank, [0], split=split)
        with pytest.raises(ValueError, match='split= is not available for a bank'):
            ops.decode_frames(bank, 16, index=[0], split=split)
    with pytest.raises(TypeError, match='expects a clips.JpegBank'):
        ops.jpeg_decode_indexed_u8(files, [0])
    with pytest.raises(ValueError, match='index must be contiguous'):
        ops.jpeg_decode_indexed_u8(bank, torch.arange(8, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match='index must be contiguous'):
        clips.jpeg_bank_decode_host(bank, torch.arange(8)[::2])
    with pytest.raises(ValueError, match='an empty index'):
        ops.jpeg_decode_indexed_u8(bank, [])
    for bad in (torch.zeros(2, dtype=torch.float32), torch.zeros((2, 2), dtype=torch.int32), 'ab', [0.5], [True]):
        with pytest.raises(TypeError, match='index is'):
            ops.jpeg_decode_indexed_u8(bank, bad)
    with pytest.raises(ValueError, match='decoded through index='):
        ops.decode_frames(bank, 16)
    with pytest.raises(ValueError, match='index= goes with a clips.JpegBank'):
        ops.decode_frames(files, 16, index=[0])
    # optimised files into the device ingest
    jf = clips.JpegFiles(torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    assert jf.geometry is None
    with pytest.raises(ValueError, match='needs H, W, layout and restart_interval'):
        clips.JpegBank.from_encoded(jf)
    jf.geometry = SimpleNamespace(H=16, W=16, layout='420', restart_interval=1, optimize=True)
    with pytest.raises(ValueError, match=r'optimised Huffman tables \(optimize=True\)'):
        clips.JpegBank.from_encoded(jf)
    with pytest.raises(TypeError, match='expects a clips.JpegFiles'):
        clips.JpegBank.from_encoded(files)
    jf.geometry.optimize = False
    with pytest.raises(ValueError, match='layout must be one of'):
        clips.JpegBank.from_encoded(jf, layout='411')
    with pytest.raises(RuntimeError, match='on one ROCm device'):
        clips.JpegBank.from_encoded(jf)


def test_entry_points_declared(clips):
    import abi_header as H
    from istvt_amd import _lib, frames, ops
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        text = fh.read()
    protos = H.prototypes(text)
    assert protos['istvt_jpeg_decode_indexed_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'm'), ('int', 'seg_max'),
                                                      ('int', 'block_stride'), ('int', 'Hmax'), ('int', 'Wmax')]
    assert protos['istvt_jpeg_bank_ingest'] == [('const istvt_jpeg_encode_args*', 'a'), ('int', 'layout')]
    I = ctypes.c_int
    assert _lib.SIGNATURES['istvt_jpeg_decode_indexed_u8'] == [ctypes.POINTER(_lib.JpegDecodeArgs), I, I, I, I, I]
    assert _lib.SIGNATURES['istvt_jpeg_bank_ingest'] == [ctypes.POINTER(_lib.JpegEncodeArgs), I]
    # no bare pointer: the argument blocks are typed, so tests/test_guard_cpu.py has nothing to decide for them
    for name in ('istvt_jpeg_decode_indexed_u8', 'istvt_jpeg_bank_ingest'):
        assert ctypes.c_void_p not in _lib.SIGNATURES[name]
    assert ops.jpeg_decode_indexed_u8 is frames.jpeg_decode_indexed_u8 and ops.jpeg_bank_ingest is frames.jpeg_bank_ingest
    assert H.defines(text)['ISTVT_JPEG_IDCT_BLOCKS'] == clips.JPEG_IDCT_BLOCKS
    assert clips.JPEG_SCAN_TILE_BYTES == 256 * clips.JPEG_SCAN_LANE_BYTES == 4096
    with open(os.path.join(os.path.dirname(frames.__file__), 'csrc', 'jpeg_bank_scan.h')) as fh:
        scan = fh.read()
    assert 'JB_LANE_BYTES = %d;' % clips.JPEG_SCAN_LANE_BYTES in scan and 'JB_TILE_BYTES = 256 * JB_LANE_BYTES;' in scan


def test_the_checker_built_plain(clips, tmp_path):
    """tools/jpeg_bank_check.cpp without sanitizers (the sanitizer build is a hand run: DESIGN.md has it)"""
    from istvt_amd import build
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / 'jpeg_bank_check'
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', 'jpeg_bank_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == 'ok' and len(lines) == 3, r.stdout + r.stderr
    assert lines[0].startswith('scan: ') and int(lines[0].split()[1]) > 2000 and lines[1] == 'plan: 12 places'
