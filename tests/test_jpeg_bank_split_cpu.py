"""The split decode of a JPEG bank (DESIGN.md "JPEG bank, split") on the CPU: the bound chunk_rows against the chunk rule by
brute force, the scratch of split and non-split banks, with_split's shared tensors and cache, 'auto' on either side of its
threshold, extend's seg_bytes_max, every refusal that needs no device, the two new entry points against the header, and
tools/jpeg_bank_split_check.cpp built plain."""
import ctypes
import os
import subprocess

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
def files(golden_dir):
    j2 = np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))
    return [bytes(j2['file_' + n]) for n in j2['names'].tolist()]


@pytest.fixture(scope='module')
def long_file(clips):
    """64 x 80 at 4:4:4 and quality 90 without restart markers: one segment of more than 256 * 16 bytes"""
    return clips.jpeg_encode_host(_smooth(64, 80, 1), 90, '444', 0)


def test_chunk_rows_bounds_the_chunk_rule(clips, files):
    bank = clips.jpeg_bank(files[:3])
    # the rule itself, where it is not monotone: the 256-lane cap raises the chunk size
    assert clips.jpeg_split_chunks(4096, 16) == (16, 256) and clips.jpeg_split_chunks(4097, 16) == (17, 241)
    assert clips.jpeg_split_chunks(0, 16) == (16, 1) and clips.jpeg_split_chunks(1, 128) == (128, 1)
    batch = clips.jpeg_batch(files[:9])
    for chunk in (16, 48):
        plan = clips.jpeg_split_plan(batch, chunk)
        lengths = (batch.segments[:, 2] - batch.segments[:, 1]).tolist()
        assert list(zip(plan.chunk, plan.count)) == [clips.jpeg_split_chunks(n, chunk) for n in lengths]
    for chunk in (16, 37, 128):
        for L in (0, 1, chunk, chunk + 1, 255 * chunk + 1, 256 * chunk - 1, 256 * chunk, 256 * chunk + 1, 256 * chunk + 15 * chunk + 7,
                  300 * chunk):
            bank.seg_bytes_max = L
            rows = bank.with_split(chunk).chunk_rows
            assert rows == min(256, max(1, -(-L // chunk))) and 1 <= rows <= clips.JPEG_SPLIT_LANES
            most = max(clips.jpeg_split_chunks(n, chunk)[1] for n in range(L + 1))
            assert most <= rows, (chunk, L, most, rows)
            assert most == rows or L > 256 * chunk or L == 0, (chunk, L)      # and tight below the cap
    at_cap = clips.jpeg_split_chunks(4097, 16)[1]
    bank.seg_bytes_max = 4097
    assert bank.with_split(16).chunk_rows == 256 > at_cap                    # not the count at seg_bytes_max itself
    assert bank.chunk_rows is None and bank.split is None


def test_scratch_bytes(clips, files, long_file):
    bank = clips.jpeg_bank(files)
    assert bank.split is None and bank.seg_bytes_max == int((bank.segments[:, 2] - bank.segments[:, 1]).max())
    for m in (1, 7):
        front = 192 * m * bank.block_stride + 4 * m * (bank.seg_max + 1)
        plain = -(-front // 16) * 16 + 80 * m + 20 * m * bank.seg_max
        assert clips.jpeg_bank_scratch_bytes(bank, m) == clips.jpeg_bank_scratch_bytes(bank.with_split(None), m) == plain
        for chunk in (16, 128):
            split = bank.with_split(chunk)
            rows = split.chunk_rows
            assert rows == min(256, -(-bank.seg_bytes_max // chunk))
            assert clips.jpeg_bank_scratch_bytes(split, m) == -(-plain // 16) * 16 + 32 * m * bank.seg_max * rows
            assert clips.jpeg_bank_scratch_bytes(split, m) % 16 == 0
    assert clips.JPEG_STATE_INTS * 4 == 32
    capped = clips.jpeg_bank([long_file], split=16)
    assert capped.seg_bytes_max > 4096 and capped.chunk_rows == 256 and capped.seg_max == 1
    assert clips.jpeg_bank_scratch_bytes(capped, 3) - clips.jpeg_bank_scratch_bytes(capped.with_split(None), 3) in \
        range(32 * 3 * 256, 32 * 3 * 256 + 16)


def test_with_split_shares_the_bank(clips, files):
    bank = clips.jpeg_bank(files[:5])
    split = bank.with_split(64)
    assert isinstance(split, clips.JpegBank) and split is not bank and split.split == 64 and bank.split is None
    for name in ('data', 'images', 'segments', 'qtabs', 'htabs'):
        assert getattr(split, name) is getattr(bank, name), name
    assert split._on is bank._on and split.headers is bank.headers
    assert split.on('cpu') is bank.on('cpu') and list(bank._on) == ['cpu']   # uploaded once, seen by both
    back = split.with_split(None)
    assert back.split is None and back._on is bank._on and back.chunk_rows is None
    assert (split.n, split.nseg, split.seg_max, split.block_stride, split.seg_bytes_max) == \
        (bank.n, bank.nseg, bank.seg_max, bank.block_stride, bank.seg_bytes_max)
    assert clips.jpeg_bank(files[:5], split=64).split == 64 and len(split) == 5


def test_auto(clips, files, long_file):
    small = [f for f in files if max(e - b for b, e in clips.jpeg_parse(f).segments) <= clips.JPEG_SPLIT_AUTO_BYTES]
    assert 50 < len(small) < len(files)
    short = clips.jpeg_bank(small, split='auto')
    assert short.seg_bytes_max <= clips.JPEG_SPLIT_AUTO_BYTES and short.split is None
    assert clips.jpeg_bank(files, split='auto').split == 128        # the noise fixtures are one long segment each
    long_ = clips.jpeg_bank(small[:4] + [long_file], split='auto')
    assert long_.seg_bytes_max > clips.JPEG_SPLIT_AUTO_BYTES and long_.split == clips.JPEG_SPLIT_DEFAULT == 128
    assert long_.chunk_rows == -(-long_.seg_bytes_max // 128)
    assert short.with_split(32).with_split('auto').split is None and long_.with_split(None).with_split('auto').split == 128
    edge = clips.jpeg_bank(files[:2])
    edge.seg_bytes_max = clips.JPEG_SPLIT_AUTO_BYTES
    assert edge.with_split('auto').split is None
    edge.seg_bytes_max += 1
    assert edge.with_split('auto').split == 128


def test_extend(clips, files, long_file):
    a, b = clips.jpeg_bank(files[:3], split=32), clips.jpeg_bank([long_file], split=128)
    longest = max(a.seg_bytes_max, b.seg_bytes_max)
    assert b.seg_bytes_max == longest > a.seg_bytes_max
    a.extend(b, device='cpu')
    assert a.seg_bytes_max == longest and a.split == 32 and a.n == 4
    assert a.chunk_rows == min(256, -(-longest // 32))
    c, d = clips.jpeg_bank(files[:2]), clips.jpeg_bank(files[2:4], split=16)
    d.seg_bytes_max = None                                        # as an ingested bank whose caller named no bound
    c.extend(d, device='cpu')
    assert c.seg_bytes_max is None and c.split is None and c.with_split(16).chunk_rows == 256
    e = clips.jpeg_bank(files[:2], split=16)
    e.seg_bytes_max = None
    e.extend(clips.jpeg_bank(files[2:4]), device='cpu')
    assert e.seg_bytes_max is None and e.split == 16 and e.chunk_rows == 256


def test_refusals(clips, files, monkeypatch):
    """each by name and before a device is asked for"""
    from istvt_amd import ops
    bank = clips.jpeg_bank(files[:3])
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: (_ for _ in ()).throw(AssertionError('a device was asked for')))
    for bad in (8, 15, 1.5, 'row', True, 0, -16):
        with pytest.raises(ValueError, match=r"jpeg_bank: split is None, 'auto' or a chunk size in bytes \(an int of at least 16\)"):
            clips.jpeg_bank(files[:3], split=bad)
        with pytest.raises(ValueError, match=r"JpegBank.with_split: split is None, 'auto' or a chunk size in bytes"):
            bank.with_split(bad)
    ingested = clips.JpegBank(n=2, nseg=2, seg_max=1, block_stride=24, device='cuda:0')
    assert ingested.seg_bytes_max is None and ingested.with_split(64).chunk_rows == 256
    with pytest.raises(ValueError, match=r"JpegBank.with_split: split='auto' needs the longest interval of the bank.*seg_bytes_max="):
        ingested.with_split('auto')
    ingested.seg_bytes_max = 5000
    assert ingested.with_split('auto').split == 128 and ingested.with_split('auto').chunk_rows == 40
    jf = clips.JpegFiles(torch.zeros(64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    for bad in (0, -1, 2.5, True, '9'):
        with pytest.raises(ValueError, match='JpegBank.from_encoded: seg_bytes_max is None or a positive int'):
            clips.JpegBank.from_encoded(jf, 16, 16, '420', 0, seg_bytes_max=bad)
    # the call's own split= stays refused, for a split bank too, and says where the split goes
    for b in (bank, bank.with_split(64)):
        for split in (64, 'auto'):
            with pytest.raises(ValueError, match='split= is not available for a bank .*with_split'):
                ops.jpeg_decode_indexed_u8(b, [0], split=split)
            with pytest.raises(ValueError, match='split= is not available for a bank'):
                ops.decode_frames(b, 16, index=[0], split=split)


def test_entry_points_declared(clips):
    import abi_header as H
    from istvt_amd import _lib
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        protos = H.prototypes(fh.read())
    tail = [('int', 'seg_max'), ('int', 'block_stride'), ('int', 'Hmax'), ('int', 'Wmax'), ('int', 'chunk_bytes'),
            ('int', 'chunk_rows'), ('int', 'seg_bytes_max')]
    assert protos['istvt_jpeg_decode_indexed_split_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'm')] + tail
    assert protos['istvt_jpeg_decode_drawn_split_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'B'), ('int', 'T'),
                                                          ('int', 'block_ints')] + tail
    I = ctypes.c_int
    assert _lib.SIGNATURES['istvt_jpeg_decode_indexed_split_u8'] == [ctypes.POINTER(_lib.JpegDecodeArgs)] + [I] * 8
    assert _lib.SIGNATURES['istvt_jpeg_decode_drawn_split_u8'] == [ctypes.POINTER(_lib.JpegDecodeArgs)] + [I] * 10
    for name in ('istvt_jpeg_decode_indexed_split_u8', 'istvt_jpeg_decode_drawn_split_u8'):
        assert ctypes.c_void_p not in _lib.SIGNATURES[name]
    assert clips.JPEG_STATE_INTS == H.defines(open(os.path.join(ROOT, 'include', 'istvt_hip.h')).read())['ISTVT_JPEG_STATE_INTS']


def test_the_checker_built_plain(clips, tmp_path):
    """tools/jpeg_bank_split_check.cpp without sanitizers (the sanitizer build is a hand run: DESIGN.md has it)"""
    from istvt_amd import build
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / 'jpeg_bank_split_check'
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', 'jpeg_bank_split_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == 'ok' and len(lines) == 5, r.stdout + r.stderr
    assert lines[0].startswith('bank: 6 places, 11 segments')
    assert [ln.split(':')[0] for ln in lines[1:4]] == ['chunk 16', 'chunk 37', 'chunk 128']
    assert '256 rows per segment, 256 lanes' in lines[1] and '64 lanes' in lines[3]
    assert all('13 places, 16 segments decoded' in ln for ln in lines[1:4])
