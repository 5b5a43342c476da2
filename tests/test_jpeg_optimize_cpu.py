"""JPEG files out with optimised Huffman tables (DESIGN.md "JPEG files out, optimised tables"), the host definition:
clips.jpeg_symbol_counts, clips.jpeg_optimal_table and clips.jpeg_encode_host(optimize=True) against what PIL wrote with
optimize=True (tests/golden/J4_jpeg_optimize.npz; no PIL needed here); the defining round trip; never more scan bytes; the
default unchanged; the properties of a table on synthetic counts; the refusals; tools/jpeg_entropy_opt_check.cpp, built plain,
on the recorded vectors."""
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'J4_jpeg_optimize.npz'))


def _case(name):
    """'17x33_s0_q75_rr1' -> (subsampling, quality, restart interval)"""
    parts = name.split('_')
    return {'s0': '444', 's2': '420'}[parts[-3 if parts[-1] == 'rr1' else -2]], \
        int(parts[-2 if parts[-1] == 'rr1' else -1][1:]), 'row' if parts[-1] == 'rr1' else 0


def _scan(clips, data):
    hd = clips.jpeg_parse(data)
    return hd, [hd.data[b:e] for b, e in hd.segments]


def test_tables_and_scans_equal_pil(clips, golden):
    names = [str(n) for n in golden['names']]
    assert len(names) == 49 and str(golden['limit']) in names
    for name in names:
        sub, q, ri = _case(name)
        x = torch.from_numpy(golden['frame_' + name])
        ours = clips.jpeg_encode_host(x, q, sub, ri, optimize=True)
        (hp, sp), (ho, so) = _scan(clips, bytes(golden['file_' + name])), _scan(clips, ours)
        assert ho.huffman == hp.huffman, name
        assert so == sp and ho.restart_interval == hp.restart_interval, name
        assert ho.huffman[0] != (clips.JPEG_STD_HUFFMAN[(0, 0)], clips.JPEG_STD_HUFFMAN[(1, 0)]), name


def test_the_limited_table(clips, golden):
    """the recorded 224 x 224 frame: a code length of 17 before the limiting, 16 after, and PIL's table"""
    name = str(golden['limit'])
    sub, q, ri = _case(name)
    hd = clips.jpeg_parse(bytes(golden['file_' + name]))
    rows = [i for i in range(golden['vec_counts'].shape[0])
            if max(clips.jpeg_code_lengths(golden['vec_counts'][i].tolist())[0]) > 16]
    tables = {clips.jpeg_optimal_table(golden['vec_counts'][i].tolist()) for i in rows}
    assert hd.huffman[1][1] in tables and hd.huffman[1][1][0][15] > 0


def test_round_trip_and_size(clips):
    """the defining property, on sizes with and without wholly outside luma blocks; never more scan bytes than the standard
    tables give; optimize=False is the call without the argument"""
    g = np.random.default_rng(29)
    for (h, w), sub, q, ri in (((17, 33), '420', 75, 0), ((8, 8), '420', 30, 'row'), ((24, 40), '444', 95, 5), ((1, 1), '444', 100, 1),
                               ((48, 72), '420', 90, 'row'), ((16, 16), '420', 50, 1)):
        x = torch.from_numpy(g.integers(0, 256, (h, w, 3), dtype=np.uint8) // 4 * (1 + (h > 16)))
        opt, std = clips.jpeg_encode_host(x, q, sub, ri, optimize=True), clips.jpeg_encode_host(x, q, sub, ri)
        assert std == clips.jpeg_encode_host(x, q, sub, ri, optimize=False) == clips.jpeg_encode_host(x, q, sub, ri, False)
        assert torch.equal(clips.jpeg_decode_host(opt), clips.jpeg_roundtrip_host(x[None], q, sub)[0]), (h, w, sub, q, ri)
        (ho, so), (hs, ss) = _scan(clips, opt), _scan(clips, std)
        assert len(so) == len(ss) and sum(map(len, so)) <= sum(map(len, ss)) and len(opt) < len(std)
        assert ho.segments[0][0] <= clips.jpeg_header_bound(h, w, sub, ri) == hs.segments[0][0]
    x = torch.from_numpy(g.integers(0, 256, (2, 16, 24, 3), dtype=np.uint8))
    files = clips.jpeg_encode_files_host(x, torch.tensor([40, 90], dtype=torch.int32), '444', 2, optimize=True)
    assert files == [clips.jpeg_encode_host(x[i], q, '444', 2, optimize=True) for i, q in enumerate((40, 90))]
    assert clips.jpeg_encode_files_host(x, 60) == clips.jpeg_encode_files_host(x, 60, optimize=False)


def test_header_places(clips):
    head = clips.jpeg_header(24, 40, 75, '420', 'row')
    lo, hi = clips.JPEG_HEADER_DHT
    assert head[lo:lo + 2] == b'\xff\xc4' and head[hi:hi + 2] == b'\xff\xdd' and head.count(b'\xff\xc4') == 4
    assert clips.jpeg_header(24, 40, 75, '444', 0)[hi:hi + 2] == b'\xff\xda'
    assert lo > clips.JPEG_HEADER_DQT[1] + 64 and clips.jpeg_header_bound(24, 40, '420', 'row') == len(head)


def _kraft(bits):
    return sum(n * 2 ** (16 - l) for l, n in enumerate(bits, 1))


def test_table_properties_on_synthetic_counts(clips, golden):
    """the recorded vectors (the files' histograms and the synthetic families) and families made here: every length <= 16, a
    Kraft sum below 1, a code for exactly the counted symbols, and the table recorded"""
    counts = [golden['vec_counts'][i].tolist() for i in range(golden['vec_counts'].shape[0])]
    g = np.random.default_rng(7)
    extra = [[int(v) for v in g.integers(0, 1 << 12, 256) * (g.random(256) < 0.3)] for _ in range(6)]
    a, b, fib = 1, 1, [0] * 256
    for k in range(30):
        fib[255 - k] = a
        a, b = b, a + b
    for i, c in enumerate(counts + extra + [fib]):
        bits, values = clips.jpeg_optimal_table(c)
        assert len(bits) == 16 and sum(bits) == len(values) <= 256
        assert sorted(values) == [s for s in range(256) if c[s]]
        if any(c):
            assert _kraft(bits) < 65536
            codes = clips._huffman_codes(bits, values)
            assert all(code != (1 << l) - 1 for code, l in codes.values())        # the all-ones code is free
        else:
            assert bits == (0,) * 16 and values == ()
        if i < len(counts):
            assert bits == tuple(golden['vec_bits'][i].tolist())
            assert values == tuple(golden['vec_values'][i][:int(golden['vec_total'][i])].tolist())
    lengths = [max(clips.jpeg_code_lengths(c)[0]) for c in counts]
    # limited tables are among them; the Fibonacci-like counts of depth 33, 40 and 47 had their counts halved to stay <= 32
    assert 16 < max(lengths) <= 32 and sum(16 < l for l in lengths) >= 3
    bits, values = clips.jpeg_optimal_table(fib)                                  # rarer symbols never get shorter codes
    codes = clips._huffman_codes(bits, values)
    assert all(codes[255 - k][1] >= codes[255 - k - 1][1] for k in range(29))
    # ties go to the larger symbol: of equal counts the smaller symbols get the shorter codes
    assert clips.jpeg_optimal_table([1 if s < 3 else 0 for s in range(256)]) == ((0, 3) + (0,) * 14, (0, 1, 2))
    assert clips.jpeg_optimal_table([5 if s == 9 else 0 for s in range(256)]) == ((1,) + (0,) * 15, (9,))


def test_symbol_counts_walk(clips):
    """two blocks by hand: a DC difference, a run of 17 zeros (ZRL), EOB; a prediction reset at the restart; clamps"""
    def blk(dc, **ac):
        b = [0] * 64
        b[0] = dc
        for k, v in ac.items():
            b[int(k[1:])] = v
        return b
    coef = [[[blk(5, k1=3, k19=-1), blk(5, k63=2)]]]
    dc0, ac0, dc1, ac1 = clips.jpeg_symbol_counts(coef, [(1, 1)], 1, 2, 0)
    assert {s: n for s, n in enumerate(dc0) if n} == {3: 1, 0: 1}
    assert {s: n for s, n in enumerate(ac0) if n} == {0x02: 1, 0xF0: 4, 0x11: 1, 0x00: 1, 0xE2: 1}
    assert not any(dc1) and not any(ac1)
    dc0, _, _, _ = clips.jpeg_symbol_counts(coef, [(1, 1)], 1, 2, 1)
    assert {s: n for s, n in enumerate(dc0) if n} == {3: 2}
    dc0, ac0, _, _ = clips.jpeg_symbol_counts([[[blk(-3000, k1=2000)]]], [(1, 1)], 1, 1, 0)
    assert dc0[11] == 1 and ac0[0x0A] == 1 and ac0[0] == 1


def test_refusals(clips):
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match='jpeg_encode_host: optimize'):
            clips.jpeg_encode_host(x, 75, '420', 0, optimize=bad)
    with pytest.raises(ValueError, match='256 non-negative counts'):
        clips.jpeg_optimal_table([1] * 255)
    with pytest.raises(ValueError, match='256 non-negative counts'):
        clips.jpeg_optimal_table([1] * 255 + [-1])
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import frames
    for bad in (1, None):                                         # before anything asks for a device
        with pytest.raises(ValueError, match='jpeg_encode_u8: optimize'):
            frames.jpeg_encode_u8(x[None], 75, optimize=bad)
        with pytest.raises(ValueError, match='jpeg_encode_u8: optimize'):
            frames.encode_frames(x[None], 8, boxes=torch.tensor([[0, 0, 8, 8]], dtype=torch.int32), optimize=bad)


def test_the_host_tool_builds_and_passes(tmp_path):
    """tools/jpeg_entropy_opt_check.cpp without sanitizers (the sanitizer build is a hand run: DESIGN.md has it) on the
    recorded vectors"""
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import build
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / 'jpeg_entropy_opt_check'
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', 'jpeg_entropy_opt_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), os.path.join(GOLDEN, 'J4_jpeg_optimize_vectors.txt')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == 'ok', r.stdout + r.stderr
    assert r.stdout.startswith('vectors: 230 tables equal') and len(r.stdout.splitlines()) == 8
