"""JPEG files without restart markers on the CPU: clips.jpeg_split_host, the host model of the split entropy
decode, on every fixture file -- its converged states against a walk with the strict decoder that knows nothing of chunks,
its block counts and statuses; clips.jpeg_split_plan; two conditions on the inputs without which the tests here and on the
GPU would exercise less than they claim; and tools/jpeg_entropy_split_check.cpp, built plain, on fixture files."""
import os
import subprocess

import numpy as np
import pytest
import torch

CHUNKS = (16, 37, 128)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def files(golden_dir):
    return np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))


def _smooth(h, w, seed):
    """the recipe of tests/golden/make_jpeg_golden.py"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return torch.from_numpy(np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8))


def _walk(clips, hd):
    """One sequential walk per segment with clips._jpeg_block, the strict decoder, on a positioned reader that notes where
    every symbol starts -> per segment [(pos, bit, block number, first symbol of its block)], in order"""
    nblk = 6 if hd.sub == 2 else 3
    tabs = [(clips.jpeg_huffman_table(*dc), clips.jpeg_huffman_table(*ac)) for dc, ac in hd.huffman]
    ri = hd.restart_interval or hd.mcus[0] * hd.mcus[1]
    out = []
    for i, (begin, end) in enumerate(hd.segments):
        symbols = []

        class Noting(clips._JpegPosBits):
            def huffman(self, t):
                symbols.append((self.pos, self.bit, block, not symbols or symbols[-1][2] != block))
                return super().huffman(t)
        bits = Noting(hd.data, end, begin, 0)
        pred = [0, 0, 0]
        for block in range(nblk * min(ri, hd.mcus[0] * hd.mcus[1] - i * ri)):
            c = (0, 0, 0, 0, 1, 2)[block % nblk] if hd.sub == 2 else block % nblk
            dead, pred[c] = clips._jpeg_block(bits, tabs[c][0], tabs[c][1], pred[c], [0] * 64)
            assert dead == 0
        assert bits.status == 0
        out.append(symbols)
    return out


def test_sound_files_states_counts_and_status(clips, files):
    names = files['names'].tolist()
    assert len(names) == 102
    seen_rounds = 0
    for name in names:
        hd = clips.jpeg_parse(bytes(files['file_' + name]))
        walk = _walk(clips, hd)
        nblk = 6 if hd.sub == 2 else 3
        ri = hd.restart_interval or hd.mcus[0] * hd.mcus[1]
        for chunk in CHUNKS:
            got = clips.jpeg_split_host(hd, chunk)
            assert got.status == 0, (name, chunk)
            for i, (seg, (begin, end)) in enumerate(zip(got.segments, hd.segments)):
                key = (name, chunk, i)
                assert seg.states[0] == (begin, 0, 0, 0), key
                assert sum(seg.blocks) == nblk * min(ri, hd.mcus[0] * hd.mcus[1] - i * ri), key
                assert seg.status == 0 and seg.rounds <= max(len(seg.states) - 1, 0), key
                assert seg.first == [sum(seg.blocks[:j]) for j in range(len(seg.blocks))], key
                for j, (pos, bit, blk, k) in enumerate(seg.states):
                    # the first symbol of the walk that starts at or after the boundary; behind the last symbol, the end
                    at = next((s for s in walk[i] if s[0] >= begin + j * seg.chunk), None)
                    if at is None:
                        assert pos >= begin + j * seg.chunk and seg.blocks[j] == 0, key
                        continue
                    assert (pos, bit, blk) == (at[0], at[1], at[2] % nblk) and (k == 0) == at[3], (key, j)
                seen_rounds = max(seen_rounds, seg.rounds)
    assert seen_rounds >= 2


def test_damaged_files_report_their_status(clips, files):
    want = dict(zip(files['damaged'].tolist(), files['damaged_status'].tolist()))
    assert sorted(want.values()) == [1, 2, 3]
    for name, status in want.items():
        data = bytes(files['file_' + name])
        assert clips.jpeg_decode_host(data, return_status=True)[1] == status
        for chunk in CHUNKS:
            assert clips.jpeg_split_host(data, chunk).status == status, (name, chunk)


def test_plan(clips, files):
    x = _smooth(64, 80, 1)
    data = [clips.jpeg_encode_host(x, 90, '444', 0), clips.jpeg_encode_host(x, 75, '420', 'row'),
            bytes(files['file_8x8_s2_q75']), bytes(files['file_damaged_cut'])]
    batch = clips.jpeg_batch(data)
    lengths = [e - b for _, b, e, _, _ in batch.segments.tolist()]
    assert max(lengths) == lengths[0] > 256 * 16                  # more than 256 chunks of 16 bytes: the cap holds
    for chunk in (16, 32, 64, 128, 4096):
        plan = clips.jpeg_split_plan(batch, chunk)
        assert len(plan.chunk) == len(plan.count) == len(plan.row0) == len(lengths)
        taken = []
        for s, (c, cnt, row0, (_, b, e, _, _)) in enumerate(zip(plan.chunk, plan.count, plan.row0, batch.segments.tolist())):
            assert c >= chunk >= 16 and 1 <= cnt <= 256
            assert b + (cnt - 1) * c <= e <= b + cnt * c and (cnt == 1 or b + (cnt - 1) * c < e)   # the last chunk ends at end
            assert 0 <= row0 and row0 + cnt <= plan.rows
            taken += range(row0, row0 + cnt)
        assert len(set(taken)) == len(taken)                      # no two segments share a row
        assert plan.states_at % 16 == 0 and plan.states_at >= batch.scratch_bytes
        assert plan.scratch_bytes == plan.states_at + 32 * plan.rows
    capped = clips.jpeg_split_plan(batch, 16)
    assert capped.chunk[0] == -(-lengths[0] // 256) > 16 and capped.count[0] == -(-lengths[0] // capped.chunk[0]) <= 256
    one = clips.jpeg_split_host(data[2], 4096)
    assert [len(s.states) for s in one.segments] == [1] and one.rounds == 0 and one.status == 0
    assert clips.jpeg_split_plan(clips.jpeg_parse(data[2]), 64).count == clips.jpeg_split_plan(clips.jpeg_batch([data[2]]), 64).count
    for bad in (8, 15, 1.5, '64', True, None):
        with pytest.raises(ValueError, match='at least 16'):
            clips.jpeg_split_plan(batch, bad)
        with pytest.raises(ValueError, match='at least 16'):
            clips.jpeg_split_host(data[2], bad)


def stuffed_boundaries(clips, files):
    """[(fixture name, chunk size)] among the noise fixtures and chunk sizes 16..48 where a chunk boundary falls on the 00
    stuffed behind an FF"""
    found = []
    for name in ('noise40x56_s%d_q%d' % (s, q) for s in (2, 0) for q in (50, 100)):
        hd = clips.jpeg_parse(bytes(files['file_' + name]))
        (begin, end), = hd.segments
        for chunk in range(16, 49):
            c = max(chunk, -(-(end - begin) // 256))
            if any(hd.data[at - 1] == 0xFF and hd.data[at] == 0 for at in range(begin + c, end, c)):
                found.append((name, chunk))
    return found


def test_conditions_on_the_inputs(clips, files):
    found = stuffed_boundaries(clips, files)
    assert found, 'no (noise fixture, chunk size) puts a boundary on a stuffed zero'
    name, chunk = found[0]
    hd = clips.jpeg_parse(bytes(files['file_' + name]))
    got = clips.jpeg_split_host(hd, chunk).segments[0]
    guessed = [j for j in range(1, len(got.states))
               if hd.data[hd.segments[0][0] + j * got.chunk] == 0 and hd.data[hd.segments[0][0] + j * got.chunk - 1] == 0xFF]
    assert guessed and all(got.states[j][0] > hd.segments[0][0] + j * got.chunk for j in guessed)
    # the relaxation loop runs: the 64 x 80 quality-75 4:2:0 encoder file needs at least two rounds at chunk 64
    data = clips.jpeg_encode_host(_smooth(64, 80, 1), 75, '420', 0)
    assert clips.jpeg_split_host(data, 64).rounds >= 2


def test_entry_point_and_row_width_declared(clips):
    import ctypes

    import abi_header as H
    from istvt_amd import _lib, frames, ops
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        text = fh.read()
    assert H.defines(text)['ISTVT_JPEG_STATE_INTS'] == clips.JPEG_STATE_INTS == 8
    assert H.prototypes(text)['istvt_jpeg_decode_split_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'chunk_bytes')]
    assert _lib.SIGNATURES['istvt_jpeg_decode_split_u8'] == [ctypes.POINTER(_lib.JpegDecodeArgs), ctypes.c_int]
    assert ops.jpeg_decode_u8 is frames.jpeg_decode_u8 and ops.decode_frames is frames.decode_frames
    assert clips.JPEG_SPLIT_MIN == 16 and clips.JPEG_SPLIT_DEFAULT >= clips.JPEG_SPLIT_MIN
    assert clips.JPEG_SPLIT_AUTO_BYTES > 2 * clips.JPEG_SPLIT_DEFAULT


def test_the_checker_built_plain(clips, files, tmp_path):
    """tools/jpeg_entropy_split_check.cpp without sanitizers (the sanitizer build is a hand run: DESIGN.md has it), on a
    restart-less file, one with a restart interval and one with optimised tables"""
    from istvt_amd import build
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / 'jpeg_entropy_split_check'
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', 'jpeg_entropy_split_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    paths = []
    for name in ('24x40_s2_q75', '17x33_s0_q75_rr1', '16x16_s2_q75_opt'):
        paths.append(str(tmp_path / (name + '.jpg')))
        with open(paths[-1], 'wb') as fh:
            fh.write(bytes(files['file_' + name]))
    r = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == 'ok', r.stdout + r.stderr
    assert len(r.stdout.splitlines()) == 4 and 'broken 0' in r.stdout
