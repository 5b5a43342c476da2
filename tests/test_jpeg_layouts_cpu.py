"""4:2:2 and greyscale JPEG files (DESIGN.md "JPEG layouts") on the CPU: clips.jpeg_decode_host(..., layouts='all') against
the bytes PIL's decoder (libjpeg-turbo) recorded in tests/golden/J3_jpeg_layouts.npz; the parser's geometry and refusals,
with and without the opt-in; the rows clips.jpeg_batch packs; clips.jpeg_split_host in the new layouts against a walk that
knows nothing of chunks; clips.jpeg_encode_layout_host; and the two host tools, built plain, on files of the new layouts."""
import os
import subprocess

import numpy as np
import pytest
import torch

from test_jpeg_split_cpu import _smooth

CHUNKS = (16, 37, 128)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TODAY_422 = 'jpeg_parse: sampling 2x1/1x1/1x1 .2x2/1x1/1x1 or 1x1/1x1/1x1 expected.'


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def files(golden_dir):
    return np.load(os.path.join(golden_dir, 'J3_jpeg_layouts.npz'))


@pytest.fixture(scope='module')
def j2(golden_dir):
    return np.load(os.path.join(golden_dir, 'J2_jpeg_files.npz'))


def test_the_definition_gives_pils_bytes(clips, files):
    names = files['names'].tolist()
    assert len(names) == 2 * 9 * 7 + 4 + 1
    for name in names:
        data = bytes(files['file_' + name])
        got, status = clips.jpeg_decode_host(data, return_status=True, layouts='all')
        want = torch.from_numpy(files['rgb_' + name])
        assert status == 0 and got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), name
        bad = int((got != want).sum())
        assert bad == 0, '%s: %d of %d bytes differ' % (name, bad, want.numel())
        layout = 'grey' if 'grey' in name else '422'
        assert torch.equal(clips.jpeg_decode_host(data, layouts=(layout,)), want), name
        if layout == 'grey':
            assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2]), name
    assert np.array_equal(files['rgb_grey_f22_24x40_q75'], files['rgb_24x40_grey_q75'])


def test_geometry(clips, files):
    def parsed(name):
        hd = clips.jpeg_parse(bytes(files['file_' + name]), 'all')
        return hd, (hd.layout, hd.mcus, hd.restart_interval, len(hd.segments))
    hd, got = parsed('9x15_422_q75')
    assert got == ('422', (2, 1), 0, 1) and (hd.factors, hd.sub, len(hd.quant), len(hd.huffman)) == ((2, 1), 2, 3, 3)
    assert hd.mcu_blocks == (0, 0, 1, 2)
    assert parsed('8x17_422_q75')[1] == ('422', (1, 2), 0, 1)
    hd, got = parsed('33x70_grey_q75')
    assert got == ('grey', (5, 9), 0, 1) and (hd.factors, hd.sub, len(hd.quant), len(hd.huffman)) == ((1, 1), 1, 1, 1)
    assert hd.mcu_blocks == (0,)
    assert parsed('grey_f22_24x40_q75')[1] == ('grey', (3, 5), 0, 1)      # the factors of a one-component file are ignored
    assert parsed('33x70_422_q75_rb1')[1] == ('422', (5, 5), 1, 25)
    assert parsed('33x70_422_q75_rr1')[1] == ('422', (5, 5), 5, 5)
    assert parsed('33x70_grey_q75_rb1')[1] == ('grey', (5, 9), 1, 45)
    assert parsed('33x70_grey_q75_rr1')[1] == ('grey', (5, 9), 9, 5)
    assert parsed('17x33_422_q75_rr1')[1] == ('422', (3, 3), 3, 3)


def test_the_old_layouts_parse_as_before(clips, j2):
    for name, layout, factors in (('17x33_s2_q75', '420', (2, 2)), ('17x33_s0_q75', '444', (1, 1))):
        for layouts in (clips.JPEG_LAYOUTS_DEFAULT, 'all'):
            hd = clips.jpeg_parse(bytes(j2['file_' + name]), layouts)
            assert (hd.layout, hd.factors, hd.sub) == (layout, factors, factors[0])
            assert hd.mcu_blocks == ((0, 0, 0, 0, 1, 2) if layout == '420' else (0, 1, 2))
    assert clips.JPEG_LAYOUTS == ('420', '444', '422', 'grey') and clips.JPEG_LAYOUTS_DEFAULT == ('420', '444')


def _sof(data, at, value, marker=None):
    """`data` with byte `at` behind its SOF0 marker set to `value`, or with the marker itself replaced"""
    out = bytearray(data)
    sof = data.index(b'\xff\xc0')
    if marker is not None:
        out[sof + 1] = marker
    else:
        out[sof + at] = value
    return bytes(out)


def test_refusals_with_all_layouts(clips, files, j2):
    f422, grey = bytes(files['file_24x40_422_q75']), bytes(files['file_24x40_grey_q75'])
    accepted = r'.2x2/1x1/1x1, 1x1/1x1/1x1 or 2x1/1x1/1x1 expected.'
    for value, name in ((0x12, '1x2/1x1/1x1'), (0x41, '4x1/1x1/1x1')):
        with pytest.raises(ValueError, match='jpeg_parse: sampling %s %s' % (name, accepted)):
            clips.jpeg_parse(_sof(f422, 11, value), 'all')
    with pytest.raises(ValueError, match='jpeg_parse: sampling 2x2/2x1/2x1 ' + accepted):
        clips.jpeg_parse(_sof(_sof(_sof(f422, 11, 0x22), 14, 0x21), 17, 0x21), 'all')
    # two and four components: the count byte and the segment's length edited together (the parser looks at the count first)
    for nf in (2, 4):
        with pytest.raises(ValueError, match='jpeg_parse: %d components .three expected: Y, Cb, Cr; or one.' % nf):
            clips.jpeg_parse(_sof(f422, 9, nf), 'all')
    for data in (f422, grey):
        with pytest.raises(ValueError, match='jpeg_parse: not baseline .SOF1.; baseline SOF0 expected'):
            clips.jpeg_parse(_sof(data, 0, 0, marker=0xC1), 'all')
    with pytest.raises(ValueError, match='jpeg_parse: progressive .SOF2.'):
        clips.jpeg_parse(bytes(j2['file_refused_progressive']), 'all')
    for bad in ('422', ('420', '411'), (), None, 3, ('all',), [422]):
        with pytest.raises(ValueError, match='jpeg_parse: layouts '):
            clips.jpeg_parse(f422, bad)
        with pytest.raises(ValueError, match='jpeg_batch: layouts '):
            clips.jpeg_batch([f422], bad)
    # a one-component file whose scan lists no component, and a cut SOS
    sos = grey.index(b'\xff\xda')
    with pytest.raises(ValueError, match='several scans: the first holds 3 of the 1 component '):
        clips.jpeg_parse(grey[:sos + 4] + b'\x03' + grey[sos + 5:], 'all')


def test_a_layout_that_was_not_asked_for_is_refused_as_it_always_was(clips, files, j2):
    f422, grey = bytes(files['file_24x40_422_q75']), bytes(files['file_24x40_grey_q75'])
    for layouts in (clips.JPEG_LAYOUTS_DEFAULT, ('420', '444', 'grey'), ('420',), ('grey',)):
        with pytest.raises(ValueError, match=TODAY_422):
            clips.jpeg_parse(f422, layouts)
    with pytest.raises(ValueError, match=TODAY_422):
        clips.jpeg_parse(f422)
    with pytest.raises(ValueError, match=TODAY_422):
        clips.jpeg_decode_host(f422)
    with pytest.raises(ValueError, match=TODAY_422):
        clips.jpeg_batch([bytes(j2['file_8x8_s2_q75']), f422])
    for layouts in (clips.JPEG_LAYOUTS_DEFAULT, ('420', '444', '422')):
        with pytest.raises(ValueError, match='jpeg_parse: 1 component .three expected: Y, Cb, Cr.$'):
            clips.jpeg_parse(grey, layouts)
    with pytest.raises(ValueError, match=r'jpeg_parse: sampling 2x2/1x1/1x1 .2x2/1x1/1x1 or 1x1/1x1/1x1 expected.'):
        clips.jpeg_parse(bytes(j2['file_8x8_s2_q75']), ('422', 'grey'))
    # the two files J2 holds as refused are these layouts
    assert clips.jpeg_parse(bytes(j2['file_refused_422']), 'all').layout == '422'
    assert clips.jpeg_parse(bytes(j2['file_refused_grey']), 'all').layout == 'grey'


def test_batch_rows(clips, files, j2):
    old = [bytes(j2['file_' + n]) for n in j2['names'].tolist()]
    a, b = clips.jpeg_batch(old), clips.jpeg_batch(old, layouts='all')
    for key in ('data', 'images', 'segments', 'qtabs', 'htabs'):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert (a.blocks, a.groups, a.nbytes, a.sizes) == (b.blocks, b.groups, b.nbytes, b.sizes)
    assert not bool(a.images[:, 19].any())
    names = ['9x15_422_q75', '33x70_grey_q75_rb1', '17x33_s2_q75', '8x17_422_q75_opt', 'grey_f22_24x40_q75', '17x33_s0_q75']
    mixed = [bytes((j2 if '_s' in n else files)['file_' + n]) for n in names]
    batch = clips.jpeg_batch(mixed, 'all')
    rows = batch.images.tolist()
    assert [r[19] for r in rows] == [1, 2, 0, 1, 2, 0] and [r[2] for r in rows] == [2, 1, 2, 2, 1, 1]
    assert [(r[4], r[3]) for r in rows] == [(2, 1), (5, 9), (2, 3), (1, 2), (3, 5), (3, 5)]
    per_mcu = [4, 1, 6, 4, 1, 3]
    assert [r[18] for r in rows] == [r[3] * r[4] * k for r, k in zip(rows, per_mcu)] == [8, 45, 36, 8, 15, 45]
    assert [r[14] for r in rows] == [0, 8, 53, 89, 97, 112] and batch.blocks == 157
    assert [r[15] for r in rows] == [0, 1, 3, 5, 6, 7] and batch.groups == 9
    assert [r[17] for r in rows] == [1, 45, 1, 1, 1, 1] and batch.segments.shape[0] == 50
    assert batch.scratch_bytes == 192 * 157 + 4 * 50
    for r in (rows[1], rows[4]):                                  # greyscale: the Cb and Cr slots repeat Y's
        assert r[5] == r[6] == r[7] and (r[8], r[9]) == (r[10], r[11]) == (r[12], r[13])
    assert all(0 <= v < batch.qtabs.shape[0] for r in rows for v in r[5:8])
    assert all(0 <= v < batch.htabs.shape[0] for r in rows for v in r[8:14])
    plan = clips.jpeg_split_plan(clips.jpeg_parse(mixed[0], 'all'), 16)
    assert plan.count == clips.jpeg_split_plan(clips.jpeg_batch(mixed[:1], 'all'), 16).count


def _walk(clips, hd):
    """One sequential walk per segment with clips._jpeg_block, the strict decoder, on a positioned reader that notes where
    every symbol starts -> per segment [(pos, bit, block number, first symbol of its block)], in order.  The blocks of an
    MCU are counted here from the layout's name alone."""
    seq = {'420': (0, 0, 0, 0, 1, 2), '444': (0, 1, 2), '422': (0, 0, 1, 2), 'grey': (0,)}[hd.layout]
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
        for block in range(len(seq) * min(ri, hd.mcus[0] * hd.mcus[1] - i * ri)):
            c = seq[block % len(seq)]
            dead, pred[c] = clips._jpeg_block(bits, tabs[c][0], tabs[c][1], pred[c], [0] * 64)
            assert dead == 0
        assert bits.status == 0
        out.append(symbols)
    return out


def test_split_states_counts_and_status(clips, files):
    seen_rounds, seen_blk = 0, set()
    for name in files['names'].tolist():
        hd = clips.jpeg_parse(bytes(files['file_' + name]), 'all')
        walk = _walk(clips, hd)
        nblk = 4 if hd.layout == '422' else 1
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
                    at = next((s for s in walk[i] if s[0] >= begin + j * seg.chunk), None)
                    if at is None:
                        assert pos >= begin + j * seg.chunk and seg.blocks[j] == 0, key
                        continue
                    assert (pos, bit, blk) == (at[0], at[1], at[2] % nblk) and (k == 0) == at[3], (key, j)
                    seen_blk.add((hd.layout, blk))
                seen_rounds = max(seen_rounds, seg.rounds)
    assert seen_rounds >= 2
    assert seen_blk == {('422', 0), ('422', 1), ('422', 2), ('422', 3), ('grey', 0)}
    # the lane cap: the 4:2:2 quality-100 noise scan is longer than 256 chunks of 16 bytes
    hd = clips.jpeg_parse(bytes(files['file_noise40x56_422_q100']), 'all')
    (begin, end), = hd.segments
    plan = clips.jpeg_split_plan(hd, 16)
    assert end - begin > 256 * 16 and plan.chunk[0] == -(-(end - begin) // 256) > 16 and plan.count[0] <= 256


def test_damaged_files_report_their_status(clips, files):
    want = dict(zip(files['damaged'].tolist(), files['damaged_status'].tolist()))
    assert sorted(want.values()) == [1, 2, 3]
    for name, status in want.items():
        data = bytes(files['file_' + name])
        hd = clips.jpeg_parse(data, 'all')
        assert hd.layout == '422' and (hd.H, hd.W) == (24, 40)
        assert clips.jpeg_decode_host(hd, return_status=True)[1] == status
        for chunk in CHUNKS:
            assert clips.jpeg_split_host(hd, chunk).status == status, (name, chunk)


@pytest.mark.parametrize('ri', [0, 1, 2, 5])
def test_encode_layout_host(clips, ri):
    x = _smooth(33, 70, 3370)
    for layout, mcus in (('422', 5 * 5), ('grey', 5 * 9)):
        data = clips.jpeg_encode_layout_host(x, 60, layout, ri)
        hd = clips.jpeg_parse(data, 'all')
        assert (hd.layout, hd.H, hd.W, hd.restart_interval, hd.eoi) == (layout, 33, 70, ri, True)
        assert len(hd.segments) == (-(-mcus // ri) if ri else 1)
        frame, status = clips.jpeg_decode_host(hd, return_status=True)
        assert status == 0 and tuple(frame.shape) == (33, 70, 3) and frame.dtype == torch.uint8
        # the file holds the quantised coefficients of the source: Y as it is, 4:2:2 chroma as the biased mean of pairs
        Y, Cb, Cr = clips._jpeg_colour_in(x[None], 8, 16 if layout == '422' else 8)
        qt = clips.jpeg_quant_tables(60)
        coef = clips._jpeg_coefficients(hd)[0]
        assert torch.equal(coef[0], clips._jpeg_quantise(Y, qt[:1])[0])
        if layout == '422':
            bias = (torch.arange(Cb.shape[2] // 2) & 1).to(torch.int32)
            assert torch.equal(coef[1], clips._jpeg_quantise((Cb[:, :, 0::2] + Cb[:, :, 1::2] + bias) >> 1, qt[1:])[0])
            assert torch.equal(coef[2], clips._jpeg_quantise((Cr[:, :, 0::2] + Cr[:, :, 1::2] + bias) >> 1, qt[1:])[0])
        else:
            assert len(coef) == 1 and torch.equal(frame[..., 0], frame[..., 2])
        assert clips.jpeg_split_host(hd, 16).status == 0
    with pytest.raises(ValueError, match="the layout is '422' or 'grey'"):
        clips.jpeg_encode_layout_host(x, 60, '420', ri)


def test_the_existing_encoder_keeps_its_bytes_and_refusals(clips):
    """jpeg_header and jpeg_encode_host were refactored around one scan writer: the header is the old literal"""
    head = clips.jpeg_header(33, 70, 75, '420', 3)
    sof = head.index(b'\xff\xc0')
    assert head[sof:sof + 19] == b'\xff\xc0\x00\x11\x08\x00\x21\x00\x46\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01'
    assert head[-14:] == b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    assert clips.jpeg_header(8, 8, 75, '444')[sof + 11] == 0x11
    for fn in (lambda: clips.jpeg_header(8, 8, 75, '422'), lambda: clips.jpeg_restart_interval(0, 8, '422'),
               lambda: clips.jpeg_encode_host(_smooth(8, 8, 1), 75, '422')):
        with pytest.raises(ValueError, match="subsampling must be '420' or '444'"):
            fn()


@pytest.mark.parametrize('tool', ['jpeg_entropy_check', 'jpeg_entropy_split_check'])
def test_the_checkers_built_plain(clips, files, tmp_path, tool):
    """the two host tools without sanitizers (the sanitizer builds are hand runs: DESIGN.md has them) on a 4:2:2 file, a
    greyscale file with a restart interval and a damaged 4:2:2 file"""
    from istvt_amd import build
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / tool
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', tool + '.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    paths = []
    for name in ('17x33_422_q75', '24x40_grey_q75_rr1', 'damaged422_code'):
        paths.append(str(tmp_path / (name + '.jpg')))
        with open(paths[-1], 'wb') as fh:
            fh.write(bytes(files['file_' + name]))
    r = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == 'ok', r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 4 and r.stdout.count('broken 0') == 3
    assert ' status 0' in lines[0] and ' status 0' in lines[1] and ' status 2' in lines[2]
    assert '3 segments' in lines[1]
