"""JPEG files (DESIGN.md "JPEG files") without a device: clips.jpeg_decode_host against PIL's recorded decode of every
fixture file, the parser's fields and refusals, the statuses of the damaged files, the encode / decode / round-trip identity,
the tables of a packed batch, and the entry point's declaration."""
import os

import numpy as np
import pytest
import torch

SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (24, 40), (33, 70), (48, 48))
VARIANTS = ('q30', 'q75', 'q95', 'q100', 'q75_opt', 'q75_rb1', 'q75_rr1')


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


def test_the_fixture_holds_every_case(files):
    names = set(files['names'].tolist())
    want = {'%dx%d_s%d_%s' % (h, w, s, v) for h, w in SIZES for s in (2, 0) for v in VARIANTS}
    want |= {'noise40x56_s%d_q%d' % (s, q) for s in (2, 0) for q in (50, 100)}
    assert names == want and len(names) == 102


def test_definition_equals_pil_on_every_sound_file(clips, files):
    for name in files['names'].tolist():
        got, status = clips.jpeg_decode_host(bytes(files['file_' + name]), return_status=True)
        ref = files['rgb_' + name]
        assert status == 0 and got.dtype == torch.uint8 and tuple(got.shape) == ref.shape, name
        assert np.array_equal(got.numpy(), ref), (name, int((got.numpy() != ref).sum()))
    assert torch.equal(clips.jpeg_decode_host(bytes(files['file_8x8_s2_q75'])), torch.from_numpy(files['rgb_8x8_s2_q75']))


def test_parser_fields_and_segments(clips, files):
    hd = clips.jpeg_parse(bytes(files['file_17x33_s2_q75']))
    assert (hd.H, hd.W, hd.sub, hd.mcus, hd.restart_interval, hd.eoi) == (17, 33, 2, (2, 3), 0, True)
    assert len(hd.segments) == 1 and len(hd.quant) == 3 and all(len(q) == 64 for q in hd.quant)
    q = clips.jpeg_quant_tables(75).reshape(2, 64).tolist()
    assert list(hd.quant[0]) == q[0] and list(hd.quant[1]) == q[1] and hd.quant[1] == hd.quant[2]
    std = clips.JPEG_STD_HUFFMAN
    assert hd.huffman == ((std[(0, 0)], std[(1, 0)]), (std[(0, 1)], std[(1, 1)]), (std[(0, 1)], std[(1, 1)]))
    assert clips.jpeg_parse(bytes(files['file_17x33_s2_q75_opt'])).huffman[0] != hd.huffman[0]
    hd = clips.jpeg_parse(bytes(files['file_17x33_s0_q75']))
    assert (hd.sub, hd.mcus) == (1, (3, 5))
    # one restart interval per MCU / per MCU row
    for name, sub, mcus, ri in (('33x70_s2_q75_rb1', 2, (3, 5), 1), ('33x70_s2_q75_rr1', 2, (3, 5), 5),
                                ('33x70_s0_q75_rb1', 1, (5, 9), 1), ('33x70_s0_q75_rr1', 1, (5, 9), 9),
                                ('1x1_s2_q75_rb1', 2, (1, 1), 1)):
        hd = clips.jpeg_parse(bytes(files['file_' + name]))
        assert (hd.sub, hd.mcus, hd.restart_interval) == (sub, mcus, ri), name
        assert len(hd.segments) == -(-mcus[0] * mcus[1] // ri), name
        assert all(b <= e for b, e in hd.segments) and all(a[1] + 2 == b[0] for a, b in zip(hd.segments, hd.segments[1:]))


def _refused(clips, data, text):
    with pytest.raises(ValueError) as ei:
        clips.jpeg_parse(data)
    assert str(ei.value).startswith('jpeg_parse: ') and text in str(ei.value), str(ei.value)


def _find(data, marker):
    return data.index(bytes([0xFF, marker]))


def test_every_refusal(clips, files):
    base = bytes(files['file_24x40_s2_q75'])
    _refused(clips, bytes(files['file_refused_progressive']), 'progressive')
    _refused(clips, bytes(files['file_refused_422']), 'sampling 2x1/1x1/1x1')
    _refused(clips, bytes(files['file_refused_grey']), '1 component ')
    sof, dqt, dht, sos = _find(base, 0xC0), _find(base, 0xDB), _find(base, 0xC4), _find(base, 0xDA)

    def edit(at, *values):
        return base[:at] + bytes(values) + base[at + len(values):]
    _refused(clips, edit(sof + 1, 0xC1), 'not baseline (SOF1)')
    _refused(clips, edit(sof + 4, 12), '12-bit precision')
    _refused(clips, edit(dqt + 4, 0x10), '16-bit quantisation table')
    _refused(clips, edit(sof + 9, 4), '4 components')
    _refused(clips, edit(sof + 5, 0, 0), 'zero width or height')
    _refused(clips, edit(sof + 7, 0, 0), 'zero width or height')
    _refused(clips, edit(sof + 5, 0x40, 0x01), 'a side above 16384')
    _refused(clips, edit(sof + 12, 3), 'quantisation table 3, which the file never defines')
    _refused(clips, edit(sos + 6, 0x30), 'DC Huffman table 3, which the file never defines')
    _refused(clips, edit(sos + 6, 0x02), 'AC Huffman table 2, which the file never defines')
    adobe = b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00'
    _refused(clips, base[:2] + adobe + b'\x00' + base[2:], 'Adobe APP14 segment with transform 0')
    assert clips.jpeg_parse(base[:2] + adobe + b'\x01' + base[2:]).H == 24              # transform 1 is YCbCr: fine
    assert clips.jpeg_parse(base[:2] + b'\xff\xfe\x00\x05abc' + base[2:]).W == 40        # a comment is skipped
    _refused(clips, base[:sos], 'no SOS')
    _refused(clips, base[:sos] + b'\xff\xd9', 'no SOS')
    _refused(clips, b'\x00\x01\x02\x03', 'does not start with SOI')
    eoi = len(base) - 2
    assert base[eoi:] == b'\xff\xd9'
    _refused(clips, base[:eoi] + base[sos:], 'several scans')
    _refused(clips, edit(sos + 4, 1), 'several scans')
    # restart markers: out of sequence, too many, too few
    rr = bytes(files['file_33x70_s2_q75_rr1'])
    first = rr.index(b'\xff\xd0', _find(rr, 0xDA))
    _refused(clips, rr[:first + 1] + b'\xd1' + rr[first + 2:], 'restart markers out of sequence')
    second = rr.index(b'\xff\xd1', first)
    _refused(clips, rr[:first] + rr[second:], 'restart markers out of sequence')
    dri = _find(rr, 0xDD)
    _refused(clips, rr[:dri + 5] + b'\x03' + rr[dri + 6:], '3 restart intervals in the scan, 5 expected')
    _refused(clips, base[:eoi] + b'\xff\xd0' + base[eoi:], '2 restart intervals in the scan, 1 expected')
    for bad in (b'', b'\xff\xd8'):
        _refused(clips, bad, 'SOI')


def test_a_scan_without_eoi_is_no_refusal(clips, files):
    base = bytes(files['file_24x40_s2_q75'])
    hd = clips.jpeg_parse(base[:-2])
    assert not hd.eoi and hd.segments[0][1] == len(base) - 2
    assert torch.equal(clips.jpeg_decode_host(base[:-2]), torch.from_numpy(files['rgb_24x40_s2_q75']))
    rr = bytes(files['file_33x70_s2_q75_rr1'])
    cut = rr.index(b'\xff\xd1')                                    # the third restart interval is gone: an empty segment
    hd = clips.jpeg_parse(rr[:cut])
    assert not hd.eoi and len(hd.segments) == 3 and hd.segments[1][1] == cut and hd.segments[2] == (cut, cut)
    out, status = clips.jpeg_decode_host(hd, return_status=True)
    assert status == 1 and torch.equal(out[:16], torch.from_numpy(files['rgb_33x70_s2_q75_rr1'])[:16])


def test_damaged_files_report_their_status(clips, files):
    base = bytes(files['file_24x40_s2_q75'])
    assert files['damaged'].tolist() == ['damaged_code', 'damaged_cut', 'damaged_run']
    assert files['damaged_status'].tolist() == [2, 1, 3]
    for name, want, (at, value) in zip(files['damaged'].tolist(), files['damaged_status'].tolist(), files['damaged_edit'].tolist()):
        data = bytes(files['file_' + name])
        assert data == (base[:at] if name == 'damaged_cut' else base[:at] + bytes([value]) + base[at + 1:])
        out, status = clips.jpeg_decode_host(data, return_status=True)
        assert status == want and tuple(out.shape) == (24, 40, 3), name
    import istvt_pkg
    istvt_pkg.load()
    with pytest.raises(ValueError, match='file 1 is damaged .status 3'):
        clips.check_jpeg_status(torch.tensor([0, 3, 1], dtype=torch.int32))
    clips.check_jpeg_status(torch.zeros(4, dtype=torch.int32))


@pytest.mark.parametrize('h,w', [(16, 16), (17, 33), (24, 40)])
def test_encode_decode_is_the_round_trip(clips, h, w):
    x = _smooth(h, w, 100 * h + w)
    for sub in ('420', '444'):
        for q in (30, 90):
            ref = clips.jpeg_roundtrip_host(x[None], q, sub)[0]
            for ri in (0, 2):
                data = clips.jpeg_encode_host(x, q, sub, ri)
                hd = clips.jpeg_parse(data)
                mcus = hd.mcus[0] * hd.mcus[1]
                assert (hd.H, hd.W, hd.sub, hd.restart_interval) == (h, w, clips.JPEG_SUBSAMPLINGS[sub], ri)
                assert len(hd.segments) == (-(-mcus // ri) if ri else 1)
                got, status = clips.jpeg_decode_host(hd, return_status=True)
                assert status == 0 and torch.equal(got, ref), (sub, q, ri)


def test_batch_tables_and_whole_boxes(clips, files):
    names = ['17x33_s2_q75', '33x70_s0_q75_rr1', '17x33_s2_q30', '8x8_s2_q75_opt']
    data = [bytes(files['file_' + k]) for k in names]
    b = clips.jpeg_batch(data)
    assert b.n == 4 and b.sizes == [(17, 33), (33, 70), (17, 33), (8, 8)]
    assert b.images.dtype == torch.int32 and tuple(b.images.shape) == (4, clips.JPEG_IMAGE_INTS)
    hds = [clips.jpeg_parse(d) for d in data]
    # H, W, chroma step, MCU columns, MCU rows
    assert b.images[:, :5].tolist() == [[17, 33, 2, 3, 2], [33, 70, 1, 9, 5], [17, 33, 2, 3, 2], [8, 8, 2, 1, 1]]
    # two quality-75 tables, two quality-30 tables; the optimised file brings four Huffman tables of its own
    assert b.images[:, 5:8].tolist() == [[0, 1, 1], [0, 1, 1], [2, 3, 3], [0, 1, 1]]
    assert b.images[:, 8:14].tolist() == [[0, 1, 2, 3, 2, 3]] * 3 + [[4, 5, 6, 7, 6, 7]]
    assert tuple(b.qtabs.shape) == (4, 64) and tuple(b.htabs.shape) == (8, clips.JPEG_HUFF_INTS)
    assert b.qtabs[0].tolist() == list(hds[0].quant[0]) and b.qtabs[3].tolist() == list(hds[2].quant[1])
    assert b.htabs[1].tolist() == clips.jpeg_huffman_table(*clips.JPEG_STD_HUFFMAN[(1, 0)])
    # blocks (6 per 4:2:0 MCU, 3 per 4:4:4 MCU), IDCT workgroups of 24 blocks, segments
    blocks = [36, 135, 36, 6]
    assert b.images[:, 18].tolist() == blocks and b.images[:, 14].tolist() == [0, 36, 171, 207] and b.blocks == 213
    assert b.images[:, 15].tolist() == [0, 2, 8, 10] and b.groups == 11
    assert b.images[:, 16].tolist() == [0, 1, 6, 7] and b.images[:, 17].tolist() == [1, 5, 1, 1]
    assert b.scratch_bytes == 192 * 213 + 4 * 8
    seg = b.segments.tolist()
    assert len(seg) == 8 and [s[0] for s in seg] == [0, 1, 1, 1, 1, 1, 2, 3]
    assert [s[3:] for s in seg[1:6]] == [[0, 9], [9, 9], [18, 9], [27, 9], [36, 9]] and seg[0][3:] == [0, 6]
    at = 0
    for i, hd in enumerate(hds):                                  # the scan bytes, end to end
        lo, hi = hd.segments[0][0], hd.segments[-1][1]
        assert bytes(b.data[at:at + hi - lo].tolist()) == data[i][lo:hi]
        mine = [s for s in seg if s[0] == i]
        assert [(s[1] - at, s[2] - at) for s in mine] == [(x - lo, y - lo) for x, y in hd.segments]
        at += hi - lo
    assert b.nbytes == at
    # the Huffman decode form: every code of a table finds its value
    counts, values = clips.JPEG_STD_HUFFMAN[(1, 1)]
    t = clips.jpeg_huffman_table(counts, values)
    for value, (code, length) in clips._huffman_codes(counts, values).items():
        c = (code << (16 - length)) | ((1 << (16 - length)) - 1)
        l = next(k for k in range(1, 17) if c < t[k - 1])
        assert l == length and t[32 + ((t[16 + l - 1] + (c >> (16 - l))) & 255)] == value
    assert clips.whole_boxes(b.sizes).tolist() == [[0, 0, 17, 33], [0, 0, 33, 70], [0, 0, 17, 33], [0, 0, 8, 8]]
    assert clips.whole_boxes(b.sizes).dtype == torch.int32
    with pytest.raises(ValueError, match='empty'):
        clips.jpeg_batch([])
    with pytest.raises(ValueError, match='jpeg_parse: progressive'):
        clips.jpeg_batch([data[0], bytes(files['file_refused_progressive'])])


def test_entry_point_declared_and_exported(clips):
    import ctypes
    from istvt_amd import _lib, frames, ops
    # (header, table, argument block and library: test_abi_cpu.py)
    assert ops.jpeg_decode_u8 is frames.jpeg_decode_u8 and ops.decode_frames is frames.decode_frames
    assert _lib.lib().istvt_jpeg_decode_u8(None) == -3                                   # no block: refused, nothing launched
    args = _lib.JpegDecodeArgs(n=1, nseg=1, nq=1, nh=1, Hc=8, Wc=8)
    assert _lib.lib().istvt_jpeg_decode_u8(ctypes.byref(args)) == -3                     # null pointers
