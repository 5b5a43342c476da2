"""PNG windows (DESIGN.md "PNG windows") without a device: the definition clips.png_bank_window_host against the whole decode
for every box at every band edge; clips.png_window_rows is tight; the statuses and their precedence, with faults a box touches
and faults it does not; every refusal by name; what the three entries refuse before any launch, on host memory; the plain build
of tools/png_window_check.cpp on the vectors the definition writes for every call the GPU tests hand to a device; the ABI rows.
Everything is exact."""
import ctypes
import os
import subprocess

import pytest
import torch

import png_alone_cases as A
import png_window_cases as Wn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def test_the_definition(clips):
    """status 0: the window is rows [w0, w1) of png_decode_host with zeros elsewhere, and the crop of the window through the
    moved box is the crop of the frame through the box"""
    bank, frames = Wn.bank(clips), Wn.frames(clips)
    index, boxes, tags = Wn.places(clips)
    rows, Wc = bank.Hmax, bank.Wmax + 3
    windows, sizes, status, origin, moved = Wn.reference(clips, 'all_wide', bank, index, boxes, rows, Wc)
    assert status.tolist() == [0] * len(index) and len(index) > 60
    assert any(t.endswith('behind_row_64_of_band_1') for t in tags) and any(t.endswith('behind_row_64_of_band_0') for t in tags)
    for j, (i, box, tag) in enumerate(zip(index, boxes, tags)):
        H, W, _, R = Wn.files(clips)[i][2]
        kfirst, klast, w0, w1 = clips.png_window_plan(H, R, -(-H // R), box, rows, bank.band_max, W)
        assert (kfirst, klast, w0, w1) == (box[0] // R, (box[0] + box[2] - 1) // R, box[0] // R * R, min(H, ((box[0] + box[2] - 1) // R + 1) * R)), tag
        want = torch.zeros((rows, Wc, 3), dtype=torch.uint8)
        want[:w1 - w0, :W] = frames[i][w0:w1]
        assert torch.equal(windows[j], want), tag
        assert int(origin[j]) == w0 and moved[j].tolist() == [box[0] - w0, box[1], box[2], box[3]] and sizes[j].tolist() == [H, W], tag
        if max(box[2], box[3]) <= 8 * S:
            a = clips.crop_resize_host(windows[j][None], moved[j][None], S)
            b = clips.crop_resize_host(frames[i][None], torch.tensor([box], dtype=torch.int32), S)
            assert torch.equal(a, b), tag
    # one file, one box
    name, f, (H, W, _, R) = Wn.files(clips)[-1]
    win, w0, box, st = clips.png_decode_window_host(f, (137, 1, 7, 3), return_status=True)
    assert (tuple(win.shape), w0, box, st) == ((72, W, 3), 72, (65, 1, 7, 3), 0) and torch.equal(win, frames[-1][72:144])
    win, w0, box = clips.png_decode_window_host(f, (0, 0, 1, 1), rows=80, Wc=9)
    assert tuple(win.shape) == (80, 9, 3) and torch.equal(win[:72, :W], frames[-1][:72]) and not bool(win[72:].any()) and not bool(win[:, W:].any())


def test_window_rows_is_tight(clips):
    """a box of height h_max at y0 = R - 1 needs exactly png_window_rows where the image is tall enough, and no box of that
    height needs more"""
    for H, R in ((150, 72), (130, 100), (64, 1), (20, 8), (17, 5), (5, 16), (36, 8)):
        hd = clips.PngHeader(H=H, W=3, colour_type=2, bpp=3, data=b'', bands=(R, [2] * (-(-H // R) + 1)), alone=True)
        count = -(-H // R)
        for h_max in sorted({1, 2, R - 1, R, R + 1, 2 * R, H} - {0}):
            if h_max > H:
                continue
            rows = min(H, R * (1 + (h_max + R - 2) // R))
            need = 0
            for y0 in range(H - h_max + 1):
                plan = clips.png_window_plan(H, R, count, (y0, 0, h_max, 1), H, count)
                need = max(need, plan[3] - plan[2])
                assert clips.png_window_plan(H, R, count, (y0, 0, h_max, 1), rows, count) != 12, (H, R, h_max, y0)
            assert need <= rows
            if R - 1 + h_max <= H and R * (1 + (h_max + R - 2) // R) <= H:
                plan = clips.png_window_plan(H, R, count, (R - 1, 0, h_max, 1), H, count)
                assert plan[3] - plan[2] == rows == need, (H, R, h_max)
                assert rows == 1 or clips.png_window_plan(H, R, count, (R - 1, 0, h_max, 1), rows - 1, count) == 12
        del hd
    bank = Wn.bank(clips)
    want = max(min(H, R * (1 + (8 + R - 2) // R)) for _, _, (H, _, _, R) in Wn.files(clips))
    assert clips.png_window_rows(bank, 8) == want == 144
    batch = clips.png_batch([f for _, f, _ in Wn.files(clips)], bands='index', alone=True)
    assert clips.png_window_rows(batch, 8) == want and clips.png_window_bands(batch, 144) == clips.png_window_bands(bank, 144) == 64
    assert clips.png_window_bands(clips.png_bank([Wn.files(clips)[-1][1]], alone=True), 144) == 2
    assert clips.png_window_scratch_bytes(bank, 3, 16) == -(-(3 * clips.png_window_stride(bank, 16) + 12 * 16) // 16) * 16 + 60
    assert clips.png_window_stride(bank, 16) == -(-16 * (1 + 70 * 4) // 16) * 16


def test_statuses_and_their_precedence(clips):
    bank, index, boxes, want = Wn.fault_bank(clips)
    band = clips.png_decode_bands_host(A.damaged_file(clips), return_status=True)[1]
    lying_band = [s for n, _, s in A.lying_files(clips) if n == 'damaged_band_and_lying_row'][0]
    assert band not in (0, 6, 9, 10, 11, 12) and lying_band not in (0, 6, 9, 10, 11, 12)
    windows, sizes, status, origin, moved = Wn.reference(clips, 'faults', bank, index, boxes, 36, 29)
    named = Wn.fault_files(clips)
    sound = {n: clips.png_decode_host(f) for n, f, _ in named if n.startswith('fixed_') or n == 'row_0_alone_has_type_2'}
    whole = {seed: torch.from_numpy(__import__('png_streams').pattern(36, 25, 3, seed)) for seed in (191, 192, 193)}   # the sources
    assert all(torch.equal(f, whole[191]) for f in sound.values())
    for j, (i, box, w) in enumerate(zip(index, boxes, want)):
        name = named[i][0] if i < len(named) else 'without_the_flag'
        w = w if w is not None else (lying_band if name == 'damaged_band_and_lying_row' else band)
        assert int(status[j]) == w, (name, box)
        if w != 0:
            assert not bool(windows[j].any()) and int(origin[j]) == 0 and moved[j].tolist() == [0, 0, 1, 1], (name, box)
            assert sizes[j].tolist() == [36, 25] if name != 'without_the_flag' else sizes[j].tolist() == [37, 29]
            continue
        w0, w1 = box[0] // 8 * 8, min(36, ((box[0] + box[2] - 1) // 8 + 1) * 8)
        frame = sound[name] if name in sound else whole[{'damaged_band': 192, 'filter_5': 193}.get(name, 191)]
        assert torch.equal(windows[j, :w1 - w0, :25], frame[w0:w1]) and not bool(windows[j, w1 - w0:].any()), (name, box)
    # the whole decode sees the fault wherever it is
    for name, f, cases in named:
        if name != 'row_0_alone_has_type_2':                        # (Paeth on every row and a 5 in band 0: no band of it is sound)
            assert clips.png_decode_alone_host(f, return_status=True)[1] != 0, name
            assert name == 'filter_5_and_lying_row' or any(s == 0 for _, s in cases), name
    # 8, and each clause of 12
    one = clips.png_bank([named[0][1]], alone=True)
    clauses = Wn.outside_boxes(36, 25)
    got = clips.png_bank_window_host(one, [-1, 1] + [0] * len(clauses), [[0, 0, 1, 1]] * 2 + [list(b) for _, b in clauses], 8)
    assert got[2].tolist() == [8, 8] + [12] * len(clauses) and got[1].tolist() == [[0, 0]] * 2 + [[36, 25]] * len(clauses)
    assert not bool(got[0].any())
    two = clips.png_bank([named[-1][1]], alone=True)                # the filter-5 file, bands 1 and 2: 16 rows, 2 bands
    assert clips.png_bank_window_host(two, [0], [[8, 0, 16, 25]], 16)[2].tolist() == [0]
    assert clips.png_bank_window_host(two, [0], [[8, 0, 16, 25]], 15)[2].tolist() == [12]            # w1 - w0 > rows
    assert clips.png_window_plan(36, 8, 5, (8, 0, 16, 25), 16, 1, 25) == 12                              # more than win_bands bands
    assert clips.png_window_plan(36, 8, 5, (8, 0, 16, 25), 16, 2, 25) == (1, 2, 8, 24)
    assert clips.png_decode_window_host(named[0][1], (8, 0, 8, 25), return_status=True)[3] == 10         # the window's own first row
    # a bank packed without alone=True, and a file without the flag: 11
    plain = clips.png_bank([named[-1][1]])
    assert clips.png_bank_window_host(plain, [0], [[8, 0, 4, 4]], 8)[2].tolist() == [11]
    # the doctored banks: 9 at the doctored place, whatever the box; the others as they were
    b = Wn.bank(clips)
    for name, d, place in A.doctored(clips, b):
        H, W = b.sizes[place]
        got = clips.png_bank_window_host(d, [place, (place + 1) % b.n, place], [[0, 0, 1, 1], [0, 0, 1, 1], [H - 1, 0, 1, W]], b.Hmax)
        assert got[2].tolist() == [9, 0, 9] and got[1][0].tolist() == [0, 0] and not bool(got[0][0].any()) and bool(got[0][1].any()), name
    texts = {}
    for s in (11, 12):
        with pytest.raises(ValueError) as e:
            clips.check_png_status(torch.tensor([0, s]))
        texts[s] = str(e.value)
    assert 'file 1 is damaged (status 11: ' + clips.PNG_WINDOW_STATUS[11] in texts[11] and clips.PNG_WINDOW_STATUS[12] in texts[12]


def test_refusals_by_name(clips):
    from istvt_amd import ops
    named = Wn.files(clips)
    flagged = [f for _, f, _ in named[1:4]]
    plain = clips.png_encode_banded_host(__import__('png_streams').pattern(20, 31, 3, 5), 8, 'adaptive', index=True)
    batch = clips.png_batch(flagged, bands='index', alone=True)
    bank = clips.png_bank(flagged, alone=True)
    boxes = torch.tensor([[0, 0, 4, 4], [0, 0, 5, 9], [0, 0, 1, 70]], dtype=torch.int32)
    with pytest.raises(ValueError, match=r'decode_frames: window=True decodes through boxes=, one per frame'):
        ops.decode_frames(batch, S, window=True)
    with pytest.raises(ValueError, match=r'decode_frames: window=True goes with a clips.PngBatch or a clips.PngBank packed with alone=True; JPEG'):
        ops.decode_frames([b'\xff\xd8'], S, boxes, window=True)
    with pytest.raises(ValueError, match=r'draw_clips: window=True goes with a clips.PngBank packed with alone=True, got NoneType'):
        ops.draw_clips(None, None, S, window=True)
    with pytest.raises(ValueError, match=r'draw_clips: the bank was not packed with alone=True'):
        ops.draw_clips(clips.png_bank(flagged), None, S, window=True)
    with pytest.raises(TypeError, match=r'png_decode_window_u8 expects a clips.PngBatch or a clips.PngBank packed with alone=True, got list'):
        ops.png_decode_window_u8(flagged, boxes)
    with pytest.raises(ValueError, match=r"png_decode_window_u8: the batch was not packed with alone=True"):
        ops.png_decode_window_u8(clips.png_batch(flagged, bands='index'), boxes)
    with pytest.raises(ValueError, match=r'png_decode_window_u8: the bank was not packed with alone=True'):
        ops.png_decode_window_u8(clips.png_bank(flagged), boxes, index=[0, 1, 2])
    with pytest.raises(ValueError, match=r'png_decode_window_u8: file 1 of the batch does not say its bands stand alone'):
        ops.png_decode_window_u8(clips.png_batch([flagged[0], plain, flagged[2]], bands='index', alone=True), boxes)
    with pytest.raises(ValueError, match=r'png_decode_window_u8: a clips.PngBank is decoded through index='):
        ops.png_decode_window_u8(bank, boxes)
    with pytest.raises(ValueError, match=r'png_decode_window_u8: index= goes with a clips.PngBank'):
        ops.png_decode_window_u8(batch, boxes, index=[0, 1, 2])
    with pytest.raises(ValueError, match=r'png_decode_window_u8: boxes are int32 \(3, 4\) = \(y0, x0, h, w\), one per place, got torch.int32 \(2, 4\)'):
        ops.png_decode_window_u8(batch, boxes[:2])
    outside = boxes.clone()
    outside[1, 2] = 6
    with pytest.raises(IndexError, match=r'png_decode_window_u8: box 1, \(y0, x0, h, w\) = \(0, 0, 6, 9\), does not lie in its image of 5 x 9'):
        ops.png_decode_window_u8(batch, outside)
    with pytest.raises(IndexError, match=r'png_decode_window_u8: box 0, .* does not lie in its image of 5 x 9'):
        ops.png_decode_window_u8(bank, outside[1:2], index=[1])
    tall = boxes.clone()
    tall[0] = torch.tensor([7, 0, 2, 4])
    with pytest.raises(ValueError, match=r'png_decode_window_u8: box 0, \(y0, x0, h, w\) = \(7, 0, 2, 4\), needs a window of 16 rows \(its bands of 8 rows\), rows is 15'):
        ops.png_decode_window_u8(batch, tall, rows=15)
    for kw, word in ((dict(rows=0), 'rows'), (dict(rows=16385), 'rows'), (dict(canvas_w=0), 'canvas_w'), (dict(canvas_w=16385), 'canvas_w')):
        with pytest.raises(ValueError, match=r'png_decode_window_u8: %s lies in 1..16384, got' % word):
            ops.png_decode_window_u8(batch, boxes, **kw)
    with pytest.raises(ValueError, match=r'png_decode_window_u8: canvas_w holds the widest image \(70\), got 69'):
        ops.png_decode_window_u8(batch, boxes, canvas_w=69)
    assert clips.check_png_window(batch, tall)[1] == 16 and clips.check_png_window(batch, boxes)[1:] == (8, 70)      # a band of 8 rows, 5 and 1
    assert clips.check_png_window(bank, boxes, index=[0, 1, 2], rows=20, canvas_w=80)[1:] == (20, 80)
    with pytest.raises(ValueError, match=r'h and w must lie in \[1, 64\]'):      # a list of boxes is checked as a tensor is
        ops.decode_frames(batch, S, [[0, 0, 4, 4], [0, 0, 5, 9], [0, 0, 1, 70]], window=True)
    with pytest.raises(TypeError, match=r'png_decode_bank_window_drawn_u8 expects a clips.PngBank, got NoneType'):
        ops.png_decode_bank_window_drawn_u8(None, None)
    with pytest.raises(TypeError, match=r'png_decode_bank_window_drawn_u8 expects a clips.BatchPlan, got NoneType'):
        ops.png_decode_bank_window_drawn_u8(bank, None)


def test_the_entries_refuse_before_any_launch(clips):
    from istvt_amd import _lib
    assert Wn.entries_refuse(clips, _lib) > 40


def test_the_host_check(clips, tmp_path):
    """tools/png_window_check.cpp, built plain, on the vectors of every call the GPU tests hand to a device; a doctored status,
    a doctored window and a doctored band row fail.  DESIGN.md has its run under AddressSanitizer and UBSan."""
    from istvt_amd import build
    vectors = tmp_path / 'png_window_vectors.txt'
    lines, statuses = Wn.write_vectors(str(vectors), clips)
    places = [l for l in lines if l.startswith('P ')]
    assert len(lines) - len(places) == 6 + 4 + 3 and {0, 6, 8, 9, 10, 11, 12} <= statuses and len(statuses) == 8
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    exe = tmp_path / 'png_window_check'
    r = subprocess.run([clang, '-std=c++17', '-O1', '-I', build.CSRC, os.path.join(ROOT, 'tools', 'png_window_check.cpp'), '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith('png_window_check: %d places and ' % len(places)) and r.stdout.strip().endswith('waves agree'), \
        r.stdout + r.stderr
    table = next(l for l in lines if l.startswith('T faults '))
    # a place with another status
    line = next(l for l in lines if l.startswith('P faults:') and l.split(' ')[6] == '10')
    f = line.split(' ')
    (tmp_path / 'wrong.txt').write_text('%s\n%s\n' % (table, ' '.join(f[:6] + ['0'] + f[7:])))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'a wave has status 10, the definition has 0' in r.stdout, r.stdout
    # a place with another window
    line = next(l for l in lines if l.startswith('P faults:') and l.split(' ')[6] == '0' and l.split(' ')[7] == '0,0,0,8')
    f = line.split(' ')
    (tmp_path / 'wrong2.txt').write_text('%s\n%s\n' % (table, ' '.join(f[:7] + ['0,0,0,9'] + f[8:])))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong2.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'the window is rows 0 to 8, the definition has another' in r.stdout, r.stdout
    # a doctored band row under a place that claims status 0
    t = table.split(' ')
    bands = t[-1].split(',')
    bands[3] = '1'                                                 # band 0 of file 0 starts a byte late
    (tmp_path / 'wrong3.txt').write_text('%s\n%s\n' % (' '.join(t[:-1] + [','.join(bands)]), line))
    r = subprocess.run([str(exe), str(tmp_path / 'wrong3.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'a wave has status 9, the definition has 0' in r.stdout, r.stdout


def test_the_abi_rows(clips):
    from istvt_amd import _lib, ops
    dec = ctypes.POINTER(_lib.JpegDecodeArgs)
    assert _lib.SIGNATURES['istvt_png_decode_window_u8'] == [dec] + [ctypes.c_int] * 2
    assert _lib.SIGNATURES['istvt_png_decode_bank_window_u8'] == [dec] + [ctypes.c_int] * 5
    assert _lib.SIGNATURES['istvt_png_decode_bank_window_drawn_u8'] == [dec] + [ctypes.c_int] * 7
    for name in ('istvt_png_decode_window_u8', 'istvt_png_decode_bank_window_u8', 'istvt_png_decode_bank_window_drawn_u8'):
        assert hasattr(_lib.lib(), name)
    assert ops.png_decode_window_u8 is not None and ops.png_decode_bank_window_drawn_u8 is not None
    assert clips.PNG_WINDOW_STATUS.keys() == {11, 12}
