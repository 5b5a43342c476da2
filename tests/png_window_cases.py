"""Files, boxes, banks and vectors for the tests of PNG windows (test_png_window_cpu.py, test_png_window_gpu.py; no tests in
here): the flagged files of png_alone_cases and one of 150 x 5 grey at R = 72, the boxes at the band edges of each, files whose
faults a box touches or does not touch, the doctored banks, and the vectors of tools/png_window_check.cpp written from the
definition.  Only tables, boxes and rows that program has walked go to a device: the GPU tests take them from here and nowhere
else."""
import numpy as np
import torch

import png_alone_cases as A
import png_streams as P

_CACHE = {}
TALL = (150, 5, 1, 72)                                            # (H, W, channels, R): three bands, the last of 6 rows
FAULT = (36, 25, 3, 8)                                            # the shape of png_alone_cases' lying and damaged files


def files(clips):
    """[(name, flagged file, (H, W, channels, R))]: png_alone_cases.ALONE's and the 150-row one"""
    if 'files' not in _CACHE:
        H, W, ch, R = TALL
        tall = clips.png_encode_banded_host(P.pattern(H, W, ch, 171), R, 'adaptive', index=True, alone=True)
        _CACHE['files'] = [(n, f, s) for (n, f), s in zip(A.alone_files(clips), A.ALONE)] + [('%dx%dx%d_r%d' % TALL, tall, TALL)]
    return _CACHE['files']


def boxes_of(H, W, R):
    """[(tag, (y0, x0, h, w))] of one file: a whole band exactly, a box that ends on a band edge and one a row over it, one row
    in the last band, the whole image, a box inside the columns, and for the files of 130 and 150 rows a box that lies wholly
    behind row 64 of its band -- band 1 of the 150-row file (rows 72 to 143), and band 0 of those of 130 rows, whose band 1 has
    no such row"""
    count = -(-H // R)
    k = 1 if count > 2 or (count == 2 and H >= 2 * R) else 0
    out = [('whole_band', (k * R, 0, min(R, H - k * R), W))]
    if count > 1:
        edge = (count - 1) * R if count == 2 else 2 * R
        top = max(0, edge - 3)
        out += [('ends_on_an_edge', (top, 0, edge - top, W)), ('one_row_over_the_edge', (top, 0, edge - top + 1, W))]
    out += [('one_row_in_the_last_band', (H - 1, 0, 1, W)), ('whole_image', (0, 0, H, W))]
    if W >= 3:
        out.append(('inside_the_columns', (min(H - 1, R // 2), 1, min(2, H - min(H - 1, R // 2)), W - 2)))
    if H == 150:
        out.append(('behind_row_64_of_band_1', (137, 1, 7, 3)))
    if H == 130 and R > 64:
        out.append(('behind_row_64_of_band_0', (70, 2, 20, 5)))
    return out


def bank(clips, first_byte=0):
    key = ('bank', first_byte)
    if key not in _CACHE:
        _CACHE[key] = clips.png_bank([f for _, f, _ in files(clips)], first_byte=first_byte, alone=True)
    return _CACHE[key]


def places(clips):
    """(index, boxes, tags): every box of every file, place by place"""
    index, boxes, tags = [], [], []
    for i, (name, _, (H, W, _, R)) in enumerate(files(clips)):
        for tag, box in boxes_of(H, W, R):
            index.append(i), boxes.append(list(box)), tags.append('%s:%s' % (name, tag))
    return index, boxes, tags


def frames(clips):
    """[the frame of png_decode_host] of files(): computed once, shared, never changed"""
    if 'frames' not in _CACHE:
        _CACHE['frames'] = [clips.png_decode_host(f) for _, f, _ in files(clips)]
    return _CACHE['frames']


def reference(clips, key, src, index, boxes, rows, Wc=None):
    """png_bank_window_host, computed once per key and shared"""
    if ('reference', key) not in _CACHE:
        _CACHE[('reference', key)] = clips.png_bank_window_host(src, index, boxes, rows, Wc)
    return _CACHE[('reference', key)]


def filter_5_file(clips):
    """a true flagged file of FAULT's shape but for a filter byte 5 in row 3, and its frame"""
    H, W, ch, R = FAULT
    frame = P.pattern(H, W, ch, 193)
    rows = clips.png_filter_rows_host(frame, 'adaptive', R).copy()
    rows[3, 0] = 5
    return A._flagged(clips, rows, ch, R)[0], torch.from_numpy(frame)


def fault_files(clips):
    """[(name, file, [(box, status)])]: 36 x 25 RGB in bands of 8 rows.  png_alone_cases' lying files, its damaged band and a
    filter byte 5, each with boxes that touch the fault and boxes that do not; None stands for the damaged band's status"""
    if 'faults' in _CACHE:
        return _CACHE['faults']
    lying = {n: (f, s) for n, f, s in A.lying_files(clips)}
    W = FAULT[1]
    out = []
    for ft in (2, 3, 4):                                          # every row k R lies: band 0 alone is sound
        out.append(('fixed_%d_flagged' % ft, lying['fixed_%d_flagged' % ft][0],
                    [((0, 0, 8, W), 0), ((2, 3, 4, 5), 0), ((8, 0, 8, W), 10), ((7, 0, 2, W), 10), ((17, 1, 3, 9), 10)]))
    # Up on every row, band 1 damaged: band 0 sound, band 1 the band's status (before 10), band 2 lies (10), 0 and 1 the band's
    out.append(('damaged_band_and_lying_row', lying['damaged_band_and_lying_row'][0],
                [((0, 0, 8, W), 0), ((9, 0, 3, W), None), ((16, 0, 8, W), 10), ((4, 0, 8, W), None), ((12, 0, 8, W), None)]))
    # Paeth on every row and a 5 in row 3: band 0 is 6, bands 0 and 1 are 6 (before 10), band 1 alone lies
    out.append(('filter_5_and_lying_row', lying['filter_5_and_lying_row'][0],
                [((0, 0, 8, W), 6), ((4, 0, 8, W), 6), ((8, 0, 4, W), 10)]))
    out.append(('row_0_alone_has_type_2', lying['row_0_alone_has_type_2'][0], [((0, 0, 36, W), 0), ((0, 2, 3, 7), 0), ((30, 0, 6, W), 0)]))
    out.append(('damaged_band', A.damaged_file(clips), [((0, 0, 8, W), 0), ((16, 0, 20, W), 0), ((8, 0, 1, W), None), ((0, 0, 36, W), None)]))
    out.append(('filter_5', filter_5_file(clips)[0], [((3, 0, 1, W), 6), ((0, 0, 36, W), 6), ((8, 0, 28, W), 0), ((35, 4, 1, 1), 0)]))
    _CACHE['faults'] = out
    return out


def fault_bank(clips):
    """(the bank of the fault files, a file without the flag behind them; index; boxes; the statuses the cases name)"""
    if 'fault_bank' not in _CACHE:
        named = fault_files(clips)
        plain = clips.png_encode_banded_host(P.pattern(37, 29, 3, 150), 8, 'adaptive', index=True)
        b = clips.png_bank([f for _, f, _ in named] + [plain], alone=True)
        index, boxes, want = [], [], []
        for i, (_, _, cases) in enumerate(named):
            for box, status in cases:
                index.append(i), boxes.append(list(box)), want.append(status)
        index.append(len(named)), boxes.append([0, 0, 8, 8]), want.append(11)
        _CACHE['fault_bank'] = (b, index, boxes, want)
    return _CACHE['fault_bank']


def outside_boxes(H, W):
    """[(clause, box)]: each clause of status 12 that the box alone decides, for an image of H x W"""
    return [('h < 1', (0, 0, 0, 1)), ('w < 1', (0, 0, 1, 0)), ('y0 < 0', (-1, 0, 2, 1)), ('x0 < 0', (0, -1, 1, 2)),
            ('y0 + h > H', (H - 1, 0, 2, 1)), ('x0 + w > W', (0, W - 1, 1, 2))]


def device_calls(clips):
    """[(name, bank, index, boxes, rows, Wc)]: every call the GPU tests hand to a device, the doctored banks among them"""
    if 'calls' in _CACHE:
        return _CACHE['calls']
    b = bank(clips)
    index, boxes, _ = places(clips)
    calls = [('all', b, index, boxes, b.Hmax, b.Wmax),
             ('tight', b, index, boxes, clips.png_window_rows(b, 8), b.Wmax + 3)]
    fb, findex, fboxes, _ = fault_bank(clips)
    extra_i = [0, -1, fb.n, 3] + [1] * 6
    extra_b = [[0, 0, 8, 25], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 8, 25]] + [list(x) for _, x in outside_boxes(36, 25)]
    calls.append(('faults', fb, findex + extra_i, fboxes + extra_b, 36, 29))
    for name, d, place in A.doctored(clips, b):
        H, W = b.sizes[place]
        calls.append(('doctored_' + name, d, [place, (place + 1) % b.n, place], [[0, 0, 1, 1], [0, 0, 1, 1], [H - 1, 0, 1, W]], b.Hmax, b.Wmax))
    _CACHE['calls'] = calls
    return calls


BEYOND = ([2, 0, 1, 1, -1, 3, 0],
          [[0, 1, 1, 68], [7, 0, 2, 31], [0, 0, 5, 9], [4, 1, 1, 7], [0, 0, 1, 1], [0, 0, 1, 1], [19, 0, 1, 31]], 16)   # index, boxes, rows
PROFILE_BOXES = [[0, 0, 4, 4], [0, 0, 5, 9], [0, 0, 1, 70]]


def small_bank(clips, first_byte=0):
    """files 1 to 3: 20 x 31 RGB at R = 8, 5 x 9 grey and 1 x 70 RGBA at R = 16"""
    key = ('small', first_byte)
    if key not in _CACHE:
        _CACHE[key] = clips.png_bank([f for _, f, _ in files(clips)[1:4]], first_byte=first_byte, alone=True)
    return _CACHE[key]


def drawn_case(clips):
    """(bank, the arguments of its clips.BatchPlan): seven smooth frames in bands of 8 rows, boxes of half their sides"""
    import png_encode_cases as C
    if 'drawn' not in _CACHE:
        made = [C.smooth(40 + 3 * j, 48 - 2 * j, 3, 80 + j) for j in range(7)]
        b = clips.png_bank([clips.png_encode_banded_host(f, 8, index=True, alone=True) for f in made], alone=True)
        base = torch.tensor([[h // 4, w // 5, h // 2, w // 2] for h, w in b.sizes], dtype=torch.int32)
        _CACHE['drawn'] = (b, dict(videos=[(0, 4, 0), (4, 3, 1)], T=3, B=2, base=base, K=16, seed=77))
    return _CACHE['drawn']


def other_calls(clips):
    """[(name, bank, index, boxes, rows, Wc)] of the GPU tests beside test_the_bank's: the bank beyond 2^32 bytes, the two
    drawn steps and the profile test's call"""
    index, boxes, rows = BEYOND
    far = small_bank(clips, 2 ** 32 + 16)
    calls = [('beyond', far, index, boxes, rows, far.Wmax)]
    b, args = drawn_case(clips)
    plan = clips.BatchPlan(b, **args)
    for step in (0, 1):
        d = clips.batch_draw_host(plan, step)
        calls.append(('drawn_%d' % step, b, d.index.tolist(), d.boxes.tolist(), clips.png_window_rows(b, plan.max_side), b.Wmax))
    near = small_bank(clips)
    calls.append(('profile', near, [0, 1, 2], PROFILE_BOXES, 8, near.Wmax))
    return calls


def _csv(v):
    v = [str(int(x)) for x in v]
    return ','.join(v) if v else '-'


def call_lines(clips, name, src, index, boxes, rows, Wc, headers, batch=None):
    """The T line of a call and a P line per place.  src: the bank whose tables the device reads; headers: the parsed files
    behind its bytes; batch: the PngBatch of the same files where the call is the batch entry's, whose tables then stand in the
    T line.  The expected values are png_bank_window_host's."""
    win_bands, win_stride = clips.png_window_bands(src, rows), clips.png_window_stride(src, rows)
    if batch is None:
        scalars = (src.first_byte + src.nbytes, src.n, src.nband, src.band_max, src.raw_stride, rows, Wc, win_bands, win_stride, 1)
        images, bands = src.images, src.bands
    else:
        scalars = (batch.nbytes, batch.n, int(batch.bands.shape[0]), int(batch.bands.shape[0]), 0x7ffffff0, rows, Wc, win_bands, win_stride, 0)
        images, bands = batch.images, batch.bands
    lines = ['T %s %s %s %s' % (name, ' '.join(str(v) for v in scalars), _csv(images.reshape(-1).tolist()), _csv(bands.reshape(-1).tolist()))]
    windows, sizes, status, origin, moved = clips.png_bank_window_host(src, index, boxes, rows, Wc)
    inflated = {}
    for j, (i, box) in enumerate(zip(index, boxes)):
        filters, statuses, plan = [], [], (0, -1, 0, 0)
        if 0 <= i < src.n and int(status[j]) not in (9, 11, 12):
            hd = headers[i]
            if i not in inflated:
                inflated[i] = clips.png_inflate_bands_host(hd)
            raw, st = inflated[i]
            plan = clips.png_window_plan(hd.H, hd.bands[0], len(st), box, rows, win_bands, hd.W)
            stride = 1 + hd.W * hd.bpp
            filters = [raw[r * stride] for r in range(plan[2], plan[3])]
            statuses = st[plan[0]:plan[1] + 1]
        lines.append('P %s:%d %d %s %s %s %d %s %s %d %s' % (name, j, i, _csv(box), _csv(filters), _csv(statuses), int(status[j]), _csv(plan),
                                                          _csv(sizes[j].tolist()), int(origin[j]), _csv(moved[j].tolist())))
    return lines, status.tolist()


def write_vectors(path, clips):
    """Every call the GPU tests hand to a device, as the vectors of tools/png_window_check.cpp -> (lines, the set of statuses)"""
    lines, seen = [], set()
    for name, b, index, boxes, rows, Wc in device_calls(clips) + other_calls(clips):
        headers = bank(clips).headers if name.startswith('doctored') else b.headers
        got, status = call_lines(clips, name, b, index, boxes, rows, Wc, headers)
        lines += got
        seen |= set(status)
    b, near = bank(clips), small_bank(clips)
    for tag, src, boxes, rows in (('batch', b, batch_boxes(clips), b.Hmax), ('batch_smallest', b, batch_boxes(clips), batch_rows(clips)),
                                  ('batch_profile', near, PROFILE_BOXES, 8)):
        batch = clips.png_batch(src.headers, bands='index', alone=True)
        got, status = call_lines(clips, tag, src, list(range(src.n)), boxes, rows, src.Wmax, src.headers, batch=batch)
        lines += got
        seen |= set(status)
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return lines, seen


def _aligned(t):
    room = torch.zeros(t.numel() * t.element_size() + 16, dtype=torch.uint8)
    room = room[(-room.data_ptr()) % 16:][:t.numel() * t.element_size()]
    room.copy_(t.contiguous().view(torch.uint8).flatten())
    return room


def entries_refuse(clips, _lib):
    """The -3 list of the three entries, once each, from scalars: a valid block on host memory, one thing made wrong per case.
    Nothing is launched by a call that returns -3, which is why host memory will do -> the number of cases"""
    import ctypes
    import png_bank_cases as K
    lib, seen = _lib.lib(), 0
    # the bank's entry and the drawn one
    bank_ = clips.png_bank(K.small_files(clips), alone=True)
    M, rows, Wc = 3, 8, 14
    wb, ws, need = clips.png_window_bands(bank_, rows), clips.png_window_stride(bank_, rows), clips.png_window_scratch_bytes(bank_, M, rows)
    assert ws % 16 == 0 and need == -(-(M * ws + 4 * M * wb) // 16) * 16 + 20 * M

    def block():
        keep = dict(data=_aligned(bank_.data), scratch=_aligned(torch.zeros(need, dtype=torch.uint8)),
                    out=torch.zeros(M * rows * Wc * 3, dtype=torch.uint8), sizes=torch.zeros((M, 2), dtype=torch.int32),
                    status=torch.zeros(M, dtype=torch.int32), index=torch.tensor([2, 0, 2], dtype=torch.int32),
                    boxes=torch.tensor([[0, 0, 1, 1]] * M, dtype=torch.int32), images=bank_.images.clone(), bands=bank_.bands.clone())
        args = _lib.JpegDecodeArgs(bytes=keep['data'].data_ptr(), nbytes=bank_.nbytes, images=keep['images'].data_ptr(),
                                   images_host=keep['index'].data_ptr(), segments=keep['bands'].data_ptr(), segments_host=None,
                                   qtabs=keep['boxes'].data_ptr(), htabs=None, scratch=keep['scratch'].data_ptr(), scratch_bytes=need,
                                   out=keep['out'].data_ptr(), sizes=keep['sizes'].data_ptr(), status=keep['status'].data_ptr(), stream=None,
                                   n=bank_.n, nseg=bank_.nband, nq=M, nh=0, Hc=rows, Wc=Wc)
        return args, keep

    scalars = dict(m=M, band_max=bank_.band_max, raw_stride=bank_.raw_stride, win_bands=wb, win_stride=ws)
    cases = [('null_' + f, {f: None}, {}) for f in ('bytes', 'images', 'segments', 'images_host', 'scratch', 'out', 'sizes', 'status', 'qtabs')]
    cases += [('m_0', {}, dict(m=0)), ('m_negative', {}, dict(m=-1)), ('band_max_0', {}, dict(band_max=0)),
              ('raw_stride_unaligned', {}, dict(raw_stride=bank_.raw_stride + 8)), ('raw_stride_small', {}, dict(raw_stride=0)),
              ('nq_other', dict(nq=M + 1), {}), ('nq_0', dict(nq=0), {}), ('win_bands_0', {}, dict(win_bands=0)),
              ('win_bands_beyond_band_max', {}, dict(win_bands=bank_.band_max + 1)), ('win_stride_small', {}, dict(win_stride=0)),
              ('win_stride_unaligned', {}, dict(win_stride=ws + 8)), ('m_win_bands_beyond_int', {}, dict(m=2 ** 20, band_max=2 ** 11, win_bands=2 ** 11)),
              ('scratch_one_byte_short', dict(scratch_bytes=need - 1), {}), ('rows_0', dict(Hc=0), {}), ('rows_tall', dict(Hc=16385), {}),
              ('canvas_wide', dict(Wc=16385), {}), ('n_0', dict(n=0), {}), ('nseg_0', dict(nseg=0), {}), ('nbytes_negative', dict(nbytes=-1), {})]
    for name, fields, extra in cases:
        args, keep = block()
        for f, v in fields.items():
            setattr(args, f, v)
        s = dict(scalars, **extra)
        assert lib.istvt_png_decode_bank_window_u8(ctypes.byref(args), s['m'], s['band_max'], s['raw_stride'], s['win_bands'], s['win_stride']) == -3, name
        seen += 1
    assert lib.istvt_png_decode_bank_window_u8(None, M, bank_.band_max, bank_.raw_stride, wb, ws) == -3
    args, keep = block()
    args.out = args.bytes
    assert lib.istvt_png_decode_bank_window_u8(ctypes.byref(args), M, bank_.band_max, bank_.raw_stride, wb, ws) == -3
    args, keep = block()
    for Bc, T, ints in ((0, 3, 64), (1, 0, 64), (1, 3, 36 + 2)):
        assert lib.istvt_png_decode_bank_window_drawn_u8(ctypes.byref(args), Bc, T, ints, bank_.band_max, bank_.raw_stride, wb, ws) == -3
    assert lib.istvt_png_decode_bank_window_drawn_u8(None, 1, 3, 64, bank_.band_max, bank_.raw_stride, wb, ws) == -3
    # the batch's entry
    named = files(clips)[1:4]
    batch = clips.png_batch([f for _, f, _ in named], bands='index', alone=True)
    n, nband, rows, Wc = batch.n, int(batch.bands.shape[0]), 16, 70
    wb, ws, need = clips.png_window_bands(batch, rows), clips.png_window_stride(batch, rows), clips.png_window_scratch_bytes(batch, n, rows)
    entry = lib.istvt_png_decode_window_u8

    def block(flags=None, bands=None):
        keep = dict(data=_aligned(batch.data), scratch=_aligned(torch.zeros(need, dtype=torch.uint8)),
                    out=torch.zeros(n * rows * Wc * 3, dtype=torch.uint8), sizes=torch.zeros((n, 2), dtype=torch.int32),
                    status=torch.zeros(n, dtype=torch.int32), images=batch.images.clone(), boxes=torch.tensor([[0, 0, 1, 1]] * n, dtype=torch.int32),
                    bands=batch.bands.clone() if bands is None else bands, flags=batch.alone.clone() if flags is None else flags)
        args = _lib.JpegDecodeArgs(bytes=keep['data'].data_ptr(), nbytes=batch.nbytes, images=keep['images'].data_ptr(),
                                   images_host=keep['images'].data_ptr(), segments=keep['bands'].data_ptr(),
                                   segments_host=keep['bands'].data_ptr(), qtabs=keep['boxes'].data_ptr(), htabs=keep['flags'].data_ptr(),
                                   scratch=keep['scratch'].data_ptr(), scratch_bytes=need, out=keep['out'].data_ptr(),
                                   sizes=keep['sizes'].data_ptr(), status=keep['status'].data_ptr(), stream=None, n=n, nseg=nband,
                                   nq=n, nh=n, Hc=rows, Wc=Wc)
        return args, keep

    cases = [('null_' + f, {f: None}) for f in ('bytes', 'images', 'images_host', 'segments', 'segments_host', 'qtabs', 'htabs', 'scratch',
                                                'out', 'sizes', 'status')]
    cases += [('nq_0', dict(nq=0)), ('nq_other', dict(nq=n + 1)), ('nh_other', dict(nh=n - 1)), ('n_0', dict(n=0)),
              ('nseg_short', dict(nseg=nband - 1)), ('scratch_one_byte_short', dict(scratch_bytes=need - 1)),
              ('rows_0', dict(Hc=0)), ('rows_tall', dict(Hc=16385)), ('canvas_narrow', dict(Wc=69)), ('canvas_wide', dict(Wc=16385)),
              ('nbytes_negative', dict(nbytes=-1))]
    for name, fields in cases:
        args, keep = block()
        for f, v in fields.items():
            setattr(args, f, v)
        assert entry(ctypes.byref(args), wb, ws) == -3, name
        seen += 1
    assert entry(None, wb, ws) == -3
    args, keep = block()
    assert entry(ctypes.byref(args), 0, ws) == -3 and entry(ctypes.byref(args), wb, ws + 8) == -3 and entry(ctypes.byref(args), wb, 0) == -3
    args.out = args.bytes
    assert entry(ctypes.byref(args), wb, ws) == -3
    for bad in (0, 2, 3, -1):                                      # every flag is 1
        flags = batch.alone.clone()
        flags[1] = bad
        args, keep = block(flags=flags)
        assert entry(ctypes.byref(args), wb, ws) == -3, bad
    first, stride = int(batch.images[0, 6]), 1 + 31 * 3             # a band edge of the 20 x 31 file moved by a row
    moved = batch.bands.clone()
    moved[first, 4] += stride
    moved[first + 1, 3] += stride
    moved[first + 1, 4] -= stride
    args, keep = block(bands=moved)
    assert entry(ctypes.byref(args), wb, ws) == -3
    return seen


def batch_rows(clips):
    """the smallest window that fits every box of the batch call"""
    need = 1
    for (_, _, (H, W, _, R)), box in zip(files(clips), batch_boxes(clips)):
        plan = clips.png_window_plan(H, R, -(-H // R), box, H, -(-H // R), W)
        need = max(need, plan[3] - plan[2])
    return need


def batch_boxes(clips):
    """the boxes of the batch call: box i mod its count of file i"""
    return [list(boxes_of(H, W, R)[i % len(boxes_of(H, W, R))][1]) for i, (_, _, (H, W, _, R)) in enumerate(files(clips))]
