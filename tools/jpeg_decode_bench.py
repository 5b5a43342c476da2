#!/usr/bin/env python3
"""JPEG files (DESIGN.md "JPEG files") on one GPU in one process: ops.jpeg_decode_u8 on one training step's frames.

    python tools/jpeg_decode_bench.py [--frames 256] [--size 224] [--cache DIR] [--out profiles/NAME.txt]
    python tools/jpeg_decode_bench.py --encode-only --cache DIR      # no GPU: write the files of the benchmark

--frames frames of --size x --size: 8 distinct smooth_image frames (tests/golden/make_jpeg_golden.py's recipe) encoded with
clips.jpeg_encode_host and repeated; quality 75 and 90, 4:2:0, restart interval 0 and one MCU row.  --cache keeps the encoded
files between runs (the host encoder is plain Python).  Per configuration, after checking the 8 distinct frames against
clips.jpeg_roundtrip_host:

decode   ops.jpeg_decode_u8 on the uploaded batch with the caller's buffers, events around the call (three launches);
         alternating with ops.jpeg_roundtrip_u8 on the same decoded frames as context; medians and min-max over the repeats
         after the warm-up.  The three kernels apart come from `rocprofv3 --kernel-trace --stats` on a run with --reps 3.
--split  adds, on the two restart-less configurations and on the row-restart one at quality 75, ops.jpeg_decode_u8(...,
         split=chunk) for chunk 64, 128, 256 and 512 (DESIGN.md "JPEG files without restart markers"): checked against the
         default call's frames, then timed in alternation with the default call, whose code no chunk size changes.  It
         also adds quality 75 with a restart marker every 2, 4 and 8 MCU rows, at the default chunk size: where between a
         row and a whole file the split starts to pay, which is what split='auto' decides by.
upload   the compressed batch (scan bytes and tables) against the decoded clip (3 bytes per pixel), both from pinned memory,
         host clock around copy + synchronise.
--layouts  instead of the above (DESIGN.md "JPEG layouts"): layouts '420' (clips.jpeg_encode_host), '422' and 'grey'
         (clips.jpeg_encode_layout_host) at quality 75 and 90, restart-less with split=128 and with a marker per MCU row by
         the default call; the 8 distinct frames are compared with clips.jpeg_decode_host, then the configurations are timed in
         alternation.  With --against OTHER.so (another build of the library, the parent commit's for instance) the four
         4:2:0 configurations by the default call, and split=128 on the restart-less ones, are timed through the entry
         points of both libraries in alternation instead.
--bank   instead of the above (DESIGN.md "JPEG bank"): at quality 75 and 90 with a marker per MCU row, a clips.JpegBank of
         --bank-files files (4096; the 8 distinct files repeated), of which every call draws --frames (256).  The same draw is
         decoded (a) from bytes by ops.jpeg_decode_u8(files): parse, pack, upload, decode; (b) from a prepacked JpegBatch with
         checked=True and the caller's buffers, the fastest path without a bank; (c) by ops.jpeg_decode_indexed_u8 through a
         device index with the caller's buffers; (d) as (c) with a fresh torch.randint index on the device per call.  (c)'s
         frames are compared with (b)'s first.  Per path the device time by events and the host's wall time per call with the
         stream drained; (b) and (c) alternate.  Then the ingest: clips.JpegBank.from_encoded on --frames files of
         ops.jpeg_encode_u8 against files() + clips.jpeg_batch + upload.  The plan kernel's own time comes from `rocprofv3
         --kernel-trace --stats` on a run with --reps 3.
--bank --split  (DESIGN.md "JPEG bank, split") the bank of files WITHOUT restart markers, at quality 75 and 90, the same
         --bank-files and --frames, through a device index with the caller's buffers: (a) the bank with split=128
         (clips.JPEG_SPLIT_DEFAULT), (b) the same bank through with_split(None), one lane per file, which is the code of a
         bank before it had a split, (c) ops.jpeg_decode_u8 on a prepacked JpegBatch of the drawn files with split=128,
         checked=True and the caller's buffers.  The three give the same frames, which is checked first; then they are timed
         by events in alternation, each first in turn.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import clips, ops  # noqa: E402

DISTINCT = 8
QUALITIES = (75, 90)
SPLIT_CHUNKS = (64, 128, 256, 512)


def smooth_image(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def say(lines, text):
    print(text, flush=True)
    lines.append(text)


def encoded(a, q, ri):
    """the 8 distinct files of a configuration, from the cache or from the host encoder"""
    path = os.path.join(a.cache, 'jpeg_decode_bench_%d_q%d_ri%d.npz' % (a.size, q, ri)) if a.cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return [bytes(z['f%d' % i]) for i in range(DISTINCT)]
    files = [clips.jpeg_encode_host(torch.from_numpy(smooth_image(a.size, a.size, 1000 + i)), q, '420', ri) for i in range(DISTINCT)]
    if path:
        os.makedirs(a.cache, exist_ok=True)
        np.savez(path, **{'f%d' % i: np.frombuffer(f, dtype=np.uint8) for i, f in enumerate(files)})
    return files


def split_rows(a, lines, res, batch, out, want, buffers, q, ri, chunks):
    """--split: ops.jpeg_decode_u8(..., split=chunk) for every chunk size of SPLIT_CHUNKS on one configuration, each checked
    against the default call's frames and timed in alternation with the default call; the rounds come from the state rows"""
    n = batch.n
    for chunk in chunks:
        plan = clips.jpeg_split_plan(batch, chunk)
        mine = (torch.empty((plan.scratch_bytes,), dtype=torch.uint8, device=out.device), buffers[1], buffers[2])
        got, _, status = ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=mine, split=chunk)
        clips.check_jpeg_status(status)
        if not torch.equal(got, want):
            raise SystemExit('q=%d ri=%d split=%d: the frames are not the default call\'s' % (q, ri, chunk))
        table = mine[0][plan.states_at:plan.states_at + 32 * plan.rows].view(torch.int32).view(-1, 8)
        rounds = [int(table[r0:r0 + c, 7].max()) for r0, c in zip(plan.row0[:len(plan.row0) // n * DISTINCT],
                                                                  plan.count[:len(plan.count) // n * DISTINCT])]
        ts, td = [], []
        for r in range(a.warmup + a.reps):
            x = event_ms(lambda: ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=mine, split=chunk))
            y = event_ms(lambda: ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=buffers))
            if r >= a.warmup:
                ts.append(x)
                td.append(y)
        ss, sd = stats(ts), stats(td)
        res['split%d' % chunk] = {'decode': ss, 'default_beside': sd, 'chunks': max(plan.count), 'chunk': max(plan.chunk),
                                  'rounds_max': max(rounds), 'rounds_median': statistics.median(rounds),
                                  'scratch_bytes': plan.scratch_bytes}
        say(lines, 'jpeg_decode_u8 q=%d, restart interval %d, split=%d: up to %d chunks of %d bytes, rounds median %g, max %d | '
            '%.3f ms (%.3f-%.3f) against %.3f ms (%.3f-%.3f) by default beside it = %.2f x'
            % (q, ri, chunk, max(plan.count), max(plan.chunk), statistics.median(rounds), max(rounds), ss['median_ms'],
               ss['min_ms'], ss['max_ms'], sd['median_ms'], sd['min_ms'], sd['max_ms'], sd['median_ms'] / ss['median_ms']))


def layout_files(a, layout, q, ri):
    """the 8 distinct files of a layout and their frames by clips.jpeg_decode_host, from the cache or made here"""
    path = os.path.join(a.cache, 'jpeg_layouts_bench_%d_%s_q%d_ri%d.npz' % (a.size, layout, q, ri)) if a.cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return [bytes(z['f%d' % i]) for i in range(DISTINCT)], torch.from_numpy(z['frames'])
    srcs = [torch.from_numpy(smooth_image(a.size, a.size, 1000 + i)) for i in range(DISTINCT)]
    files = [clips.jpeg_encode_host(x, q, '420', ri) if layout == '420' else clips.jpeg_encode_layout_host(x, q, layout, ri)
             for x in srcs]
    frames = torch.stack([clips.jpeg_decode_host(f, layouts='all') for f in files])
    if path:
        os.makedirs(a.cache, exist_ok=True)
        np.savez(path, frames=frames.numpy(), **{'f%d' % i: np.frombuffer(f, dtype=np.uint8) for i, f in enumerate(files)})
    return files, frames


def entry_call(lib, batch, out, buffers, chunk):
    """one call of a library's entry point on an uploaded batch, as frames.jpeg_decode_u8 makes it"""
    from istvt_amd import _lib
    dev = batch.on(out.device)
    args = _lib.JpegDecodeArgs(
        bytes=dev.data.data_ptr(), nbytes=batch.nbytes, images=dev.images.data_ptr(), images_host=batch.images.data_ptr(),
        segments=dev.segments.data_ptr(), segments_host=batch.segments.data_ptr(), qtabs=dev.qtabs.data_ptr(),
        htabs=dev.htabs.data_ptr(), scratch=buffers[0].data_ptr(), scratch_bytes=buffers[0].numel(), out=out.data_ptr(),
        sizes=buffers[1].data_ptr(), status=buffers[2].data_ptr(), stream=None, n=batch.n, nseg=int(batch.segments.shape[0]),
        nq=int(batch.qtabs.shape[0]), nh=int(batch.htabs.shape[0]), Hc=out.shape[1], Wc=out.shape[2])
    if chunk is None:
        rc = lib.istvt_jpeg_decode_u8(ctypes.byref(args))
    else:
        rc = lib.istvt_jpeg_decode_split_u8(ctypes.byref(args), chunk)
    if rc != 0:
        raise SystemExit('the entry point returned %d' % rc)


def layouts_main(a):
    """--layouts: the layout table, or with --against the alternation of two libraries on the 4:2:0 configurations"""
    from istvt_amd import _lib
    n, S = a.frames, a.size
    chunk = clips.JPEG_SPLIT_DEFAULT
    layouts = ('420',) if a.against else ('420', '422', 'grey')
    step = {'420': 16, '422': 16, 'grey': 8}
    configs = [(lay, q, ri, split) for lay in layouts for q in QUALITIES
               for ri, split in ((0, chunk), (-(-S // step[lay]), None))]
    if a.against:
        configs += [(lay, q, 0, None) for lay in layouts for q in QUALITIES]
    if a.encode_only:
        for lay, q, ri, _ in configs:
            nbytes = sum(len(f) for f in layout_files(a, lay, q, ri)[0])
            print('%s q=%d restart interval %d: %d bytes in %d files' % (lay, q, ri, nbytes, DISTINCT))
        return
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_decode_bench.py measures on a GPU; none is visible')
    dev = torch.device('cuda', torch.cuda.current_device())
    torch.zeros(1, device=dev)
    libs = [('this', _lib.lib())]
    if a.against:
        other = ctypes.CDLL(os.path.abspath(a.against))
        for name in ('istvt_jpeg_decode_u8', 'istvt_jpeg_decode_split_u8'):
            getattr(other, name).argtypes, getattr(other, name).restype = _lib.SIGNATURES[name], ctypes.c_int
        libs.append(('other', other))
    lines, res, runs = [], {}, []
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    for lay, q, ri, split in configs:
        files, frames = layout_files(a, lay, q, ri)
        batch = clips.jpeg_batch([files[i % DISTINCT] for i in range(n)], layouts='all')
        need = batch.scratch_bytes if split is None else clips.jpeg_split_plan(batch, split).scratch_bytes
        buffers = (torch.empty((need,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                   torch.empty((n,), dtype=torch.int32, device=dev))
        for name, lib in libs:                                    # the frames before anything is timed
            out.zero_()
            entry_call(lib, batch, out, buffers, split)
            clips.check_jpeg_status(buffers[2])
            if not torch.equal(out[:DISTINCT].cpu(), frames) or not torch.equal(out[n - DISTINCT:], out[:DISTINCT]):
                raise SystemExit('%s q=%d ri=%d (%s): the decoded frames are not the definition' % (lay, q, ri, name))
        runs.append((lay, q, ri, split, batch, buffers))
    times = {(i, name): [] for i in range(len(runs)) for name, _ in libs}
    for r in range(a.warmup + a.reps):                            # alternating between configurations and libraries
        for i, (lay, q, ri, split, batch, buffers) in enumerate(runs):
            for name, lib in (libs if r % 2 == 0 else libs[::-1]):
                t = event_ms(lambda: entry_call(lib, batch, out, buffers, split))
                if r >= a.warmup:
                    times[(i, name)].append(t)
    for i, (lay, q, ri, split, batch, buffers) in enumerate(runs):
        up = sum(t.numel() * t.element_size() for t in (batch.data, batch.images, batch.segments, batch.qtabs, batch.htabs))
        key = '%s_q%d_ri%d_%s' % (lay, q, ri, 'default' if split is None else 'split%d' % split)
        res[key] = {'segments': int(batch.segments.shape[0]), 'scan_bytes': batch.nbytes, 'blocks': batch.blocks,
                    'uploaded_bytes': up, 'decoded_bytes': out.numel()}
        text = ('%s q=%d, restart interval %d, %s: %d frames of %d x %d, scans %.2f MB, %d blocks, uploaded %.2f MB against '
                '%.2f MB decoded') \
            % (lay, q, ri, 'default call' if split is None else 'split=%d' % split, n, S, S, batch.nbytes * 1e-6, batch.blocks,
               up * 1e-6, out.numel() * 1e-6)
        for name, _ in libs:
            st = stats(times[(i, name)])
            res[key][name] = st
            text += ' | %s %.3f ms (%.3f-%.3f)' % (name, st['median_ms'], st['min_ms'], st['max_ms'])
        if a.against:
            t, o = res[key]['this'], res[key]['other']
            text += ' | this / other = %.4f, other\'s spread %+.1f %% .. %+.1f %%' % (
                t['median_ms'] / o['median_ms'], 100 * (o['min_ms'] / o['median_ms'] - 1), 100 * (o['max_ms'] / o['median_ms'] - 1))
        say(lines, text)
    line = json.dumps({'jpeg_layouts_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def bank_main(a):
    """--bank: the indexed decode from a resident bank against the two ways of decoding the same files without one"""
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_decode_bench.py measures on a GPU; none is visible')
    n, S, N = a.frames, a.size, a.bank_files
    dev = torch.device('cuda', torch.cuda.current_device())
    torch.zeros(1, device=dev)
    lines, res = [], {}
    row = -(-S // 16)
    out, out_b = (torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    raw_dev = src.repeat((-(-n // DISTINCT), 1, 1, 1))[:n].contiguous().to(dev)

    def both(fn, reps, warmup=a.warmup):
        """(device ms by events, host ms with the stream drained) per call, after the warm-up"""
        td, th = [], []
        for r in range(warmup + reps):
            x, y = event_ms(fn), timed(fn)
            if r >= warmup:
                td.append(x)
                th.append(y)
        return stats(td), stats(th)

    def small(n_):
        return (torch.empty((n_, 2), dtype=torch.int32, device=dev), torch.empty((n_,), dtype=torch.int32, device=dev))
    for q in QUALITIES:
        files = encoded(a, q, row)
        headers = [clips.jpeg_parse(f) for f in files]            # parsed once: the bank's 4096 files are these 8, repeated
        bank = clips.jpeg_bank([headers[i % DISTINCT] for i in range(N)])
        bank.on(dev)
        g = torch.Generator().manual_seed(q)
        draw = torch.randint(0, N, (n,), generator=g)
        index = draw.to(torch.int32).to(dev)
        drawn = [files[i % DISTINCT] for i in draw.tolist()]
        batch = clips.jpeg_batch(drawn)
        buf_b = (torch.empty((batch.scratch_bytes,), dtype=torch.uint8, device=dev),) + small(n)
        buf_c = (torch.empty((clips.jpeg_bank_scratch_bytes(bank, n),), dtype=torch.uint8, device=dev),) + small(n)
        want, _, st_b = ops.jpeg_decode_u8(batch, out=out_b, checked=True, buffers=buf_b)
        got, _, st_c = ops.jpeg_decode_indexed_u8(bank, index, out=out, buffers=buf_c)
        clips.check_jpeg_status(st_b)
        clips.check_jpeg_bank_status(st_c)
        if not torch.equal(got, want):
            raise SystemExit('q=%d: the indexed decode is not the default call on the same files' % q)
        sa = both(lambda: ops.jpeg_decode_u8(drawn, out=out_b), max(2, a.reps // 5), 1)     # a second per call: the host parse
        tb, tc, hb, hc = [], [], [], []

        def by_batch():
            return ops.jpeg_decode_u8(batch, out=out_b, checked=True, buffers=buf_b)

        def by_bank():
            return ops.jpeg_decode_indexed_u8(bank, index, out=out, buffers=buf_c)
        for r in range(a.warmup + a.reps):                        # (b) and (c) in alternation, either first in turn
            order = ((by_batch, tb, hb), (by_bank, tc, hc))[::1 if r % 2 == 0 else -1]
            for clock, which in ((event_ms, 1), (timed, 2)):
                for entry in order:
                    t = clock(entry[0])
                    if r >= a.warmup:
                        entry[which].append(t)
        sd = both(lambda: ops.jpeg_decode_indexed_u8(bank, torch.randint(0, N, (n,), device=dev), out=out, buffers=buf_c), a.reps)
        # the ingest, on the same frames at this quality
        jf = ops.jpeg_encode_u8(raw_dev, q, '420', 'row')
        si = both(lambda: clips.JpegBank.from_encoded(jf), a.reps)
        sh = both(lambda: clips.jpeg_batch(jf.files()).on(dev), max(2, a.reps // 5), 1)
        ingested = clips.JpegBank.from_encoded(jf)
        again, _, st_i = ops.jpeg_decode_indexed_u8(ingested, torch.arange(n, device=dev))
        clips.check_jpeg_bank_status(st_i)
        if not torch.equal(again, ops.jpeg_decode_u8(jf.files())[0]):
            raise SystemExit('q=%d: the ingested bank does not decode to the files\' frames' % q)
        res['q%d' % q] = {'bank_files': N, 'frames': n, 'size': S, 'bank_scan_bytes': bank.nbytes, 'drawn_scan_bytes': batch.nbytes,
                          'seg_max': bank.seg_max, 'block_stride': bank.block_stride,
                          'scratch_bytes': {'batch': batch.scratch_bytes, 'bank': clips.jpeg_bank_scratch_bytes(bank, n)},
                          'a_files': {'device': sa[0], 'host': sa[1]}, 'b_batch': {'device': stats(tb), 'host': stats(hb)},
                          'c_bank': {'device': stats(tc), 'host': stats(hc)}, 'd_bank_randint': {'device': sd[0], 'host': sd[1]},
                          'ingest_device': {'device': si[0], 'host': si[1]}, 'ingest_host': {'device': sh[0], 'host': sh[1]}}
        fmt = '%.3f ms (%.3f-%.3f)'
        say(lines, 'bank q=%d: %d of %d files of %d x %d per call, bank scans %.2f MB, drawn %.2f MB, seg_max %d, block_stride %d'
            % (q, n, N, S, S, bank.nbytes * 1e-6, batch.nbytes * 1e-6, bank.seg_max, bank.block_stride))
        for name, key in (('(a) files: parse, pack, upload, decode', 'a_files'), ('(b) prepacked JpegBatch, checked', 'b_batch'),
                          ('(c) bank, device index', 'c_bank'), ('(d) bank, torch.randint per call', 'd_bank_randint'),
                          ('ingest: JpegBank.from_encoded', 'ingest_device'),
                          ('ingest: files() + jpeg_batch + upload', 'ingest_host')):
            d, h = res['q%d' % q][key]['device'], res['q%d' % q][key]['host']
            say(lines, ('  %-42s device ' + fmt + ' | host, drained ' + fmt)
                % (name, d['median_ms'], d['min_ms'], d['max_ms'], h['median_ms'], h['min_ms'], h['max_ms']))
    line = json.dumps({'jpeg_bank_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def bank_split_main(a):
    """--bank --split: a bank of restart-less files with and without its split, beside the split call on a prepacked batch"""
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_decode_bench.py measures on a GPU; none is visible')
    n, S, N = a.frames, a.size, a.bank_files
    chunk = clips.JPEG_SPLIT_DEFAULT
    dev = torch.device('cuda', torch.cuda.current_device())
    torch.zeros(1, device=dev)
    lines, res = [], {}
    outs = [torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(3)]

    def small():
        return (torch.empty((n, 2), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
    for q in QUALITIES:
        files = encoded(a, q, 0)
        headers = [clips.jpeg_parse(f) for f in files]
        bank = clips.jpeg_bank([headers[i % DISTINCT] for i in range(N)], split=chunk)
        plain = bank.with_split(None)
        bank.on(dev)
        g = torch.Generator().manual_seed(q)
        draw = torch.randint(0, N, (n,), generator=g)
        index = draw.to(torch.int32).to(dev)
        batch = clips.jpeg_batch([headers[i % DISTINCT] for i in draw.tolist()])
        need = {'a_bank_split': clips.jpeg_bank_scratch_bytes(bank, n), 'b_bank_one_lane': clips.jpeg_bank_scratch_bytes(plain, n),
                'c_batch_split': clips.jpeg_split_plan(batch, chunk).scratch_bytes}
        bufs = {k: (torch.empty((v,), dtype=torch.uint8, device=dev),) + small() for k, v in need.items()}
        calls = {'a_bank_split': lambda: ops.jpeg_decode_indexed_u8(bank, index, out=outs[0], buffers=bufs['a_bank_split']),
                 'b_bank_one_lane': lambda: ops.jpeg_decode_indexed_u8(plain, index, out=outs[1], buffers=bufs['b_bank_one_lane']),
                 'c_batch_split': lambda: ops.jpeg_decode_u8(batch, out=outs[2], checked=True, buffers=bufs['c_batch_split'],
                                                             split=chunk)}
        first = {k: fn() for k, fn in calls.items()}
        clips.check_jpeg_bank_status(first['a_bank_split'][2])
        clips.check_jpeg_bank_status(first['b_bank_one_lane'][2])
        clips.check_jpeg_status(first['c_batch_split'][2])
        if not (torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])):
            raise SystemExit('q=%d: the three decodes of the same draw differ' % q)
        names = list(calls)
        times = {k: [] for k in names}
        for r in range(a.warmup + a.reps):                        # in alternation, each first in turn
            for k in names[r % 3:] + names[:r % 3]:
                t = event_ms(calls[k])
                if r >= a.warmup:
                    times[k].append(t)
        st = {k: stats(v) for k, v in times.items()}
        res['q%d' % q] = dict(st, bank_files=N, frames=n, size=S, chunk_bytes=chunk, chunk_rows=bank.chunk_rows,
                              seg_bytes_max=bank.seg_bytes_max, bank_scan_bytes=bank.nbytes, drawn_scan_bytes=batch.nbytes,
                              scratch_bytes=need)
        say(lines, 'bank, split q=%d: %d of %d restart-less files of %d x %d per call, bank scans %.2f MB, drawn %.2f MB, longest scan '
            '%d bytes, chunk %d, %d state rows per segment' % (q, n, N, S, S, bank.nbytes * 1e-6, batch.nbytes * 1e-6,
                                                               bank.seg_bytes_max, chunk, bank.chunk_rows))
        for name, key in (('(a) bank with split=%d, device index' % chunk, 'a_bank_split'),
                          ('(b) the same bank, with_split(None)', 'b_bank_one_lane'),
                          ('(c) prepacked JpegBatch, split=%d, checked' % chunk, 'c_batch_split')):
            say(lines, '  %-44s %.3f ms (%.3f-%.3f), scratch %.2f MB' % (name, st[key]['median_ms'], st[key]['min_ms'],
                                                                         st[key]['max_ms'], need[key] * 1e-6))
        c = st['c_batch_split']
        say(lines, '  (a) - (c) = %+.3f ms; (c)\'s own spread is %.3f ms; (b) / (a) = %.2f x'
            % (st['a_bank_split']['median_ms'] - c['median_ms'], c['max_ms'] - c['min_ms'],
               st['b_bank_one_lane']['median_ms'] / st['a_bank_split']['median_ms']))
    line = json.dumps({'jpeg_bank_split_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bank', action='store_true')
    ap.add_argument('--bank-files', type=int, default=4096)
    ap.add_argument('--layouts', action='store_true')
    ap.add_argument('--against', default=None)
    ap.add_argument('--split', action='store_true')
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cache', default=None)
    ap.add_argument('--encode-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.layouts:
        return layouts_main(a)
    if a.bank:
        return bank_split_main(a) if a.split else bank_main(a)
    row = -(-a.size // 16)                                        # MCUs of one MCU row at 4:2:0
    configs = [(q, ri) for q in QUALITIES for ri in (0, row)]
    longer = [(QUALITIES[0], k * row) for k in (2, 4, 8)] if a.split else []     # where between a row and a file it starts to pay
    configs += longer
    if a.encode_only:
        for q, ri in configs:
            print('q=%d restart interval %d: %d bytes in %d files' % (q, ri, sum(len(f) for f in encoded(a, q, ri)), DISTINCT))
        return
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_decode_bench.py measures on a GPU; none is visible')
    n, S = a.frames, a.size
    lines, res = [], {}
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    raw = src.repeat((-(-n // DISTINCT), 1, 1, 1))[:n].contiguous().pin_memory()
    raw_dev = raw.cuda()
    out, rt_out = torch.empty_like(raw_dev), torch.empty_like(raw_dev)
    for q, ri in configs:
        files = encoded(a, q, ri)
        batch = clips.jpeg_batch([files[i % DISTINCT] for i in range(n)])
        dev = torch.device('cuda', torch.cuda.current_device())
        buffers = (torch.empty((batch.scratch_bytes,), dtype=torch.uint8, device=dev),
                   torch.empty((n, 2), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        got, _, status = ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=buffers)
        clips.check_jpeg_status(status)
        want = clips.jpeg_roundtrip_host(src, q, '420')
        if not torch.equal(got[:DISTINCT].cpu(), want) or not torch.equal(got[n - DISTINCT:], got[:DISTINCT]):
            raise SystemExit('q=%d ri=%d: the decoded frames are not the definition' % (q, ri))
        qdev = torch.full((n,), q, dtype=torch.int32, device=dev)
        td, tr = [], []
        for r in range(a.warmup + a.reps):
            x = event_ms(lambda: ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=buffers))
            y = event_ms(lambda: ops.jpeg_roundtrip_u8(raw_dev, qdev, '420', out=rt_out, checked=True))
            if r >= a.warmup:
                td.append(x)
                tr.append(y)
        host = [batch.data, batch.images, batch.segments, batch.qtabs, batch.htabs]
        up = sum(t.numel() * t.element_size() for t in host)
        tu, tw = [], []
        for r in range(a.warmup + a.reps):
            x = timed(lambda: [t.to(dev, non_blocking=True) for t in host])
            y = timed(lambda: raw.to(dev, non_blocking=True))
            if r >= a.warmup:
                tu.append(x)
                tw.append(y)
        sd, sr, su, sw = stats(td), stats(tr), stats(tu), stats(tw)
        key = 'q%d_ri%d' % (q, ri)
        res[key] = {'frames': n, 'size': S, 'segments': int(batch.segments.shape[0]), 'scan_bytes': batch.nbytes,
                    'uploaded_bytes': up, 'decoded_bytes': raw.numel(), 'decode': sd, 'roundtrip': sr, 'upload_compressed': su,
                    'upload_decoded': sw, 'scratch_bytes': batch.scratch_bytes}
        say(lines, 'jpeg_decode_u8 q=%d, restart interval %d: %d frames of %d x %d in %d segments | %.3f ms (%.3f-%.3f) = %.2f us per '
            'frame, %.2f ns per pixel | jpeg_roundtrip_u8 on the same frames %.3f ms (%.3f-%.3f) | uploaded %.2f MB (scans %.2f MB) '
            'against %.2f MB decoded = 1 / %.1f: %.3f ms (%.3f-%.3f) against %.3f ms (%.3f-%.3f)'
            % (q, ri, n, S, S, res[key]['segments'], sd['median_ms'], sd['min_ms'], sd['max_ms'], sd['median_ms'] * 1e3 / n,
               sd['median_ms'] * 1e6 / (n * S * S), sr['median_ms'], sr['min_ms'], sr['max_ms'], up * 1e-6, batch.nbytes * 1e-6,
               raw.numel() * 1e-6, raw.numel() / up, su['median_ms'], su['min_ms'], su['max_ms'], sw['median_ms'], sw['min_ms'],
               sw['max_ms']))
        if a.split and (ri == 0 or q == QUALITIES[0]):
            chunks = (clips.JPEG_SPLIT_DEFAULT,) if (q, ri) in longer else SPLIT_CHUNKS
            split_rows(a, lines, res[key], batch, out, got.clone(), buffers, q, ri, chunks)
    line = json.dumps({'jpeg_decode_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
