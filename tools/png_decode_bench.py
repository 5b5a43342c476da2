#!/usr/bin/env python
"""PNG files (DESIGN.md "PNG files") on one GPU in one process: ops.png_decode_u8 on one training step's frames.

    python tools/png_decode_bench.py [--frames 256] [--size 224] [--out profiles/png_decode_bench.txt]

The frames are tools/jpeg_decode_bench.py's (8 distinct ones, repeated), written by PIL as PNG at compress level 6 and again
at level 1.  In one run, the legs in alternation (medians, with the fastest and the slowest repetition):

device   ops.png_decode_u8 from a prepacked, uploaded PngBatch with the caller's buffers, events around the call (two
         launches); each kernel's share from a torch.profiler trace of ten more calls; the frames are compared with the source
         pixels first (PNG is lossless)
host     what a user does without it: PIL decodes the same files on the host, the decoded bytes go up (3 bytes per pixel)
jpeg     for context, ops.jpeg_decode_u8 on the same frames at quality 90, as tools/jpeg_decode_bench.py measures it
upload   the bytes each route sends to the device
large    one batch of 8 frames of 1080 x 1920 at level 6, the same legs without the JPEG one

--bands [--against PARENT.so] [--bench-py K [--parent-tree DIR]]  instead of the above (DESIGN.md "PNG files by their bands"): the same frames, 256
of 224 x 224 and 8 of 1080 x 1920, as our own files with their band index (ops.png_encode_u8(index=True), whose bytes the tests
pin to the definition) at band_rows 8, 16 and 32.  Per size and band_rows, after the decoded frames are compared with the
source pixels, in alternation:

bands    ops.png_decode_u8 on the batch packed with bands='index': one wave per band; each kernel's share from a
         torch.profiler trace of ten more calls
seq      the same files packed without bands: one wave per file, this tree
parent   with --against, the sequential entry of that library (the parent commit's build, made as tools/build_variant.sh makes
         a variant: the same flags) on the same arguments: the speed-up is stated against this leg
host     PIL decodes the same files on the host, the decoded bytes go up
encode   ops.png_encode_u8 with and without the index on the same frames
--bench-py K   bench.py at its defaults K times on this tree and, with --parent-tree DIR, on that checkout of the parent commit
         (built: this tree's Python does not load a library without the new entry points), in alternation, each in a fresh
         process (--only-bench-py: nothing else)

--bank [--bench-py K [--parent-tree DIR]]  instead of the above (DESIGN.md "PNG bank"): the 224 x 224 frames as our own indexed files at
band_rows 16 and 8, repeated to a bank of --bank-files (4096) places, 256 drawn per call by a fixed device index, with the
caller's buffers.  After the frames of both routes are compared with each other and with the source pixels:

b        the prepacked PngBatch of the drawn files with bands through ops.png_decode_u8: what the parent commit has
c        ops.png_decode_bank_u8 on the bank with the device index; b and c in alternation, each first in turn; each kernel's
         share of both from a torch.profiler trace of ten more calls
a        ops.png_decode_u8 from the drawn files' bytes, clips.png_batch and the upload in every call: 3 repeats
d        ops.draw_clips from the PNG bank beside ops.draw_clips from a JPEG bank of the same frames at quality 90

--alone --against PARENT.so [--bench-py K [--parent-tree DIR]]  instead of the above (DESIGN.md "PNG bands that stand alone"): 256
frames of 224 x 224 and 8 of 1080 x 1920 at band_rows 8 and 16, written by ops.png_encode_u8 with their index (indexed) and
with bands that stand alone (alone).  After the frames of every route are compared with the source pixels, in alternation, each
leg first in turn:

b        the parent commit's istvt_png_decode_bands_u8 (the library given with --against) on the indexed files
c        this tree's ops.png_decode_u8 on the alone files packed with alone=True: one wave per band in the unfilter too
n        this tree's ops.png_decode_u8 on the indexed files packed with alone=True, on the same buffers: no file has the flag
         and every one takes the serial unfilter, which must cost what (b) costs
each kernel's share of b and c from a torch.profiler trace of ten more calls; the files' bytes either way, and how many
band-first rows changed their type (clips.png_filter_rows_host on the distinct frames).  Then the 224 x 224 frames as a bank
of --bank-files places, 256 drawn per call: ops.png_decode_bank_u8 and ops.draw_clips from the indexed bank and from the alone
bank.

--window --against PARENT.so [--bench-py K [--parent-tree DIR]]  instead of the above (DESIGN.md "PNG windows"): window_main's
docstring has the cases.  b: the parent commit's whole decode of an alone bank and its crop; w: this tree's windowed decode and
the crop of the windows through the moved boxes.
"""
import argparse
import io
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import clips, ops  # noqa: E402
from jpeg_decode_bench import DISTINCT, event_ms, say, smooth_image, stats, timed  # noqa: E402


def png_file(frame, level):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, 'PNG', compress_level=level)
    return buf.getvalue()


def fmt(s):
    return '%.3f ms (%.3f-%.3f)' % (s['median_ms'], s['min_ms'], s['max_ms'])


def kernel_shares(call, reps=10, frags=('png_inflate_kernel', 'png_unfilter_kernel')):
    """device time per kernel of `reps` calls -> {kernel name fragment: mean us per call}; a trace without the two kernels is
    an error, not a gap in the table"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for frag in frags:
            if frag in ev.key:
                total = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0)
                out[frag] = out.get(frag, 0.0) + total / reps
    if len(out) != 2:
        raise SystemExit('the profiler trace does not hold %s: %r' % (' / '.join(frags), out))
    return out


def measure(a, lines, res, key, src, n, levels, jpeg_quality, host_reps):
    """one size: src uint8 [DISTINCT, H, W, 3] -> the legs in alternation"""
    dev = torch.device('cuda', torch.cuda.current_device())
    H, W = src.shape[1:3]
    pick = [i % DISTINCT for i in range(n)]
    frames_np = src.numpy()
    files = {lv: [png_file(frames_np[i], lv) for i in range(DISTINCT)] for lv in levels}
    batches = {lv: clips.png_batch([files[lv][i] for i in pick]) for lv in levels}
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    calls, bufs = {}, {}
    for lv, b in batches.items():
        b.on(dev)
        bufs[lv] = (torch.empty((b.scratch_bytes,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                    torch.empty((n,), dtype=torch.int32, device=dev))
        calls['png_l%d' % lv] = (lambda b=b, lv=lv: ops.png_decode_u8(b, out=out, checked=True, buffers=bufs[lv]))
        got, _, status = calls['png_l%d' % lv]()
        clips.check_png_status(status)
        if not torch.equal(got[:DISTINCT].cpu(), src) or not torch.equal(got[n - DISTINCT:].cpu(), src[torch.tensor(pick[n - DISTINCT:])]):
            raise SystemExit('%s level %d: the decoded frames are not the source pixels' % (key, lv))
    if jpeg_quality:
        jf = [clips.jpeg_encode_host(src[i], jpeg_quality, '420', 'row') for i in range(DISTINCT)]
        jb = clips.jpeg_batch([jf[i] for i in pick])
        jbuf = (torch.empty((jb.scratch_bytes,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                torch.empty((n,), dtype=torch.int32, device=dev))
        jout = torch.empty_like(out)
        calls['jpeg_q%d' % jpeg_quality] = lambda: ops.jpeg_decode_u8(jb, out=jout, checked=True, buffers=jbuf)
        clips.check_jpeg_status(calls['jpeg_q%d' % jpeg_quality]()[2])
    ts = {k: [] for k in calls}
    for r in range(a.warmup + a.reps):
        for k, fn in calls.items():
            t = event_ms(fn)
            if r >= a.warmup:
                ts[k].append(t)
    # the host route: PIL decodes every file of the batch, the decoded bytes are uploaded from pinned memory
    staging = torch.empty((n, H, W, 3), dtype=torch.uint8).pin_memory()
    view = staging.numpy()

    def host_route(lv):
        for j, i in enumerate(pick):
            view[j] = np.asarray(Image.open(io.BytesIO(files[lv][i])).convert('RGB'))
        return staging.to(dev, non_blocking=True)
    th, tu = {lv: [] for lv in levels}, {lv: [] for lv in levels}
    for r in range(1 + host_reps):
        for lv in levels:
            x = timed(lambda: host_route(lv))
            host = [batches[lv].data, batches[lv].images]
            y = timed(lambda: [t.to(dev, non_blocking=True) for t in host])
            if r >= 1:
                th[lv].append(x)
                tu[lv].append(y)
    tw = [timed(lambda: staging.to(dev, non_blocking=True)) for _ in range(1 + host_reps)][1:]
    if not torch.equal(host_route(levels[0])[:DISTINCT].cpu(), src):
        raise SystemExit('%s: PIL does not give the source pixels' % key)
    res[key] = {'frames': n, 'H': H, 'W': W, 'decoded_bytes': n * H * W * 3, 'upload_decoded': stats(tw)}
    say(lines, '%s: %d frames of %d x %d, %.2f MB decoded (3 bytes per pixel), its upload alone %s' % (key, n, H, W, n * H * W * 3e-6, fmt(stats(tw))))
    for lv in levels:
        b, k = batches[lv], 'png_l%d' % lv
        up = b.data.numel() + 4 * b.images.numel()
        shares = kernel_shares(calls[k])
        sd, sh, su = stats(ts[k]), stats(th[lv]), stats(tu[lv])
        res[key][k] = {'device': sd, 'host_route': sh, 'upload_compressed': su, 'uploaded_bytes': up, 'stream_bytes': b.nbytes,
                       'scratch_bytes': b.scratch_bytes, 'kernel_us': shares}
        share = 'inflate %.0f us, unfilter %.0f us per call' % (shares['png_inflate_kernel'], shares['png_unfilter_kernel'])
        say(lines, '  png_decode_u8, PIL compress level %d: %s on the device = %.2f us per frame, %.2f ns per pixel (%s) | uploaded %.2f MB '
            'against %.2f MB decoded = 1 / %.2f, its upload %s | the host route (PIL decode + upload of the pixels) %s = %.1f x the '
            'device call' % (lv, fmt(sd), sd['median_ms'] * 1e3 / n, sd['median_ms'] * 1e6 / (n * H * W), share, up * 1e-6, n * H * W * 3e-6,
                             n * H * W * 3 / up, fmt(su), fmt(sh), sh['median_ms'] / sd['median_ms']))
    if jpeg_quality:
        k = 'jpeg_q%d' % jpeg_quality
        up = sum(t.numel() * t.element_size() for t in (jb.data, jb.images, jb.segments, jb.qtabs, jb.htabs))
        res[key][k] = {'device': stats(ts[k]), 'uploaded_bytes': up}
        say(lines, '  jpeg_decode_u8 on the same frames at quality %d (a restart marker per MCU row; lossy): %s, uploaded %.2f MB'
            % (jpeg_quality, fmt(stats(ts[k])), up * 1e-6))


def bands_size(a, lines, res, key, src, n, other):
    """--bands, one size: src uint8 [DISTINCT, H, W, 3] -> the legs in alternation for every band_rows"""
    from istvt_amd import _lib
    dev = torch.device('cuda', torch.cuda.current_device())
    H, W = src.shape[1:3]
    pick = [i % DISTINCT for i in range(n)]
    src_dev = src.to(dev)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    staging = torch.empty((n, H, W, 3), dtype=torch.uint8).pin_memory()
    view = staging.numpy()
    res[key] = {'frames': n, 'H': H, 'W': W}
    say(lines, '%s: %d frames of %d x %d' % (key, n, H, W))
    for R in a.band_rows:
        distinct = ops.png_encode_u8(src_dev, R, index=True).files()       # files() raises where a status is not 0
        plain_bytes = sum(len(f) for f in ops.png_encode_u8(src_dev, R).files())
        files = [distinct[i] for i in pick]
        bb, bs = clips.png_batch(files, bands='index'), clips.png_batch(files)
        bufs = {}
        for name, b in (('bands', bb), ('seq', bs)):
            b.on(dev)
            bufs[name] = (torch.empty((b.scratch_bytes,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                          torch.empty((n,), dtype=torch.int32, device=dev))
        calls = {'bands': lambda: ops.png_decode_u8(bb, out=out, checked=True, buffers=bufs['bands']),
                 'seq': lambda: ops.png_decode_u8(bs, out=out, checked=True, buffers=bufs['seq'])}
        if other is not None:
            d, (scratch, sizes, status) = bs.on(dev), bufs['seq']
            args = _lib.JpegDecodeArgs(
                bytes=d.data.data_ptr(), nbytes=bs.nbytes, images=d.images.data_ptr(), images_host=bs.images.data_ptr(),
                scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), out=out.data_ptr(), sizes=sizes.data_ptr(),
                status=status.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, n=n, Hc=H, Wc=W)
            calls['parent'] = lambda: (_lib.check(other.istvt_png_decode_u8(ctypes.byref(args), bs.raw_stride), 'parent istvt_png_decode_u8'),
                                       (out, sizes, status))[1]
        for name, fn in calls.items():                            # the frames before anything is timed
            out.fill_(7)
            got, _, status = fn()
            clips.check_png_status(status)
            if not torch.equal(got[:DISTINCT], src_dev) or not torch.equal(got[n - DISTINCT:].cpu(), src[torch.tensor(pick[n - DISTINCT:])]):
                raise SystemExit('%s band_rows %d, %s: the decoded frames are not the source pixels' % (key, R, name))
        ts = {k: [] for k in calls}
        for r in range(a.warmup + a.reps):
            order = list(calls.items())
            for k, fn in order[r % len(order):] + order[:r % len(order)]:      # each leg first in turn
                t = event_ms(fn)
                if r >= a.warmup:
                    ts[k].append(t)

        def host_route():
            for j, i in enumerate(pick):
                view[j] = np.asarray(Image.open(io.BytesIO(distinct[i])).convert('RGB'))
            return staging.to(dev, non_blocking=True)
        th = [timed(host_route) for _ in range(1 + a.host_reps)][1:]
        if not torch.equal(host_route()[:DISTINCT], src_dev):
            raise SystemExit('%s: PIL does not give the source pixels of an indexed file' % key)
        te = {False: [], True: []}
        for r in range(a.warmup + a.reps):
            for index in ((False, True) if r % 2 else (True, False)):
                t = event_ms(lambda: ops.png_encode_u8(src_dev, R, index=index))
                if r >= a.warmup:
                    te[index].append(t)
        shares = kernel_shares(calls['bands'], frags=('png_inflate_bands_kernel', 'png_unfilter_bands_kernel'))
        st = {k: stats(v) for k, v in ts.items()}
        row = {'bands_per_file': int(bb.bands.shape[0]) // n, 'waves': int(bb.bands.shape[0]), 'stream_bytes': bb.nbytes,
               'index_bytes': sum(len(f) for f in distinct) - plain_bytes, 'file_bytes': sum(len(f) for f in distinct),
               'host_route': stats(th), 'kernel_us': shares, 'encode': stats(te[False]), 'encode_indexed': stats(te[True])}
        row.update(st)
        res[key]['band_rows_%d' % R] = row
        text = ('  band_rows %d: %d bands per file, %d waves in place of %d | by bands %s (inflate %.0f us, unfilter %.0f us per call = %.0f %% '
                'and %.0f %%) | sequential, this tree %s'
                % (R, row['bands_per_file'], row['waves'], n, fmt(st['bands']), shares['png_inflate_bands_kernel'],
                   shares['png_unfilter_bands_kernel'], 100 * shares['png_inflate_bands_kernel'] / sum(shares.values()),
                   100 * shares['png_unfilter_bands_kernel'] / sum(shares.values()), fmt(st['seq'])))
        if other is not None:
            p_ = st['parent']
            text += (' | sequential, the parent\'s library %s, its spread %.3f ms | parent / bands = %.2f x, parent - bands = %.3f ms = %.1f '
                     'spreads | this tree\'s sequential / the parent\'s = %.4f'
                     % (fmt(p_), p_['max_ms'] - p_['min_ms'], p_['median_ms'] / st['bands']['median_ms'],
                        p_['median_ms'] - st['bands']['median_ms'],
                        (p_['median_ms'] - st['bands']['median_ms']) / max(p_['max_ms'] - p_['min_ms'], 1e-9),
                        st['seq']['median_ms'] / p_['median_ms']))
        text += (' | the host route (PIL decode + upload of the pixels) %s = %.2f x the call by bands | files %.2f MB, of which the index '
                 '%.1f kB | encode %s, with the index %s'
                 % (fmt(stats(th)), stats(th)['median_ms'] / st['bands']['median_ms'], row['file_bytes'] * 1e-6 * n / DISTINCT,
                    row['index_bytes'] * 1e-3 * n / DISTINCT, fmt(stats(te[False])), fmt(stats(te[True]))))
        say(lines, text)


def bench_py(a, lines, res):
    """bench.py at its defaults in fresh processes, this tree and the parent's checkout in alternation -> its result lines"""
    legs = [('this', ROOT)] + ([('parent', os.path.abspath(a.parent_tree))] if a.parent_tree else [])
    res['bench_py'] = {k: [] for k, _ in legs}
    for r in range(a.bench_py):
        for name, tree in (legs if r % 2 == 0 else legs[::-1]):
            env = dict(os.environ)
            env.pop('ISTVT_LIB', None)
            p = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1'], env=env, cwd=tree, capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit('bench.py (%s) failed:\n%s' % (name, p.stderr[-2000:]))
            line = [l for l in p.stdout.splitlines() if l.startswith('{')][-1]
            res['bench_py'][name].append(json.loads(line))
            say(lines, 'bench.py, %s, run %d: %s' % (name, r, line[:400]))


def bands_main(a):
    if not torch.cuda.is_available():
        raise SystemExit('png_decode_bench.py measures on a GPU; none is visible')
    from istvt_amd import _lib
    torch.zeros(1, device='cuda')
    other = None
    if a.against:
        other = ctypes.CDLL(os.path.abspath(a.against))
        other.istvt_png_decode_u8.argtypes, other.istvt_png_decode_u8.restype = _lib.SIGNATURES['istvt_png_decode_u8'], ctypes.c_int
    lines, res = [], {}
    S = a.size
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    if not a.only_bench_py:
        bands_size(a, lines, res, 'step', src, a.frames, other)
    if not a.no_large and not a.only_bench_py:
        big = torch.stack([torch.from_numpy(smooth_image(1080, 1920, 2000 + i)) for i in range(DISTINCT)])
        bands_size(a, lines, res, 'large', big, DISTINCT, other)
    if a.bench_py:
        bench_py(a, lines, res)
    line = json.dumps({'png_bands_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def bank_main(a):
    if not torch.cuda.is_available():
        raise SystemExit('png_decode_bench.py measures on a GPU; none is visible')
    dev = torch.device('cuda', torch.cuda.current_device())
    torch.zeros(1, device=dev)
    lines, res = [], {}
    S, n, N = a.size, a.frames, a.bank_files
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    src_dev = src.to(dev)
    g = torch.Generator().manual_seed(31)
    index = torch.randint(0, N, (n,), generator=g, dtype=torch.int32)
    idx = index.to(dev)
    drawn = [i % DISTINCT for i in index.tolist()]
    want = src_dev[torch.tensor(drawn, device=dev)]
    out_b, out_c = (torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    say(lines, 'bank: %d places of %d x %d (%d distinct files repeated), %d drawn per call by a device index' % (N, S, S, DISTINCT, n))
    for R in a.band_rows:
        if a.only_bench_py:
            break
        distinct = ops.png_encode_u8(src_dev, R, index=True).files()
        headers = [clips.png_parse(f) for f in distinct]
        bank = clips.png_bank([headers[i % DISTINCT] for i in range(N)])
        bank.on(dev)
        files = [distinct[i] for i in drawn]
        batch = clips.png_batch([headers[i] for i in drawn], bands='index')
        batch.on(dev)
        mk = lambda need: (torch.empty((need,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                           torch.empty((n,), dtype=torch.int32, device=dev))
        buf_b, buf_c = mk(batch.scratch_bytes), mk(clips.png_bank_scratch_bytes(bank, n))
        calls = {'b': lambda: ops.png_decode_u8(batch, out=out_b, checked=True, buffers=buf_b),
                 'c': lambda: ops.png_decode_bank_u8(bank, idx, out=out_c, buffers=buf_c)}
        for k, fn in calls.items():
            got, _, status = fn()
            clips.check_png_status(status)
            if not torch.equal(got, want):
                raise SystemExit('band_rows %d, leg %s: the decoded frames are not the source pixels' % (R, k))
        ts = {k: [] for k in calls}
        for r in range(a.warmup + a.reps):
            order = list(calls.items())
            for k, fn in order[r % 2:] + order[:r % 2]:               # each leg first in turn
                t = event_ms(fn)
                if r >= a.warmup:
                    ts[k].append(t)
        ta = [timed(lambda: ops.png_decode_u8(files, bands='index')) for _ in range(1 + 3)][1:]
        sb = kernel_shares(calls['b'], frags=('png_inflate_bands_kernel', 'png_unfilter_bands_kernel'))
        sc = kernel_shares(calls['c'], frags=('png_bank_inflate_kernel', 'png_bank_unfilter_kernel'))
        st = {k: stats(v) for k, v in ts.items()}
        inside = st['b']['min_ms'] <= st['c']['median_ms'] <= st['b']['max_ms']
        row = {'bands_per_file': bank.band_max, 'waves_b': int(batch.bands.shape[0]), 'waves_c': n * bank.band_max, 'bank_bytes': bank.nbytes,
               'b': st['b'], 'c': st['c'], 'a': stats(ta), 'kernel_us_b': sb, 'kernel_us_c': sc, 'c_inside_b_range': inside}
        res['band_rows_%d' % R] = row
        say(lines, '  band_rows %d: %d bands per file, bank of %.1f MB | (b) prepacked PngBatch with bands %s (inflate %.0f us, unfilter %.0f us '
            'per call) | (c) the bank by a device index %s (inflate %.0f us, unfilter %.0f us per call) | c / b = %.4f, c - b = %.3f ms, the '
            'range of b %.3f ms: c is %s it | (a) from bytes, png_batch and upload every call %s = %.1f x c'
            % (R, bank.band_max, bank.nbytes * 1e-6, fmt(st['b']), sb['png_inflate_bands_kernel'], sb['png_unfilter_bands_kernel'], fmt(st['c']),
               sc['png_bank_inflate_kernel'], sc['png_bank_unfilter_kernel'], st['c']['median_ms'] / st['b']['median_ms'],
               st['c']['median_ms'] - st['b']['median_ms'], st['b']['max_ms'] - st['b']['min_ms'], 'inside' if inside else 'OUTSIDE',
               fmt(stats(ta)), stats(ta)['median_ms'] / st['c']['median_ms']))
        if R == a.band_rows[0]:                                     # (d) the whole input side from either bank
            T = 8
            B = n // T
            jh = [clips.jpeg_parse(f) for f in ops.jpeg_encode_u8(src_dev, 90, '420', 'row').files()]
            jbank = clips.jpeg_bank([jh[i % DISTINCT] for i in range(N)])
            jbank.on(dev)
            out_d = torch.empty((B, T, S, S, 3), dtype=torch.uint8, device=dev)
            plans = {k: clips.BatchPlan(bk, [(0, N, 0)], T=T, B=B, seed=5).on(dev) for k, bk in (('png', bank), ('jpeg', jbank))}
            dcalls = {'png': lambda: ops.draw_clips(bank, plans['png'], S, out=out_d),
                      'jpeg': lambda: ops.draw_clips(jbank, plans['jpeg'], S, out=out_d)}
            td = {k: [] for k in dcalls}
            for r in range(a.warmup + a.reps):
                order = list(dcalls.items())
                for k, fn in order[r % 2:] + order[:r % 2]:
                    t = event_ms(fn)
                    if r >= a.warmup:
                        td[k].append(t)
            row['draw_clips_png'], row['draw_clips_jpeg'] = stats(td['png']), stats(td['jpeg'])
            say(lines, '  (d) draw_clips, B = %d clips of T = %d at %d x %d, all stages: from the PNG bank %s | from a JPEG bank of the same '
                'frames at quality 90 %s' % (B, T, S, S, fmt(stats(td['png'])), fmt(stats(td['jpeg']))))
            del jbank, plans
        bank._on.clear()
    if a.bench_py:
        bench_py(a, lines, res)
    line = json.dumps({'png_bank_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def alone_size(a, lines, res, key, src, n, other):
    """--alone, one size: src uint8 [DISTINCT, H, W, 3] -> legs b, c and n in alternation for every band_rows"""
    from istvt_amd import _lib
    dev = torch.device('cuda', torch.cuda.current_device())
    H, W = src.shape[1:3]
    pick = [i % DISTINCT for i in range(n)]
    src_dev = src.to(dev)
    want_tail = src[torch.tensor(pick[n - DISTINCT:])]
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    res[key] = {'frames': n, 'H': H, 'W': W}
    say(lines, '%s: %d frames of %d x %d' % (key, n, H, W))
    for R in a.band_rows:
        indexed = ops.png_encode_u8(src_dev, R, index=True).files()
        alone = ops.png_encode_u8(src_dev, R, index=True, alone=True).files()
        changed = rows = 0
        for f in src.numpy():                                     # on the host: the types of the band-first rows either way
            free, kept = clips.png_filter_rows_host(f)[::R, 0], clips.png_filter_rows_host(f, alone_rows=R)[::R, 0]
            changed, rows = changed + int((free != kept).sum()), rows + len(free)
        bi = clips.png_batch([indexed[i] for i in pick], bands='index')
        bc = clips.png_batch([alone[i] for i in pick], bands='index', alone=True)
        bn = clips.png_batch([indexed[i] for i in pick], bands='index', alone=True)
        assert sum(bc.alone.tolist()) == n and sum(bn.alone.tolist()) == 0 and bc.scratch_bytes == bi.scratch_bytes == bn.scratch_bytes
        for b in (bi, bc, bn):
            b.on(dev)
        bufs = (torch.empty((bi.scratch_bytes,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                torch.empty((n,), dtype=torch.int32, device=dev))
        d = bi.on(dev)
        args = _lib.JpegDecodeArgs(
            bytes=d.data.data_ptr(), nbytes=bi.nbytes, images=d.images.data_ptr(), images_host=bi.images.data_ptr(),
            segments=d.bands.data_ptr(), segments_host=bi.bands.data_ptr(), scratch=bufs[0].data_ptr(), scratch_bytes=bufs[0].numel(),
            out=out.data_ptr(), sizes=bufs[1].data_ptr(), status=bufs[2].data_ptr(), stream=torch.cuda.current_stream().cuda_stream, n=n,
            nseg=int(bi.bands.shape[0]), Hc=H, Wc=W)
        calls = {'b': lambda: (_lib.check(other.istvt_png_decode_bands_u8(ctypes.byref(args), bi.raw_stride), 'parent istvt_png_decode_bands_u8'),
                               (out, bufs[1], bufs[2]))[1],
                 'c': lambda: ops.png_decode_u8(bc, out=out, checked=True, buffers=bufs),
                 'n': lambda: ops.png_decode_u8(bn, out=out, checked=True, buffers=bufs)}
        for name, fn in calls.items():                            # the frames before anything is timed
            out.fill_(7)
            got, _, status = fn()
            clips.check_png_status(status)
            if not torch.equal(got[:DISTINCT], src_dev) or not torch.equal(got[n - DISTINCT:].cpu(), want_tail):
                raise SystemExit('%s band_rows %d, leg %s: the decoded frames are not the source pixels' % (key, R, name))
        ts = {k: [] for k in calls}
        for r in range(a.warmup + a.reps):
            order = list(calls.items())
            for k, fn in order[r % len(order):] + order[:r % len(order)]:      # each leg first in turn
                t = event_ms(fn)
                if r >= a.warmup:
                    ts[k].append(t)
        sb = kernel_shares(calls['b'], frags=('png_inflate_bands_kernel', 'png_unfilter_bands_kernel'))
        sc = kernel_shares(calls['c'], frags=('png_inflate_bands_kernel', 'png_unfilter_alone_kernel'))
        st = {k: stats(v) for k, v in ts.items()}
        spread = max(st['b']['max_ms'] - st['b']['min_ms'], 1e-9)
        inside = st['b']['min_ms'] <= st['n']['median_ms'] <= st['b']['max_ms']
        bytes_i, bytes_a = sum(len(f) for f in indexed), sum(len(f) for f in alone)
        res[key]['band_rows_%d' % R] = dict(st, kernel_us_b=sb, kernel_us_c=sc, waves=int(bi.bands.shape[0]), bytes_indexed=bytes_i,
                                            bytes_alone=bytes_a, band_first_rows=rows, band_first_rows_changed=changed, n_inside_b_range=inside)
        say(lines, '  band_rows %d, %d waves: (b) the parent\'s banded call on the indexed files %s, its range %.3f ms (inflate %.0f us, unfilter '
            '%.0f us per call) | (c) this tree on the alone files %s (inflate %.0f us, unfilter %.0f us per call) | b / c = %.2f x, b - c = '
            '%.3f ms = %.1f ranges of b | (n) this tree on the indexed files packed with alone=True %s: n - b = %.3f ms, n is %s the range '
            'of b | the %d distinct files: indexed %d bytes, alone %d bytes = %+.3f %%; %d of %d band-first rows changed their type'
            % (R, int(bi.bands.shape[0]), fmt(st['b']), spread, sb['png_inflate_bands_kernel'], sb['png_unfilter_bands_kernel'], fmt(st['c']),
               sc['png_inflate_bands_kernel'], sc['png_unfilter_alone_kernel'], st['b']['median_ms'] / st['c']['median_ms'],
               st['b']['median_ms'] - st['c']['median_ms'], (st['b']['median_ms'] - st['c']['median_ms']) / spread, fmt(st['n']),
               st['n']['median_ms'] - st['b']['median_ms'], 'inside' if inside else 'OUTSIDE', DISTINCT, bytes_i, bytes_a,
               100.0 * (bytes_a - bytes_i) / bytes_i, changed, rows))


def alone_bank(a, lines, res, src):
    """--alone, the bank: ops.png_decode_bank_u8 and ops.draw_clips from the indexed bank and from the alone bank"""
    dev = torch.device('cuda', torch.cuda.current_device())
    S, n, N = a.size, a.frames, a.bank_files
    src_dev = src.to(dev)
    g = torch.Generator().manual_seed(31)
    index = torch.randint(0, N, (n,), generator=g, dtype=torch.int32)
    idx = index.to(dev)
    want = src_dev[torch.tensor([i % DISTINCT for i in index.tolist()], device=dev)]
    out = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    say(lines, 'bank: %d places of %d x %d (%d distinct files repeated), %d drawn per call by a device index' % (N, S, S, DISTINCT, n))
    for R in a.band_rows:
        banks = {}
        for k, alone in (('b', False), ('c', True)):
            hs = [clips.png_parse(f) for f in ops.png_encode_u8(src_dev, R, index=True, alone=alone).files()]
            banks[k] = clips.png_bank([hs[i % DISTINCT] for i in range(N)], alone=alone)
            banks[k].on(dev)
        buf = (torch.empty((clips.png_bank_scratch_bytes(banks['b'], n),), dtype=torch.uint8, device=dev),
               torch.empty((n, 2), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
        T = 8
        B = n // T
        out_d = torch.empty((B, T, S, S, 3), dtype=torch.uint8, device=dev)
        plans = {k: clips.BatchPlan(bk, [(0, N, 0)], T=T, B=B, seed=5).on(dev) for k, bk in banks.items()}
        calls = {k: (lambda k=k: ops.png_decode_bank_u8(banks[k], idx, out=out, buffers=buf)) for k in banks}
        dcalls = {k: (lambda k=k: ops.draw_clips(banks[k], plans[k], S, out=out_d)) for k in banks}
        for k, fn in calls.items():
            got, _, status = fn()
            clips.check_png_status(status)
            if not torch.equal(got, want):
                raise SystemExit('bank, band_rows %d, leg %s: the decoded frames are not the source pixels' % (R, k))
        row = {}
        for tag, legs in (('decode', calls), ('draw_clips', dcalls)):
            ts = {k: [] for k in legs}
            for r in range(a.warmup + a.reps):
                order = list(legs.items())
                for k, fn in order[r % 2:] + order[:r % 2]:
                    t = event_ms(fn)
                    if r >= a.warmup:
                        ts[k].append(t)
            row[tag] = {k: stats(v) for k, v in ts.items()}
        sb = kernel_shares(calls['b'], frags=('png_bank_inflate_kernel', 'png_bank_unfilter_kernel'))
        sc = kernel_shares(calls['c'], frags=('png_bank_inflate_kernel', 'png_bank_unfilter_alone_kernel'))
        row.update(kernel_us_b=sb, kernel_us_c=sc)
        res['bank_band_rows_%d' % R] = row
        db, dc = row['decode']['b'], row['decode']['c']
        say(lines, '  band_rows %d: png_decode_bank_u8, the indexed bank %s, its range %.3f ms (inflate %.0f us, unfilter %.0f us per call) | the '
            'alone bank %s (inflate %.0f us, unfilter %.0f us per call) | b - c = %.3f ms = %.1f ranges of b | draw_clips, B = %d clips of T = '
            '%d, all stages: from the indexed bank %s, from the alone bank %s'
            % (R, fmt(db), db['max_ms'] - db['min_ms'], sb['png_bank_inflate_kernel'], sb['png_bank_unfilter_kernel'], fmt(dc),
               sc['png_bank_inflate_kernel'], sc['png_bank_unfilter_alone_kernel'], db['median_ms'] - dc['median_ms'],
               (db['median_ms'] - dc['median_ms']) / max(db['max_ms'] - db['min_ms'], 1e-9), B, T, fmt(row['draw_clips']['b']),
               fmt(row['draw_clips']['c'])))
        for bk in banks.values():
            bk._on.clear()


def alone_main(a):
    if not torch.cuda.is_available():
        raise SystemExit('png_decode_bench.py measures on a GPU; none is visible')
    from istvt_amd import _lib
    torch.zeros(1, device='cuda')
    lines, res = [], {}
    if not a.only_bench_py:
        if not a.against:
            raise SystemExit('--alone measures against the parent commit\'s library: --against PARENT.so')
        other = ctypes.CDLL(os.path.abspath(a.against))
        other.istvt_png_decode_bands_u8.argtypes, other.istvt_png_decode_bands_u8.restype = _lib.SIGNATURES['istvt_png_decode_bands_u8'], ctypes.c_int
        src = torch.stack([torch.from_numpy(smooth_image(a.size, a.size, 1000 + i)) for i in range(DISTINCT)])
        alone_size(a, lines, res, 'step', src, a.frames, other)
        if not a.no_large:
            big = torch.stack([torch.from_numpy(smooth_image(1080, 1920, 2000 + i)) for i in range(DISTINCT)])
            alone_size(a, lines, res, 'large', big, DISTINCT, other)
        alone_bank(a, lines, res, src)
    if a.bench_py:
        bench_py(a, lines, res)
    line = json.dumps({'png_alone_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def window_case(a, lines, res, key, bank, src_dev, index, boxes, S, other):
    """--window, one case: m places of `bank` through `boxes` -> (b) the parent's whole decode and the crop, (w) this tree's
    windowed decode and the crop, in alternation, each first in turn"""
    from istvt_amd import _lib
    dev = src_dev.device
    m, H, W = len(index), bank.Hmax, bank.Wmax
    idx, bx = torch.tensor(index, dtype=torch.int32, device=dev), torch.tensor(boxes, dtype=torch.int32, device=dev)
    rows = clips.check_png_window(bank, torch.tensor(boxes, dtype=torch.int32), index)[1]      # the smallest window that fits them
    d = bank.on(dev)
    whole = torch.empty((m, H, W, 3), dtype=torch.uint8, device=dev)
    bbuf = (torch.empty((clips.png_bank_scratch_bytes(bank, m),), dtype=torch.uint8, device=dev),
            torch.empty((m, 2), dtype=torch.int32, device=dev), torch.empty((m,), dtype=torch.int32, device=dev))
    wins = torch.empty((m, rows, W, 3), dtype=torch.uint8, device=dev)
    wbuf = (torch.empty((clips.png_window_scratch_bytes(bank, m, rows),), dtype=torch.uint8, device=dev),
            torch.empty((m, 2), dtype=torch.int32, device=dev), torch.empty((m,), dtype=torch.int32, device=dev))
    cut_b, cut_w = (torch.empty((m, S, S, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    args = _lib.JpegDecodeArgs(bytes=d.data.data_ptr(), nbytes=bank.first_byte + bank.nbytes, images=d.images.data_ptr(),
                               images_host=idx.data_ptr(), segments=d.segments.data_ptr(), scratch=bbuf[0].data_ptr(),
                               scratch_bytes=bbuf[0].numel(), out=whole.data_ptr(), sizes=bbuf[1].data_ptr(), status=bbuf[2].data_ptr(),
                               stream=stream, n=bank.n, nseg=bank.nband, Hc=H, Wc=W)

    def leg_b():
        _lib.check(other.istvt_png_decode_bank_alone_u8(ctypes.byref(args), m, bank.band_max, bank.raw_stride), 'parent istvt_png_decode_bank_alone_u8')
        _lib.check(other.istvt_crop_resize_u8(whole.data_ptr(), whole.numel(), H, W, bx.data_ptr(), cut_b.data_ptr(), m, S, stream),
                   'parent istvt_crop_resize_u8')
        return cut_b, bbuf[2]

    def leg_w():
        got = ops.png_decode_window_u8(bank, bx, index=idx, rows=rows, out=wins, buffers=wbuf)
        return ops.crop_resize_u8(got[0], got[1], S, out=cut_w, checked=True), got[3]

    for name, fn in (('b', leg_b), ('w', leg_w)):                 # the pixels before anything is timed
        for t in ((whole, cut_b) if name == 'b' else (wins, cut_w)):
            t.fill_(7)
        cut, status = fn()
        clips.check_png_status(status)
        torch.cuda.synchronize()
        for j in (0, m // 2, m - 1):
            y0, x0, h, w = boxes[j]
            frame = src_dev[index[j] % DISTINCT]
            if name == 'b' and not torch.equal(whole[j], frame):
                raise SystemExit('%s, leg b: the decoded frames are not the source pixels' % key)
            if name == 'w':
                at = clips.png_window_boxes_at(bank, m, rows)
                w0 = int(wbuf[0][at:at + 20 * m].view(torch.int32)[4 * m + j])                    # the origins stand behind the boxes
                R = clips._png_window_files(bank)[index[j]][3]
                w1 = min(H, ((y0 + h - 1) // R + 1) * R)
                if w0 != y0 // R * R or not torch.equal(wins[j, :w1 - w0], frame[w0:w1]):
                    raise SystemExit('%s, leg w: the windows are not the source pixels' % key)
    if not torch.equal(cut_b, cut_w):
        raise SystemExit('%s: the crops of the two routes differ' % key)
    legs = {'b': leg_b, 'w': leg_w}
    ts = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        order = list(legs.items())
        for k, fn in order[r % 2:] + order[:r % 2]:
            t = event_ms(fn)
            if r >= a.warmup:
                ts[k].append(t)
    st = {k: stats(v) for k, v in ts.items()}
    sb = kernel_shares(leg_b, frags=('png_bank_inflate_kernel', 'png_bank_unfilter_alone_kernel'))
    sw = kernel_shares(leg_w, frags=('png_window_inflate_kernel', 'png_window_unfilter_kernel'))
    spread = max(st['b']['max_ms'] - st['b']['min_ms'], 1e-9)
    diff = st['b']['median_ms'] - st['w']['median_ms']
    inside = st['b']['min_ms'] <= st['w']['median_ms'] <= st['b']['max_ms']
    bytes_b, bytes_w = whole.numel() + bbuf[0].numel(), wins.numel() + wbuf[0].numel()
    res[key] = dict(st, kernel_us_b=sb, kernel_us_w=sw, places=m, rows=rows, bytes_b=bytes_b, bytes_w=bytes_w, w_inside_b_range=inside,
                    waves_b=m * bank.band_max, waves_w=m * clips.png_window_bands(bank, rows))
    say(lines, '  %s: %d places, window of %d rows, %d waves against %d | (b) the parent\'s whole decode and the crop %s, its range %.3f ms '
        '(inflate %.0f us, unfilter %.0f us per call) | (w) the windowed decode and the crop %s (inflate %.0f us, unfilter %.0f us per call) | '
        'b - w = %.3f ms = %.1f ranges of b, b / w = %.2f x, w is %s the range of b | out + scratch: %.1f MB against %.1f MB'
        % (key, m, rows, m * clips.png_window_bands(bank, rows), m * bank.band_max, fmt(st['b']), spread, sb['png_bank_inflate_kernel'],
           sb['png_bank_unfilter_alone_kernel'], fmt(st['w']), sw['png_window_inflate_kernel'], sw['png_window_unfilter_kernel'], diff,
           diff / spread, st['b']['median_ms'] / st['w']['median_ms'], 'inside' if inside else 'OUTSIDE', bytes_w / 1e6, bytes_b / 1e6))


def window_main(a):
    """--window --against PARENT.so (DESIGN.md "PNG windows"): frames of 1080 x 1920 at band_rows 8 and 16, written by
    ops.png_encode_u8(alone=True), as a bank of 32 places (8 distinct frames); 8 and 256 places drawn by a device index through
    boxes of 360 x 360 at a fixed and at a random y0 and through the degenerate box of all 1080 rows; 256 places of 224 x 224
    through whole-image boxes; ops.draw_clips with and without window=True at 32 clips of 8 frames.  (b) is the parent commit's
    istvt_png_decode_bank_alone_u8 and istvt_crop_resize_u8 from the library given with --against, (w) this tree's
    ops.png_decode_window_u8 and ops.crop_resize_u8; caller's buffers, the legs in alternation, each first in turn."""
    if not torch.cuda.is_available():
        raise SystemExit('png_decode_bench.py measures on a GPU; none is visible')
    from istvt_amd import _lib
    torch.zeros(1, device='cuda')
    dev = torch.device('cuda', torch.cuda.current_device())
    lines, res = [], {}
    if not a.only_bench_py:
        if not a.against:
            raise SystemExit('--window measures against the parent commit\'s library: --against PARENT.so')
        other = ctypes.CDLL(os.path.abspath(a.against))
        for name in ('istvt_png_decode_bank_alone_u8', 'istvt_crop_resize_u8'):
            getattr(other, name).argtypes, getattr(other, name).restype = _lib.SIGNATURES[name], ctypes.c_int
        S, N = a.size, 32
        g = torch.Generator().manual_seed(41)
        big = torch.stack([torch.from_numpy(smooth_image(1080, 1920, 2000 + i)) for i in range(DISTINCT)]).to(dev)
        small = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)]).to(dev)
        for R in a.band_rows:
            hs = [clips.png_parse(f) for f in ops.png_encode_u8(big, R, index=True, alone=True).files()]
            bank = clips.png_bank([hs[i % DISTINCT] for i in range(N)], alone=True)
            say(lines, 'band_rows %d: a bank of %d places of 1080 x 1920 (%d distinct frames), crops of %d x %d' % (R, N, DISTINCT, S, S))
            for m in (8, a.frames):
                index = torch.randint(0, N, (m,), generator=g).tolist()
                ys = torch.randint(0, 1080 - 360 + 1, (m,), generator=g).tolist()
                for tag, boxes in (('fixed_y0', [[360, 780, 360, 360]] * m), ('random_y0', [[y, 780, 360, 360] for y in ys]),
                                   ('all_rows', [[0, 420, 1080, 1080]] * m)):
                    window_case(a, lines, res, 'r%d_%d_places_%s' % (R, m, tag), bank, big, index, boxes, S, other)
            T, B = 8, 32
            base = torch.tensor([[360, 780, 360, 360]] * N, dtype=torch.int32)
            out_d = torch.empty((B, T, S, S, 3), dtype=torch.uint8, device=dev)
            plans = {k: clips.BatchPlan(bank, [(0, N, 0)], T=T, B=B, base=base, seed=5).on(dev) for k in ('whole', 'window')}
            legs = {k: (lambda k=k: ops.draw_clips(bank, plans[k], S, out=out_d, window=k == 'window')) for k in plans}
            first = {k: fn()[0].clone() for k, fn in legs.items()}
            if not torch.equal(first['whole'], first['window']):
                raise SystemExit('draw_clips: the two routes differ')
            ts = {k: [] for k in legs}
            for r in range(a.warmup + a.reps):
                order = list(legs.items())
                for k, fn in order[r % 2:] + order[:r % 2]:
                    t = event_ms(fn)
                    if r >= a.warmup:
                        ts[k].append(t)
            st = {k: stats(v) for k, v in ts.items()}
            res['r%d_draw_clips' % R] = st
            say(lines, '  draw_clips, %d clips of %d frames, base boxes of 360 x 360, all stages: %s without window=True, %s with it (this tree both)'
                % (B, T, fmt(st['whole']), fmt(st['window'])))
            bank._on.clear()
            hs = [clips.png_parse(f) for f in ops.png_encode_u8(small, R, index=True, alone=True).files()]
            bank = clips.png_bank([hs[i % DISTINCT] for i in range(N)], alone=True)
            index = torch.randint(0, N, (a.frames,), generator=g).tolist()
            window_case(a, lines, res, 'r%d_%d_places_of_%d_whole_image' % (R, a.frames, S), bank, small, index, [[0, 0, S, S]] * a.frames, S, other)
            bank._on.clear()
    if a.bench_py:
        bench_py(a, lines, res)
    line = json.dumps({'png_window_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--frames', type=int, default=256)
    p.add_argument('--size', type=int, default=224)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--host-reps', type=int, default=3)
    p.add_argument('--no-large', action='store_true')
    p.add_argument('--out', default=None)
    p.add_argument('--bands', action='store_true')
    p.add_argument('--band-rows', type=int, nargs='+', default=[8, 16, 32])
    p.add_argument('--against', default=None, help='another build of the library (the parent commit\'s) for the sequential leg')
    p.add_argument('--bench-py', type=int, default=0, help='runs of bench.py per library, in alternation')
    p.add_argument('--parent-tree', default=None, help='a built checkout of the parent commit, for --bench-py')
    p.add_argument('--only-bench-py', action='store_true', help='with --bands --bench-py: skip the decode legs')
    p.add_argument('--bank', action='store_true')
    p.add_argument('--bank-files', type=int, default=4096)
    p.add_argument('--alone', action='store_true')
    p.add_argument('--window', action='store_true')
    a = p.parse_args()
    if a.window:
        a.band_rows = [8, 16] if a.band_rows == [8, 16, 32] else a.band_rows
        return window_main(a)
    if a.alone:
        a.band_rows = [8, 16] if a.band_rows == [8, 16, 32] else a.band_rows
        return alone_main(a)
    if a.bank:
        a.band_rows = [16, 8] if a.band_rows == [8, 16, 32] else a.band_rows
        return bank_main(a)
    if a.bands:
        return bands_main(a)
    if not torch.cuda.is_available():
        raise SystemExit('png_decode_bench.py measures on a GPU; none is visible')
    lines, res = [], {}
    S = a.size
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    measure(a, lines, res, 'step', src, a.frames, (6, 1), 90, a.host_reps)
    if not a.no_large:
        big = torch.stack([torch.from_numpy(smooth_image(1080, 1920, 2000 + i)) for i in range(DISTINCT)])
        measure(a, lines, res, 'large', big, DISTINCT, (6,), 0, a.host_reps)
    line = json.dumps({'png_decode_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
