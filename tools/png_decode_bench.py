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
    a = p.parse_args()
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
