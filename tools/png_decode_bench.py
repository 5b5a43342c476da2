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
"""
import argparse
import io
import json
import os
import statistics
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


def kernel_shares(call, reps=10):
    """device time per kernel of `reps` calls -> {kernel name fragment: mean us per call}; a trace without the two kernels is
    an error, not a gap in the table"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for frag in ('png_inflate_kernel', 'png_unfilter_kernel'):
            if frag in ev.key:
                total = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0)
                out[frag] = out.get(frag, 0.0) + total / reps
    if len(out) != 2:
        raise SystemExit('the profiler trace holds no png_inflate_kernel / png_unfilter_kernel: %r' % (out,))
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--frames', type=int, default=256)
    p.add_argument('--size', type=int, default=224)
    p.add_argument('--reps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--host-reps', type=int, default=3)
    p.add_argument('--no-large', action='store_true')
    p.add_argument('--out', default=None)
    a = p.parse_args()
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
