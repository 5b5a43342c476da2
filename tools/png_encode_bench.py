#!/usr/bin/env python
"""PNG files out (DESIGN.md "PNG files out") on one GPU in one process: ops.png_encode_u8 on one training step's frames.

    python tools/png_encode_bench.py [--frames 256] [--size 224] [--out profiles/png_encode_bench.txt]

The frames are tools/png_decode_bench.py's (8 distinct ones, repeated), resident on the device.  Medians of --reps calls after
--warmup, with the fastest and the slowest:

device   ops.png_encode_u8 with the caller's buffers, events around the call (four launches), at band_rows 8, 16 and 32; each
         kernel's share from a torch.profiler trace of ten more calls; the files are decoded by PIL and compared with the
         source pixels first
host     what a user does without it: the pixels come down (3 bytes per pixel) and PIL saves every frame, at compress level 6
         and at level 1
bytes    the files against PIL's at both levels, on these frames and on the same pattern without its noise
decode   ops.png_decode_u8 on the device's files against PIL's level-6 files of the same frames
large    one batch of 8 frames of 1080 x 1920: the device call at band_rows 16 and the host route at level 6
"""
import argparse
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import clips, frames as F, ops  # noqa: E402
from jpeg_decode_bench import DISTINCT, event_ms, say, smooth_image, stats, timed  # noqa: E402
from png_decode_bench import fmt, png_file  # noqa: E402

KERNELS = ('png_filter_count_kernel', 'png_prefix_kernel', 'png_store_kernel', 'png_container_kernel')


def kernel_shares(call, reps=10):
    """device time per kernel of `reps` calls -> {kernel: mean us per call}; a trace without the four kernels is an error"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for frag in KERNELS:
            if frag in ev.key:
                total = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0)
                out[frag] = out.get(frag, 0.0) + total / reps
    if len(out) != len(KERNELS):
        raise SystemExit('the profiler trace does not hold the four kernels: %r' % (out,))
    return out


def noiseless_image(h, w):
    """jpeg_decode_bench.smooth_image without its Gaussian noise"""
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return np.clip(np.round(np.stack(planes, -1)), 0, 255).astype(np.uint8)


def encoder(dev_frames, R):
    n, H, W, c = dev_frames.shape
    cap = n * clips.png_encoded_bound(H, W, c, R)
    need = F.png_encode_scratch(n, H, W, c, R)[1]
    dev = dev_frames.device
    bufs = (torch.empty((cap,), dtype=torch.uint8, device=dev), torch.empty((need,), dtype=torch.uint8, device=dev),
            torch.empty((n + 1,), dtype=torch.int64, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
    return lambda: ops.png_encode_u8(dev_frames, R, 'adaptive', buffers=bufs)


def measure(a, lines, res, key, src, n, band_rows, levels, decode):
    dev = torch.device('cuda', torch.cuda.current_device())
    H, W = src.shape[1:3]
    pick = [i % DISTINCT for i in range(n)]
    dev_frames = src[torch.tensor(pick)].to(dev)
    calls = {R: encoder(dev_frames, R) for R in band_rows}
    files = {}
    for R, fn in calls.items():
        files[R] = fn().files()
        for i in range(DISTINCT):
            if not np.array_equal(np.asarray(Image.open(io.BytesIO(files[R][i]))), src[i].numpy()):
                raise SystemExit('%s band_rows %d: PIL does not read the source pixels from file %d' % (key, R, i))
    ts = {R: [] for R in calls}
    for r in range(a.warmup + a.reps):
        for R, fn in calls.items():
            t = event_ms(fn)
            if r >= a.warmup:
                ts[R].append(t)
    staging = torch.empty((n, H, W, 3), dtype=torch.uint8).pin_memory()

    def host_route(lv):
        staging.copy_(dev_frames, non_blocking=True)
        torch.cuda.synchronize()
        view = staging.numpy()
        return [png_file(view[j], lv) for j in range(n)]
    th = {lv: [] for lv in levels}
    for r in range(1 + a.host_reps):
        for lv in levels:
            x = timed(lambda: host_route(lv))
            if r >= 1:
                th[lv].append(x)
    pil = {lv: [png_file(src[i].numpy(), lv) for i in range(DISTINCT)] for lv in levels}
    pil_bytes = {lv: sum(len(pil[lv][i]) for i in pick) for lv in levels}
    res[key] = {'frames': n, 'H': H, 'W': W, 'pixel_bytes': n * H * W * 3, 'pil_bytes': pil_bytes,
                'host_route': {lv: stats(th[lv]) for lv in levels}}
    say(lines, '%s: %d frames of %d x %d, %.2f MB of pixels' % (key, n, H, W, n * H * W * 3e-6))
    for lv in levels:
        say(lines, '  host route, download + PIL save at compress level %d: %s, %.2f MB of files' % (lv, fmt(stats(th[lv])), pil_bytes[lv] * 1e-6))
    for R in band_rows:
        sd, nb = stats(ts[R]), sum(len(f) for f in files[R])
        shares = kernel_shares(calls[R])
        res[key]['band_rows_%d' % R] = {'device': sd, 'bytes': nb, 'kernel_us': shares,
                                        'ratio_to_pil': {lv: nb / pil_bytes[lv] for lv in levels}}
        say(lines, '  png_encode_u8, band_rows %d: %s on the device = %.2f us per frame, %.2f ns per pixel (%s) | %.2f MB of files = %s '
            'of PIL | the host route is %s x the device call'
            % (R, fmt(sd), sd['median_ms'] * 1e3 / n, sd['median_ms'] * 1e6 / (n * H * W),
               ', '.join('%s %.0f us' % (k[4:-7], shares[k]) for k in KERNELS), nb * 1e-6,
               ', '.join('%.3f at level %d' % (nb / pil_bytes[lv], lv) for lv in levels),
               ', '.join('%.1f (level %d)' % (stats(th[lv])['median_ms'] / sd['median_ms'], lv) for lv in levels)))
    if decode:
        R = 16 if 16 in files else band_rows[0]
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        legs = {'ours': clips.png_batch(files[R]), 'pil_l6': clips.png_batch([pil[6][i] for i in pick])}
        td = {}
        for k, b in legs.items():
            b.on(dev)
            bufs = (torch.empty((b.scratch_bytes,), dtype=torch.uint8, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                    torch.empty((n,), dtype=torch.int32, device=dev))
            fn = (lambda b=b, bufs=bufs: ops.png_decode_u8(b, out=out, checked=True, buffers=bufs))
            got, _, status = fn()
            clips.check_png_status(status)
            if not torch.equal(got, dev_frames):
                raise SystemExit('%s: png_decode_u8 does not give the source pixels from the %s files' % (key, k))
            td[k] = stats([event_ms(fn) for _ in range(a.warmup + a.reps)][a.warmup:])
        res[key]['decode'] = td
        say(lines, '  png_decode_u8 on the device\'s files (band_rows %d): %s; on PIL\'s level-6 files of the same frames: %s'
            % (R, fmt(td['ours']), fmt(td['pil_l6'])))


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
        raise SystemExit('png_encode_bench.py measures on a GPU; none is visible')
    lines, res = [], {}
    S = a.size
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    measure(a, lines, res, 'step', src, a.frames, (8, 16, 32), (6, 1), True)
    # the same pattern without its noise: what having no match search costs
    clean = torch.stack([torch.from_numpy(noiseless_image(S, S)) for _ in range(1)])
    ours = sum(len(f) for f in ops.png_encode_u8(clean.cuda()).files())
    pil6 = sum(len(png_file(clean[i].numpy(), 6)) for i in range(clean.shape[0]))
    res['noiseless'] = {'bytes': ours, 'pil_l6_bytes': pil6, 'ratio': ours / pil6}
    say(lines, 'noiseless: the pattern without its noise, one frame: %d bytes against PIL level 6 %d = %.3f' % (ours, pil6, ours / pil6))
    if not a.no_large:
        big = torch.stack([torch.from_numpy(smooth_image(1080, 1920, 2000 + i)) for i in range(DISTINCT)])
        measure(a, lines, res, 'large', big, DISTINCT, (16,), (6,), False)
    line = json.dumps({'png_encode_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
