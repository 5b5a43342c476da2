#!/usr/bin/env python3
"""JPEG round trip (DESIGN.md "JPEG round trip") on one GPU in one process: the kernel, the scorer and the training step.

    python tools/jpeg_bench.py [--frames 256] [--size 224] [--out profiles/NAME.txt]
    python tools/jpeg_bench.py --only kernel            # one part: kernel | videos | train

kernel   ops.jpeg_roundtrip_u8 on --frames device-resident frames of --size x --size, q = 30, 75 and 95, '420' and '444',
         events around the call (two launches), against a device-to-device copy of the same bytes (3 per pixel read, 3
         written); alternating, medians and min-max over the repeats after the warm-up.  Integer operations are not counted
         as a rate: the figure next to the copy is algorithmic GB/s.
videos   score_videos on --set-size device-resident uint8 videos of --video-frames frames at stride 8, with and without
         jpeg_quality=50; alternating, host clock around the call (it synchronises).
train    the training step from resident bytes (B = 32, T = 8, depth 12, bf16, fused SGD): model(u8, view=flips) against
         model(ops.jpeg_roundtrip_u8(u8, q), view=flips) with q = clips.random_qualities(B) uploaded beforehand; alternating
         legs of --steps steps, host clock around a leg, medians over --repeats rounds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import clips, ops, parallel, video  # noqa: E402
from istvt_amd.network.vivit.vivit import XceptionVidTr  # noqa: E402


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


def kernel_bench(a, lines):
    n, S = a.frames, a.size
    u8 = torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).cuda()
    out, dst = torch.empty_like(u8), torch.empty_like(u8)
    nbytes = 2 * u8.numel()
    res = {}
    for sub in ('420', '444'):
        for q in (30, 75, 95):
            qdev = torch.full((n,), q, dtype=torch.int32, device='cuda')
            tk, tc = [], []
            for r in range(a.warmup + a.reps):
                x = event_ms(lambda: ops.jpeg_roundtrip_u8(u8, qdev, sub, out=out, checked=True))
                y = event_ms(lambda: dst.copy_(u8))
                if r >= a.warmup:
                    tk.append(x)
                    tc.append(y)
            sk, sc = stats(tk), stats(tc)
            res['%s_q%d' % (sub, q)] = {'kernel': sk, 'copy': sc, 'kernel_GB_per_s': nbytes / sk['median_ms'] * 1e-6,
                                        'copy_GB_per_s': nbytes / sc['median_ms'] * 1e-6,
                                        'kernel_over_copy': sk['median_ms'] / sc['median_ms']}
            say(lines, 'jpeg_roundtrip_u8 %s q=%d: %d frames of %d x %d, %.1f MB in + out | %.3f ms (%.3f-%.3f) = %.0f GB/s, %.2f ns '
                'per pixel | device copy %.3f ms (%.3f-%.3f) = %.0f GB/s | kernel / copy x%.1f'
                % (sub, q, n, S, S, nbytes * 1e-6, sk['median_ms'], sk['min_ms'], sk['max_ms'], res['%s_q%d' % (sub, q)]['kernel_GB_per_s'],
                   sk['median_ms'] * 1e6 / (n * S * S), sc['median_ms'], sc['min_ms'], sc['max_ms'],
                   res['%s_q%d' % (sub, q)]['copy_GB_per_s'], sk['median_ms'] / sc['median_ms']))
    # the two launches apart (ops.prof times the pair; here each kernel of one call through its own quality: a table of
    # zeros runs the second kernel alone, as a copy)
    zeros = torch.zeros((n,), dtype=torch.int32, device='cuda')
    tz = [event_ms(lambda: ops.jpeg_roundtrip_u8(u8, zeros, '420', out=out, checked=True)) for _ in range(a.warmup + a.reps)][a.warmup:]
    res['passthrough'] = stats(tz)
    say(lines, 'jpeg_roundtrip_u8 with every quality 0 (first kernel returns at once, second copies): %.3f ms (%.3f-%.3f)'
        % (res['passthrough']['median_ms'], res['passthrough']['min_ms'], res['passthrough']['max_ms']))
    return res


def videos_bench(a, lines, model):
    g = torch.Generator().manual_seed(3)
    vids = [torch.randint(0, 256, (a.video_frames, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
            for _ in range(a.set_size)]
    plain = video.VideoScorer(model, stride=8)
    jpeg = video.VideoScorer(model, stride=8, jpeg_quality=50)
    ta, tb = [], []
    for r in range(a.warmup + a.reps):
        x, y = timed(lambda: plain.score_videos(vids)), timed(lambda: jpeg.score_videos(vids))
        if r >= a.warmup:
            ta.append(x)
            tb.append(y)
    sa, sb = stats(ta), stats(tb)
    ops.kernel_profile = []
    try:
        jpeg.score_videos(vids)
        torch.cuda.synchronize()
        kern = [e0.elapsed_time(e1) for name, e0, e1, _, _ in ops.kernel_profile if name == 'jpeg_roundtrip_u8']
    finally:
        ops.kernel_profile = None
    res = {'videos': a.set_size, 'frames_per_video': a.video_frames, 'plain': sa, 'jpeg_quality_50': sb,
           'added_ms': sb['median_ms'] - sa['median_ms'], 'added_share': (sb['median_ms'] - sa['median_ms']) / sa['median_ms'],
           'jpeg_device_ms': sum(kern), 'jpeg_calls': len(kern)}
    say(lines, 'score_videos, %d videos of %d frames, stride 8: plain %.2f ms (%.2f-%.2f) | jpeg_quality=50 %.2f ms (%.2f-%.2f) | '
        'difference %.2f ms = %.2f %% | the round trip in one instrumented run: %.3f ms on the device in %d calls'
        % (a.set_size, a.video_frames, sa['median_ms'], sa['min_ms'], sa['max_ms'], sb['median_ms'], sb['min_ms'], sb['max_ms'],
           res['added_ms'], 100 * res['added_share'], res['jpeg_device_ms'], res['jpeg_calls']))
    return res


def train_bench(a, lines):
    dev = torch.device('cuda', 0)
    B, T, S = 32, 8, a.size
    h = ((S - 3) // 2 + 1) - 2
    for _ in range(3):
        h = (h - 1) // 2 + 1
    torch.manual_seed(0)
    model = XceptionVidTr(num_frames=T, grid=h, depth=12, compute_dtype=torch.bfloat16).to(dev).train()
    model.set_crop_side(S)
    live = [p for _, p in parallel.live_named_parameters(model)]
    bucket = parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
    opt = parallel.FusedSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=0, zero_grad=True)
    crit = torch.nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(1)
    x = [torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(2)]
    y = [(torch.rand((B,), generator=g) > 0.5).float().to(dev) for _ in range(2)]
    flips = [clips.random_views(B, S, S, S, g).pin_memory() for _ in range(2)]      # host tables, as the loader hands them
    quals = [clips.random_qualities(B, generator=g) for _ in range(2)]
    qdev = [q.repeat_interleave(T).to(dev) for q in quals]

    def leg(jpeg, n):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(n):
            u8 = x[i % 2]
            if jpeg:
                u8 = ops.jpeg_roundtrip_u8(u8, qdev[i % 2], checked=True)
            opt.zero_grad()
            loss = crit(model(u8, view=flips[i % 2]).view(-1), y[i % 2])
            loss.backward()
            opt.step()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e3

    for jpeg in (False, True):
        leg(jpeg, a.warmup)
    times = {'bytes': [], 'bytes_jpeg': []}
    for r in range(a.repeats):
        times['bytes'].append(leg(False, a.steps))
        times['bytes_jpeg'].append(leg(True, a.steps))
        say(lines, 'train round %d: bytes %.3f ms / step | jpeg + bytes %.3f ms / step' % (r, times['bytes'][-1], times['bytes_jpeg'][-1]))
    ma, mb = statistics.median(times['bytes']), statistics.median(times['bytes_jpeg'])
    res = {'batch': B, 'frames': T, 'size': S, 'steps': a.steps, 'repeats': a.repeats, 'ms_per_step': times,
           'median_bytes': ma, 'median_bytes_jpeg': mb, 'added_ms': mb - ma, 'added_share': (mb - ma) / ma,
           'compressed_clips': [int((q > 0).sum()) for q in quals]}
    say(lines, 'training step from bytes, B=%d T=%d %d x %d depth 12 bf16: %.3f ms (%.3f-%.3f) | with the round trip in front (%s of '
        '%d clips compressed) %.3f ms (%.3f-%.3f) | added %.3f ms = %.2f %%'
        % (B, T, S, S, ma, min(times['bytes']), max(times['bytes']), res['compressed_clips'], B, mb, min(times['bytes_jpeg']),
           max(times['bytes_jpeg']), mb - ma, 100 * (mb - ma) / ma))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--set-size', type=int, default=64)
    ap.add_argument('--video-frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default=None, choices=['kernel', 'videos', 'train'])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_bench.py measures on a GPU; none is visible')
    lines, res = [], {}
    if a.only in (None, 'kernel'):
        res['kernel'] = kernel_bench(a, lines)
    if a.only in (None, 'videos'):
        from oracle import istvt_ref as R
        torch.manual_seed(0)
        model = XceptionVidTr(num_frames=8, grid=R.stem_out_side(a.size), depth=12, compute_dtype=torch.bfloat16).cuda().eval()
        res['videos'] = videos_bench(a, lines, model)
        del model
    if a.only in (None, 'train'):
        res['train'] = train_bench(a, lines)
    line = json.dumps({'jpeg_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
