#!/usr/bin/env python3
"""Perturbations (DESIGN.md "Perturbations") on one GPU, one process per part: the call per kind, and the scorer.

    python tools/perturb_bench.py --only call   [--frames 256] [--size 224] [--out profiles/NAME.txt]
    python tools/perturb_bench.py --only videos [--set-size 64] [--video-frames 32]

call     ops.perturb_u8 on --frames device-resident frames of --size x --size, one kind at a time (every frame of that kind;
         device tables, checked=True), events around the call (three launches), against a device-to-device copy of the same
         bytes (3 per pixel read, 3 written) and against ops.jpeg_roundtrip_u8 at q = 75 ('420') on the same frames; the three
         legs alternate within a repeat, medians and min-max over the repeats after the warm-up.  Integer operations are not
         counted as a rate: the figure next to the copy is algorithmic GB/s (bytes in + bytes out).
videos   score_videos on --set-size device-resident uint8 videos of --video-frames frames at stride 8: plain, with
         perturb=('blur', 2.0) and with perturb=('noise', 10.0); the three legs alternate, host clock around the call (it
         synchronises); then one instrumented run per perturbation for the device time of its ops.perturb_u8 calls.
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
from istvt_amd import clips, ops, video  # noqa: E402
from istvt_amd.network.vivit.vivit import XceptionVidTr  # noqa: E402

# (label, kind name, value) of part `call`
CALL_CASES = [('copy', 'copy', None), ('brightness 0.8', 'brightness', 0.8), ('contrast 0.6', 'contrast', 0.6),
              ('saturation 0.4', 'saturation', 0.4), ('noise 10', 'noise', 10.0), ('blur 0.5', 'blur', 0.5),
              ('blur 2.0', 'blur', 2.0), ('blur 4.0', 'blur', 4.0), ('pixelate 4', 'pixelate', 4), ('pixelate 32', 'pixelate', 32)]
VIDEO_CASES = [('blur', 2.0), ('noise', 10.0)]


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


def fmt(s):
    return '%.3f ms (%.3f-%.3f)' % (s['median_ms'], s['min_ms'], s['max_ms'])


def say(lines, text):
    print(text, flush=True)
    lines.append(text)


def call_bench(a, lines):
    n, S = a.frames, a.size
    u8 = torch.randint(0, 256, (n, S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).cuda()
    out, dst, jout = torch.empty_like(u8), torch.empty_like(u8), torch.empty_like(u8)
    q75 = torch.full((n,), 75, dtype=torch.int32, device='cuda')
    nbytes = 2 * u8.numel()
    res = {}
    say(lines, 'perturb_u8: %d frames of %d x %d, %.1f MB in + out; per case the call, a device copy and jpeg_roundtrip_u8 q=75 '
        'alternate, %d repeats after %d warm-up: median (min-max)' % (n, S, S, nbytes * 1e-6, a.reps, a.warmup))
    for label, name, value in CALL_CASES:
        tab, taps = clips.perturbation_table(n, name, value)
        tab, taps = tab.cuda(), None if taps is None else taps.cuda()
        tk, tc, tj = [], [], []
        for r in range(a.warmup + a.reps):
            x = event_ms(lambda: ops.perturb_u8(u8, tab, taps, 1, out=out, checked=True))
            y = event_ms(lambda: dst.copy_(u8))
            z = event_ms(lambda: ops.jpeg_roundtrip_u8(u8, q75, out=jout, checked=True))
            if r >= a.warmup:
                tk.append(x), tc.append(y), tj.append(z)
        sk, sc, sj = stats(tk), stats(tc), stats(tj)
        res[label] = {'call': sk, 'copy': sc, 'jpeg_q75': sj, 'GB_per_s': nbytes / sk['median_ms'] * 1e-6,
                      'over_copy': sk['median_ms'] / sc['median_ms'], 'over_jpeg': sk['median_ms'] / sj['median_ms']}
        say(lines, '%-15s %s = %.0f GB/s, %.1f ps per pixel | copy %s | jpeg q=75 %s | call / copy x%.2f | call / jpeg x%.2f'
            % (label, fmt(sk), res[label]['GB_per_s'], sk['median_ms'] * 1e9 / (n * S * S), fmt(sc), fmt(sj),
               res[label]['over_copy'], res[label]['over_jpeg']))
    return res


def videos_bench(a, lines, model):
    g = torch.Generator().manual_seed(3)
    vids = [torch.randint(0, 256, (a.video_frames, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
            for _ in range(a.set_size)]
    scorers = [('plain', video.VideoScorer(model, stride=8))] + \
              [('%s %s' % P, video.VideoScorer(model, stride=8, perturb=P, perturb_seed=1)) for P in VIDEO_CASES]
    times = {name: [] for name, _ in scorers}
    for r in range(a.warmup + a.reps):
        for name, s in scorers:
            t = timed(lambda: s.score_videos(vids))
            if r >= a.warmup:
                times[name].append(t)
    res = {'videos': a.set_size, 'frames_per_video': a.video_frames}
    plain = stats(times['plain'])
    res['plain'] = plain
    say(lines, 'score_videos, %d videos of %d frames of %d x %d, stride 8, %d repeats after %d warm-up, legs alternating: plain %s'
        % (a.set_size, a.video_frames, a.size, a.size, a.reps, a.warmup, fmt(plain)))
    for name, s in scorers[1:]:
        st = stats(times[name])
        ops.kernel_profile = []
        try:
            s.score_videos(vids)
            torch.cuda.synchronize()
            kern = [e0.elapsed_time(e1) for what, e0, e1, _, _ in ops.kernel_profile if what == 'perturb_u8']
        finally:
            ops.kernel_profile = None
        added = st['median_ms'] - plain['median_ms']
        spread = max(plain['max_ms'] - plain['min_ms'], st['max_ms'] - st['min_ms'])
        res[name] = {'time': st, 'added_ms': added, 'added_share': added / plain['median_ms'], 'spread_ms': spread,
                     'perturb_device_ms': sum(kern), 'perturb_calls': len(kern)}
        say(lines, 'perturb=(%s): %s | difference to plain %.2f ms = %.2f %% (the wider of the two legs\' min-max spreads: %.2f ms%s) | '
            'ops.perturb_u8 in one instrumented run: %.3f ms on the device in %d calls = %.2f %% of the plain pass'
            % (name, fmt(st), added, 100 * added / plain['median_ms'], spread,
               ': the difference is inside it' if abs(added) < spread else '', sum(kern), len(kern),
               100 * sum(kern) / plain['median_ms']))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', required=True, choices=['call', 'videos'])
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--set-size', type=int, default=64)
    ap.add_argument('--video-frames', type=int, default=32)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('perturb_bench.py measures on a GPU; none is visible')
    lines = []
    if a.only == 'call':
        res = {'call': call_bench(a, lines)}
    else:
        from oracle import istvt_ref as R
        torch.manual_seed(0)
        model = XceptionVidTr(num_frames=8, grid=R.stem_out_side(a.size), depth=12, compute_dtype=torch.bfloat16).cuda().eval()
        res = {'videos': videos_bench(a, lines, model)}
    line = json.dumps({'perturb_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
