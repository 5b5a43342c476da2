#!/usr/bin/env python3
"""Video scoring (DESIGN.md "Video scoring") against the clip path it replaces, on one GPU in one process.

    python tools/video_bench.py [--frames 256] [--size 224] [--T 8] [--depth 12] [--strides 1,2,4,8] [--json out.json]
    python tools/video_bench.py --conv1-only        # the two conv1 kernels alone, for a kernel trace
    python tools/video_bench.py --explain           # VideoScorer.explain against model.relevance on materialised windows
    python tools/video_bench.py --boxes             # whole 1080 x 1920 frames and face boxes (DESIGN.md "Frames and boxes")

    python tools/video_bench.py --nv12              # NV12 frames: the fused crop against convert + crop (DESIGN.md "NV12 frames")
    python tools/video_bench.py --videos            # a set of 64 videos of 32 frames (DESIGN.md "Scoring a set of videos")
    python tools/video_bench.py --align             # one similarity per frame: the warp against the crop (DESIGN.md "Aligned crops")
    python tools/video_bench.py --paste             # maps pasted back onto whole frames (DESIGN.md "Pasting maps onto frames")

(a) VideoScorer.score on a device-resident uint8 video; (b) the same windows gathered on the device from the normalised
float32 video into clips and run through model(clips) in eval mode under no_grad, window_batch clips at a time -- the
code path that exists without the scorer (its host-side normalisation and 4x larger upload are NOT charged to it).
Each repeat times (a) then (b), the device synchronised on both sides of each; the figures are medians over the repeats
after the warm-up, with the min-max spread of both.  The split of (a) into stem / token assembly / transformer comes from
ops.prof events in one further, instrumented run.

--explain (DESIGN.md "Explaining whole videos"), strides 1 and 8 unless --strides says otherwise: (a) VideoScorer.explain
on the device-resident uint8 video; (b) the loop a user writes without it: model.relevance on the windows gathered from the
normalised float32 video, window_batch at a time (normalisation and upload again not charged; the fusion over windows,
which that user would still have to write, is not part of (b) either).  Alternating, medians as above.  One further,
instrumented explain() and one explain.overlay() of the whole video give the device time of the fuse and overlay kernels
(events around the launches) and the overlay's rate against its algorithmic bytes.

--boxes (DESIGN.md "Frames and boxes"): --frames whole frames of --full-size on the device, one random box of side
--box-sides per frame.  Alternating, medians and spread as above: (a) score(frames, boxes=...); (b) score on the crops the
same kernel made beforehand -- (a) - (b) is what the crop costs inside a call; (c) the host loop it replaces,
clips.crop_resize_host on host frames + upload of the crops, twice on its own (it takes seconds: this project's plain
torch restatement of the definition, not a tuned image library); (d) the kernel alone on all frames (events around the launch)
against (e) a device-to-device copy that moves the same algorithmic bytes (box areas * 3 in, S * S * 3 out per frame: a
copy of half their sum reads and writes that many).

--nv12 (DESIGN.md "NV12 frames"), stride 8 unless --strides says otherwise: --frames NV12 frames of --full-size on the
device, made once with clips.rgb_to_nv12_host, one random box of side --box-sides per frame.  Events around the launches,
the legs of a comparison alternating, median and range of --reps: (a) ops.crop_resize_nv12 against (b) ops.nv12_to_rgb_u8
followed by ops.crop_resize_u8; each of those two kernels on its own; then score(nv12, boxes) on an NV12 scorer against
score(rgb, boxes) on the frames (b) converted beforehand.

--align (DESIGN.md "Aligned crops"), stride 8 unless --strides says otherwise: --frames frames of --full-size on the device,
as packed RGB and as NV12, one random similarity per frame (source side --box-sides, within --degrees, half of them
mirrored, the rotated square inside the frame).  Events around the launches, the legs alternating, median and range of
--reps: ops.warp_similarity_u8, ops.warp_similarity_nv12, and the yardstick, ops.crop_resize_u8 on the square boxes of the
same centres and sides; then score(frames, transforms=...) against score on the warps made beforehand.

--paste (DESIGN.md "Pasting maps onto frames"): --frames frames of --full-size on the device, as packed RGB and as NV12 (random
bytes), one random similarity per frame as --align draws them, one random 14 x 14 map per frame (--size / 16 cells a side).
Events around the launches, the legs alternating, median and range of --reps, per format: a plain device copy of the frames
(the yardstick of the out-of-place form), the paste out of place, the paste in place, and for scale on packed RGB
ops.warp_similarity_u8 followed by explain.overlay on the crops.  The in-place leg is also given as GB/s over the bytes it
moves: every rectangle read once and every region written once.  No model is built.

--videos (DESIGN.md "Scoring a set of videos"), strides 8 and 1 unless --strides says otherwise: --set-size device-resident
uint8 videos of --video-frames frames.  Alternating, medians and spread as above: (a) score_videos(videos, labels=...);
(b) the loop that exists without it, score(video) for every video.  One further, instrumented run of each gives the device
time of the phases (stem, token assembly, transformer) and of the two new kernels (ops.prof events); the plan's full and
partial window batches are reported with them.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import _lib, ops, video  # noqa: E402
from istvt_amd.network.vivit.vivit import XceptionVidTr  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3              # ms


def stats(ts):
    s = sorted(ts)
    return {'median_ms': s[len(s) // 2], 'min_ms': s[0], 'max_ms': s[-1]}


def conv1_only(a):
    """both conv1 kernels on the same frames, `reps` launches each (run under a kernel trace)"""
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (a.frames, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
    mean, std = torch.tensor(video.DEFAULT_MEAN).cuda(), torch.tensor(video.DEFAULT_STD).cuda()
    x = (((u8.float() / 255) - mean) / std).permute(0, 3, 1, 2).contiguous()
    w = torch.randn((32, 3, 3, 3), generator=g).cuda()
    Ho = (a.size - 3) // 2 + 1
    ref = torch.empty((a.frames * Ho * Ho, 32), dtype=torch.bfloat16, device='cuda')
    for _ in range(a.reps + a.warmup):
        out = ops.conv1_fwd_u8(u8, mean, std, w, torch.bfloat16)
        _lib.check(_lib.lib().istvt_conv1_fwd(x.data_ptr(), w.data_ptr(), ref.data_ptr(), a.frames, a.size, 1, ops._stream()),
                   'istvt_conv1_fwd')
    torch.cuda.synchronize()
    # (x was normalised on the device here, where torch divides by multiplying with a reciprocal: close, not equal bits)
    print('conv1_only: %d launches each, max abs diff %.3e' % (a.reps + a.warmup, float((out.float() - ref.float()).abs().max())))


def explain_bench(a, model, u8, xn):
    from istvt_amd import explain
    out = {}
    for stride in [int(s) for s in a.strides.split(',')]:
        scorer = video.VideoScorer(model, stride=stride, frame_batch=a.frame_batch, window_batch=a.window_batch)
        starts = video.window_starts(a.frames, a.T, stride, True)
        W = len(starts)
        tab = (torch.tensor(starts).view(-1, 1) + torch.arange(a.T).view(1, -1)).cuda()
        res = {}

        def run_explain():
            res['a'] = scorer.explain(u8)

        def run_loop():
            res['b'] = [model.relevance(xn[tab[i:i + a.window_batch]]) for i in range(0, W, a.window_batch)]
        ta, tb = [], []
        for r in range(a.warmup + a.reps):
            x, y = timed(run_explain), timed(run_loop)
            if r >= a.warmup:
                ta.append(x)
                tb.append(y)
        cam = torch.cat([r.cam_s for r in res['b']]).double()
        diff = float((res['a'].windows.cam_s.double() - cam).norm() / cam.norm())
        ops.kernel_profile = []
        try:
            run_explain()
            shown = explain.overlay(u8, res['a'].frame_s)
            torch.cuda.synchronize()
            kern = {}
            for name, e0, e1, nbytes, flops in ops.kernel_profile:
                if name in ('relevance_fuse_windows', 'relevance_overlay_u8'):
                    d = kern.setdefault(name, {'ms': 0.0, 'bytes': 0})
                    d['ms'] += e0.elapsed_time(e1)
                    d['bytes'] += nbytes
        finally:
            ops.kernel_profile = None
        sa, sb = stats(ta), stats(tb)
        for d in kern.values():
            d['GB_per_s'] = d['bytes'] / d['ms'] * 1e-6
            d['share_of_explain'] = d['ms'] / sa['median_ms']
        rec = {'windows': W, 'explain': sa, 'relevance_loop': sb, 'loop_over_explain': sb['median_ms'] / sa['median_ms'],
               'explain_spread': (sa['max_ms'] - sa['min_ms']) / sa['median_ms'],
               'loop_spread': (sb['max_ms'] - sb['min_ms']) / sb['median_ms'], 'cam_s_relerr': diff, 'kernels': kern,
               'overlay_shape': list(shown.shape)}
        out[str(stride)] = rec
        print('explain stride %d: %d windows | explain %.1f ms (%.1f-%.1f) | model.relevance loop %.1f ms (%.1f-%.1f) | loop / '
              'explain x%.3f | cam_s relerr %.2e' % (stride, W, sa['median_ms'], sa['min_ms'], sa['max_ms'], sb['median_ms'],
                                                    sb['min_ms'], sb['max_ms'], rec['loop_over_explain'], diff), flush=True)
        for k, d in kern.items():
            print('          %s: %.3f ms on the device, %.1f GB/s of %.1f MB algorithmic, %.3f %% of one explain()'
                  % (k, d['ms'], d['GB_per_s'], d['bytes'] * 1e-6, 100 * d['share_of_explain']), flush=True)
    return out


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def boxes_bench(a, model):
    from istvt_amd import clips
    Hs, Ws = (int(v) for v in a.full_size.split('x'))
    lo, hi = (int(v) for v in a.box_sides.split('-'))
    S, n = a.size, a.frames
    g = torch.Generator().manual_seed(2)
    host = torch.randint(0, 256, (n, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    h = torch.randint(lo, hi + 1, (n,), generator=g)
    w = torch.randint(lo, hi + 1, (n,), generator=g)
    y0 = torch.minimum((torch.rand(n, generator=g) * (Hs - h + 1)).long(), Hs - h)
    x0 = torch.minimum((torch.rand(n, generator=g) * (Ws - w + 1)).long(), Ws - w)
    boxes = torch.stack([y0, x0, h, w], dim=1).to(torch.int32)
    frames = host.cuda()
    bdev = boxes.cuda()
    crops = ops.crop_resize_u8(frames, boxes, S)
    bytes_in, bytes_out = int((h * w).sum()) * 3, n * S * S * 3
    half = (bytes_in + bytes_out) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device='cuda'), torch.empty(half, dtype=torch.uint8, device='cuda')
    out = {'frames': n, 'full_size': [Hs, Ws], 'box_sides': [lo, hi], 'size': S, 'bytes_in': bytes_in, 'bytes_out': bytes_out,
           'strides': {}}
    tk, tc = [], []
    for r in range(a.warmup + a.reps):
        x = event_ms(lambda: ops.crop_resize_u8(frames, bdev, S, out=crops, checked=True))
        y = event_ms(lambda: dst.copy_(src))
        if r >= a.warmup:
            tk.append(x)
            tc.append(y)
    sk, sc = stats(tk), stats(tc)
    out['kernel'] = dict(sk, GB_per_s=(bytes_in + bytes_out) / sk['median_ms'] * 1e-6)
    out['copy'] = dict(sc, GB_per_s=(bytes_in + bytes_out) / sc['median_ms'] * 1e-6)
    print('crop_resize_u8: %d frames, %.1f MB in + %.1f MB out | kernel %.3f ms (%.3f-%.3f) = %.0f GB/s | device copy of the '
          'same bytes %.3f ms (%.3f-%.3f) = %.0f GB/s | kernel / copy x%.2f'
          % (n, bytes_in * 1e-6, bytes_out * 1e-6, sk['median_ms'], sk['min_ms'], sk['max_ms'], out['kernel']['GB_per_s'],
             sc['median_ms'], sc['min_ms'], sc['max_ms'], out['copy']['GB_per_s'], sk['median_ms'] / sc['median_ms']), flush=True)
    for stride in [int(s) for s in a.strides.split(',')]:
        scorer = video.VideoScorer(model, stride=stride, frame_batch=a.frame_batch, window_batch=a.window_batch, side=S)
        res = {}

        def run_boxed():
            res['a'] = scorer.score(frames, boxes=boxes).window_logits

        def run_crops():
            res['b'] = scorer.score(crops).window_logits
        ta, tb = [], []
        for r in range(a.warmup + a.reps):
            x, y = timed(run_boxed), timed(run_crops)
            if r >= a.warmup:
                ta.append(x)
                tb.append(y)
        sa, sb = stats(ta), stats(tb)
        rec = {'boxed': sa, 'crops': sb, 'equal_bits': bool(torch.equal(res['a'], res['b'])),
               'crop_cost_ms': sa['median_ms'] - sb['median_ms'],
               'crop_cost_share': (sa['median_ms'] - sb['median_ms']) / sb['median_ms']}
        out['strides'][str(stride)] = rec
        print('boxes stride %d: score(frames, boxes) %.2f ms (%.2f-%.2f) | score(crops) %.2f ms (%.2f-%.2f) | difference %.2f ms = '
              '%.2f %% | equal bits %s' % (stride, sa['median_ms'], sa['min_ms'], sa['max_ms'], sb['median_ms'], sb['min_ms'],
                                          sb['max_ms'], rec['crop_cost_ms'], 100 * rec['crop_cost_share'], rec['equal_bits']),
              flush=True)
    res = {}

    def run_host():
        res['c'] = clips.crop_resize_host(host, boxes, S).pin_memory().cuda()
    clips.crop_resize_host(host[:4], boxes[:4], S)
    th = [timed(run_host) for _ in range(2)]
    differ = int((res['c'] != crops).sum())
    out['host_loop'] = {'ms': th, 'bytes_differing_from_the_kernel': differ, 'of': crops.numel(),
                        'max_abs_byte_diff': int((res['c'].int() - crops.int()).abs().max())}
    print('host loop (crop_resize_host + upload): %.0f and %.0f ms | %d of %d bytes differ from the kernel, by at most %d'
          % (th[0], th[1], differ, crops.numel(), out['host_loop']['max_abs_byte_diff']), flush=True)
    return out


def paste_bench(a):
    import math
    from istvt_amd import clips, explain
    Hs, Ws = (int(v) for v in a.full_size.split('x'))
    lo, hi = (int(v) for v in a.box_sides.split('-'))
    S, n = a.size, a.frames
    gc = max(1, min(19, S // 16))
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (n, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda()
    nv = torch.randint(0, 256, (n, Hs + Hs // 2, Ws), generator=g, dtype=torch.uint8).cuda()
    side = torch.randint(lo, hi + 1, (n,), generator=g).double()
    u = torch.rand((4, n), generator=g, dtype=torch.float64)
    ang = (2 * u[0] - 1) * math.radians(a.degrees)
    half = 0.5 * side * (torch.cos(ang).abs() + torch.sin(ang).abs())
    cx, cy = half + u[1] * (Ws - 2 * half), half + u[2] * (Hs - 2 * half)
    M = clips.similarities_of_squares(side, ang, cx, cy, u[3] < 0.5, S)
    maps = torch.randn((n, gc, gc), generator=g).cuda()
    lut = explain.jet_lut()
    alpha = torch.full((n,), 0.5, dtype=torch.float32, device='cuda')
    out = {'frames': n, 'full_size': [Hs, Ws], 'box_sides': [lo, hi], 'degrees': a.degrees, 'size': S, 'grid': gc}
    crops = ops.warp_similarity_u8(frames, M, S)
    mdev = M.cuda()
    for fmt, src, bpp in (('rgb24', frames, 3.0), ('nv12', nv, 1.5)):
        A, rect = clips.paste_geometry(n, Hs, Ws, S, transforms=M, even=fmt == 'nv12')
        paste = ops.relevance_paste_nv12 if fmt == 'nv12' else ops.relevance_paste_u8
        table = (clips.lut_to_ycc(lut, a.matrix) if fmt == 'nv12' else lut).cuda()
        Ad, rd = A.cuda(), rect.cuda()
        dst, work = torch.empty_like(src), src.clone()
        legs = {'copy': lambda: dst.copy_(src),
                'paste_out_of_place': lambda: paste(src, maps, Ad, rd, table, alpha, S, out=dst, checked=True),
                'paste_in_place': lambda: paste(work, maps, Ad, rd, table, alpha, S, inplace=True, checked=True)}
        if fmt == 'rgb24':
            legs['warp_then_overlay_on_crops'] = lambda: explain.overlay(
                ops.warp_similarity_u8(frames, mdev, S, out=crops, checked=True), maps, scale=16, lut=table)
        ts = {k: [] for k in legs}
        for r in range(a.warmup + a.reps):
            for k, fn in legs.items():                      # alternating
                t = event_ms(fn)
                if r >= a.warmup:
                    ts[k].append(t)
        res = {k: stats(ts[k]) for k in legs}
        moved = bpp * (float((rect[:, 2].double() * rect[:, 3].double()).sum()) + float((side * side).sum()))
        res['in_place_bytes'] = moved
        res['in_place_GB_per_s'] = moved / (res['paste_in_place']['median_ms'] * 1e-3) / 1e9
        res['frame_bytes'] = float(src.numel())
        res['in_place_over_copy'] = res['paste_in_place']['median_ms'] / res['copy']['median_ms']
        for k in legs:
            print('paste %-5s %-27s %.3f ms (%.3f-%.3f)' % (fmt, k, res[k]['median_ms'], res[k]['min_ms'], res[k]['max_ms']),
                  flush=True)
        print('paste %-5s in place moves %.1f MB of %.1f MB of frames: %.0f GB/s; in place / copy x%.3f'
              % (fmt, moved / 1e6, src.numel() / 1e6, res['in_place_GB_per_s'], res['in_place_over_copy']), flush=True)
        out[fmt] = res
    return out


def nv12_bench(a, model):
    from istvt_amd import clips
    Hs, Ws = (int(v) for v in a.full_size.split('x'))
    lo, hi = (int(v) for v in a.box_sides.split('-'))
    S, n = a.size, a.frames
    g = torch.Generator().manual_seed(2)
    nv = torch.empty((n, Hs + Hs // 2, Ws), dtype=torch.uint8, device='cuda')
    for i in range(0, n, 8):                                # the float64 encoder, a few frames at a time
        k = min(8, n - i)
        nv[i:i + k] = clips.rgb_to_nv12_host(torch.randint(0, 256, (k, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda(), a.matrix)
    h = torch.randint(lo, hi + 1, (n,), generator=g)
    w = torch.randint(lo, hi + 1, (n,), generator=g)
    y0 = torch.minimum((torch.rand(n, generator=g) * (Hs - h + 1)).long(), Hs - h)
    x0 = torch.minimum((torch.rand(n, generator=g) * (Ws - w + 1)).long(), Ws - w)
    boxes = torch.stack([y0, x0, h, w], dim=1).to(torch.int32)
    bdev = boxes.cuda()
    rgb = ops.nv12_to_rgb_u8(nv, a.matrix)
    crops = ops.crop_resize_u8(rgb, boxes, S)
    fused = ops.crop_resize_nv12(nv, boxes, S, a.matrix)
    area = int((h * w).sum())
    out = {'frames': n, 'full_size': [Hs, Ws], 'box_sides': [lo, hi], 'size': S, 'matrix': a.matrix, 'box_pixels': area,
           'equal_bits': bool(torch.equal(fused, crops)), 'strides': {}}
    legs = {'fused': lambda: ops.crop_resize_nv12(nv, bdev, S, a.matrix, out=fused, checked=True),
            'convert_then_crop': lambda: ops.crop_resize_u8(ops.nv12_to_rgb_u8(nv, a.matrix, out=rgb), bdev, S, out=crops, checked=True),
            'nv12_to_rgb_u8': lambda: ops.nv12_to_rgb_u8(nv, a.matrix, out=rgb),
            'crop_resize_u8': lambda: ops.crop_resize_u8(rgb, bdev, S, out=crops, checked=True)}
    ts = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():                          # alternating
            t = event_ms(fn)
            if r >= a.warmup:
                ts[k].append(t)
    # algorithmic bytes: the fused kernel reads 1.5 bytes per box pixel, the conversion 1.5 per frame pixel and writes 3
    nbytes = {'fused': area * 3 // 2 + n * S * S * 3, 'nv12_to_rgb_u8': n * Hs * Ws * 9 // 2, 'crop_resize_u8': area * 3 + n * S * S * 3}
    for k in legs:
        out[k] = stats(ts[k])
        if k in nbytes:
            out[k]['GB_per_s'] = nbytes[k] / out[k]['median_ms'] * 1e-6
        print('nv12 %-18s %.3f ms (%.3f-%.3f)%s' % (k, out[k]['median_ms'], out[k]['min_ms'], out[k]['max_ms'],
                                                     ' = %.0f GB/s of its algorithmic bytes' % out[k]['GB_per_s'] if k in nbytes else ''),
              flush=True)
    print('nv12: fused / (convert + crop) x%.3f | equal bits %s' % (out['fused']['median_ms'] / out['convert_then_crop']['median_ms'],
                                                                  out['equal_bits']), flush=True)
    for stride in [int(s) for s in a.strides.split(',')]:
        kw = dict(stride=stride, frame_batch=a.frame_batch, window_batch=a.window_batch, side=S)
        s_nv = video.VideoScorer(model, pixel_format='nv12', yuv_matrix=a.matrix, **kw)
        s_rgb = video.VideoScorer(model, **kw)
        res = {}

        def run_nv12():
            res['a'] = s_nv.score(nv, boxes=boxes).window_logits

        def run_rgb():
            res['b'] = s_rgb.score(rgb, boxes=boxes).window_logits
        ta, tb = [], []
        for r in range(a.warmup + a.reps):
            x, y = timed(run_nv12), timed(run_rgb)
            if r >= a.warmup:
                ta.append(x)
                tb.append(y)
        sa, sb = stats(ta), stats(tb)
        out['strides'][str(stride)] = {'nv12': sa, 'rgb': sb, 'equal_bits': bool(torch.equal(res['a'], res['b']))}
        print('nv12 stride %d: score(nv12, boxes) %.2f ms (%.2f-%.2f) | score(rgb, boxes) %.2f ms (%.2f-%.2f) | equal bits %s'
              % (stride, sa['median_ms'], sa['min_ms'], sa['max_ms'], sb['median_ms'], sb['min_ms'], sb['max_ms'],
                 out['strides'][str(stride)]['equal_bits']), flush=True)
    return out


def align_bench(a, model):
    import math
    from istvt_amd import clips
    Hs, Ws = (int(v) for v in a.full_size.split('x'))
    lo, hi = (int(v) for v in a.box_sides.split('-'))
    S, n = a.size, a.frames
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (n, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda()
    nv = torch.empty((n, Hs + Hs // 2, Ws), dtype=torch.uint8, device='cuda')
    for i in range(0, n, 8):
        nv[i:i + 8] = clips.rgb_to_nv12_host(frames[i:i + 8], a.matrix)
    side = torch.randint(lo, hi + 1, (n,), generator=g).double()
    u = torch.rand((4, n), generator=g, dtype=torch.float64)
    ang = (2 * u[0] - 1) * math.radians(a.degrees)
    cos, sin = torch.cos(ang), torch.sin(ang)
    half = 0.5 * side * (cos.abs() + sin.abs())
    cx, cy = half + u[1] * (Ws - 2 * half), half + u[2] * (Hs - 2 * half)
    M = clips.check_similarities(clips.similarities_of_squares(side, ang, cx, cy, u[3] < 0.5, S), n, Hs, Ws, S)
    # the yardstick's boxes: the same centres and sides, axis-aligned
    isd = side.long()
    y0 = (cy - 0.5 * side).round().long().clamp_(min=0)
    x0 = (cx - 0.5 * side).round().long().clamp_(min=0)
    boxes = torch.stack([torch.minimum(y0, Hs - isd), torch.minimum(x0, Ws - isd), isd, isd], dim=1).to(torch.int32)
    mdev, bdev = M.cuda(), boxes.cuda()
    warps = ops.warp_similarity_u8(frames, M, S)
    warps_nv = ops.warp_similarity_nv12(nv, M, S, a.matrix)
    crops = ops.crop_resize_u8(frames, boxes, S)
    out = {'frames': n, 'full_size': [Hs, Ws], 'box_sides': [lo, hi], 'degrees': a.degrees, 'size': S, 'matrix': a.matrix,
           'source_pixels': int((isd * isd).sum()), 'strides': {},
           'nv12_equals_rgb_path': bool(torch.equal(warps_nv, ops.warp_similarity_u8(ops.nv12_to_rgb_u8(nv, a.matrix), M, S)))}
    legs = {'warp_similarity_u8': lambda: ops.warp_similarity_u8(frames, mdev, S, out=warps, checked=True),
            'warp_similarity_nv12': lambda: ops.warp_similarity_nv12(nv, mdev, S, a.matrix, out=warps_nv, checked=True),
            'crop_resize_u8': lambda: ops.crop_resize_u8(frames, bdev, S, out=crops, checked=True)}
    ts = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():                          # alternating
            t = event_ms(fn)
            if r >= a.warmup:
                ts[k].append(t)
    for k in legs:
        out[k] = stats(ts[k])
        print('align %-22s %.3f ms (%.3f-%.3f)' % (k, out[k]['median_ms'], out[k]['min_ms'], out[k]['max_ms']), flush=True)
    out['warp_over_crop'] = out['warp_similarity_u8']['median_ms'] / out['crop_resize_u8']['median_ms']
    out['warp_nv12_over_crop'] = out['warp_similarity_nv12']['median_ms'] / out['crop_resize_u8']['median_ms']
    print('align: warp / crop x%.2f (RGB), x%.2f (NV12) on the same %d faces | NV12 equals the RGB path: %s'
          % (out['warp_over_crop'], out['warp_nv12_over_crop'], n, out['nv12_equals_rgb_path']), flush=True)
    for stride in [int(v) for v in a.strides.split(',')]:
        scorer = video.VideoScorer(model, stride=stride, frame_batch=a.frame_batch, window_batch=a.window_batch, side=S)
        res = {}

        def run_aligned():
            res['a'] = scorer.score(frames, transforms=M).window_logits

        def run_crops():
            res['b'] = scorer.score(warps).window_logits
        ta, tb = [], []
        for r in range(a.warmup + a.reps):
            x, y = timed(run_aligned), timed(run_crops)
            if r >= a.warmup:
                ta.append(x)
                tb.append(y)
        sa, sb = stats(ta), stats(tb)
        rec = {'aligned': sa, 'crops': sb, 'equal_bits': bool(torch.equal(res['a'], res['b'])),
               'warp_cost_ms': sa['median_ms'] - sb['median_ms'],
               'warp_cost_share': (sa['median_ms'] - sb['median_ms']) / sb['median_ms']}
        out['strides'][str(stride)] = rec
        print('align stride %d: score(frames, transforms) %.2f ms (%.2f-%.2f) | score(warps) %.2f ms (%.2f-%.2f) | difference '
              '%.2f ms = %.2f %% | equal bits %s' % (stride, sa['median_ms'], sa['min_ms'], sa['max_ms'], sb['median_ms'],
                                                    sb['min_ms'], sb['max_ms'], rec['warp_cost_ms'],
                                                    100 * rec['warp_cost_share'], rec['equal_bits']), flush=True)
    return out


def _phases(scorer, model, fn, extra=()):
    """one instrumented run of fn: device ms between the events around the three phases and the kernels named in `extra`"""
    ops.kernel_profile = []
    stem0, gather0, ft0 = scorer._stem, ops.tokens_gather_fwd, model.vit.forward_tokens

    def wrap(name, f0):
        def f(*p, **k):
            with ops.prof(name):
                return f0(*p, **k)
        return f
    try:
        scorer._stem = wrap('phase:stem', stem0)
        ops.tokens_gather_fwd = wrap('phase:tokens', gather0)
        model.vit.forward_tokens = wrap('phase:transformer', ft0)
        fn()
        torch.cuda.synchronize()
        split = {}
        for name, e0, e1, nbytes, flops in ops.kernel_profile:
            if name.startswith('phase:') or name in extra:
                d = split.setdefault(name.replace('phase:', ''), {'ms': 0.0, 'launches': 0})
                d['ms'] += e0.elapsed_time(e1)
                d['launches'] += 1
    finally:
        ops.kernel_profile = None
        scorer._stem, ops.tokens_gather_fwd = stem0, gather0
        del model.vit.forward_tokens                       # the instance attribute; the method is back
    return split


def videos_bench(a, model):
    g = torch.Generator().manual_seed(3)
    V, n = a.set_size, a.video_frames
    vids = [torch.randint(0, 256, (n, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(V)]
    labels = torch.randint(0, 2, (V,), generator=g)
    out = {}
    for stride in [int(s) for s in a.strides.split(',')]:
        scorer = video.VideoScorer(model, stride=stride, frame_batch=a.frame_batch, window_batch=a.window_batch)
        plan = video.SetPlan([n] * V, a.T, stride, True, a.frame_batch, a.window_batch)
        W = len(plan.starts)
        res = {}

        def run_set():
            res['a'] = scorer.score_videos(vids, labels=labels)

        def run_loop():
            res['b'] = [scorer.score(v) for v in vids]
        ta, tb = [], []
        for r in range(a.warmup + a.reps):
            x, y = timed(run_set), timed(run_loop)
            if r >= a.warmup:
                ta.append(x)
                tb.append(y)
        ref = torch.cat([r.window_logits for r in res['b']])
        diff = float((res['a'].window_logits - ref).abs().max())
        mdiff = float((res['a'].logit_mean - torch.stack([r.logit_mean for r in res['b']])).abs().max())
        split_a = _phases(scorer, model, run_set, ('windows_reduce', 'auc_pairs'))
        split_b = _phases(scorer, model, run_loop)
        sa, sb = stats(ta), stats(tb)
        m = res['a'].metrics
        rec = {'videos': V, 'frames_per_video': n, 'windows': W, 'score_videos': sa, 'score_loop': sb,
               'loop_over_set': sb['median_ms'] / sa['median_ms'], 'set_ms_per_32_windows': sa['median_ms'] * 32 / W,
               'loop_ms_per_32_windows': sb['median_ms'] * 32 / W, 'set_spread_ms': sa['max_ms'] - sa['min_ms'],
               'loop_spread_ms': sb['max_ms'] - sb['min_ms'], 'max_abs_logit_diff': diff, 'max_abs_logit_mean_diff': mdiff,
               'equal_bits': bool(torch.equal(res['a'].window_logits, ref)), 'full_window_batches': plan.full_batches,
               'partial_window_batches': plan.partial_batches, 'bank_slots': plan.slots_used, 'split_set_ms': split_a,
               'split_loop_ms': split_b, 'auc': float(m.auc), 'correct': int(m.correct)}
        out[str(stride)] = rec
        print('videos stride %d: %d videos, %d windows (%d full + %d partial batches, %d bank slots) | score_videos %.1f ms '
              '(%.1f-%.1f) = %.2f ms / 32 windows | loop of score %.1f ms (%.1f-%.1f) = %.2f ms / 32 windows | loop / set x%.3f | '
              'max |logit diff| %.2e, equal bits %s' % (stride, V, W, plan.full_batches, plan.partial_batches, plan.slots_used,
                                                       sa['median_ms'], sa['min_ms'], sa['max_ms'], rec['set_ms_per_32_windows'],
                                                       sb['median_ms'], sb['min_ms'], sb['max_ms'], rec['loop_ms_per_32_windows'],
                                                       rec['loop_over_set'], diff, rec['equal_bits']), flush=True)
        for what, split in (('score_videos', split_a), ('loop', split_b)):
            print('          %s, one instrumented run: ' % what +
                  ', '.join('%s %.3f ms in %d' % (k, v['ms'], v['launches']) for k, v in split.items()), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--T', type=int, default=8)
    ap.add_argument('--depth', type=int, default=12)
    ap.add_argument('--strides', default=None)
    ap.add_argument('--frame-batch', type=int, default=64)
    ap.add_argument('--window-batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--conv1-only', action='store_true')
    ap.add_argument('--explain', action='store_true')
    ap.add_argument('--boxes', action='store_true')
    ap.add_argument('--videos', action='store_true')
    ap.add_argument('--nv12', action='store_true')
    ap.add_argument('--align', action='store_true')
    ap.add_argument('--paste', action='store_true')
    ap.add_argument('--degrees', type=float, default=15.0)
    ap.add_argument('--matrix', default='bt709', choices=['bt601', 'bt709', 'jfif'])
    ap.add_argument('--set-size', type=int, default=64)
    ap.add_argument('--video-frames', type=int, default=32)
    ap.add_argument('--full-size', default='1080x1920')
    ap.add_argument('--box-sides', default='150-600')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    a.strides = a.strides or ('8' if a.nv12 or a.align else '8,1' if a.videos else '1,8' if a.explain or a.boxes else '1,2,4,8')
    if not torch.cuda.is_available():
        raise SystemExit('video_bench.py measures on a GPU; none is visible')
    if a.conv1_only:
        return conv1_only(a)
    if a.paste:
        out = dict(paste_bench(a), reps=a.reps, warmup=a.warmup)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(out, f, indent=1)
        print(json.dumps({'video_paste_bench': {f: {'copy_ms': out[f]['copy']['median_ms'],
                                                    'out_of_place_ms': out[f]['paste_out_of_place']['median_ms'],
                                                    'in_place_ms': out[f]['paste_in_place']['median_ms'],
                                                    'in_place_GB_per_s': out[f]['in_place_GB_per_s']} for f in ('rgb24', 'nv12')}}))
        return
    from oracle import istvt_ref as R
    grid = R.stem_out_side(a.size)
    dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float32
    torch.manual_seed(0)
    model = XceptionVidTr(num_frames=a.T, grid=grid, depth=a.depth, compute_dtype=dt).cuda().eval()
    if a.videos:
        out = {'size': a.size, 'T': a.T, 'depth': a.depth, 'dtype': a.dtype, 'frame_batch': a.frame_batch,
               'window_batch': a.window_batch, 'reps': a.reps, 'warmup': a.warmup, 'strides': videos_bench(a, model)}
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(out, f, indent=1)
        print(json.dumps({'video_set_bench': {k: {'loop_over_set': v['loop_over_set'],
                                                  'set_ms_per_32_windows': v['set_ms_per_32_windows']}
                                              for k, v in out['strides'].items()}}))
        return
    if a.align:
        out = dict(align_bench(a, model), T=a.T, depth=a.depth, dtype=a.dtype, frame_batch=a.frame_batch,
                   window_batch=a.window_batch, reps=a.reps, warmup=a.warmup)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(out, f, indent=1)
        print(json.dumps({'video_align_bench': {'warp_u8_ms': out['warp_similarity_u8']['median_ms'],
                                                'warp_nv12_ms': out['warp_similarity_nv12']['median_ms'],
                                                'crop_resize_u8_ms': out['crop_resize_u8']['median_ms'],
                                                'warp_over_crop': out['warp_over_crop']}}))
        return
    if a.nv12:
        out = dict(nv12_bench(a, model), T=a.T, depth=a.depth, dtype=a.dtype, frame_batch=a.frame_batch,
                   window_batch=a.window_batch, reps=a.reps, warmup=a.warmup)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(out, f, indent=1)
        print(json.dumps({'video_nv12_bench': {'fused_ms': out['fused']['median_ms'],
                                               'convert_then_crop_ms': out['convert_then_crop']['median_ms'],
                                               'crop_resize_u8_ms': out['crop_resize_u8']['median_ms'], 'equal_bits': out['equal_bits']}}))
        return
    if a.boxes:
        out = dict(boxes_bench(a, model), T=a.T, depth=a.depth, dtype=a.dtype, frame_batch=a.frame_batch,
                   window_batch=a.window_batch, reps=a.reps, warmup=a.warmup)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(out, f, indent=1)
        print(json.dumps({'video_boxes_bench': {'kernel_ms': out['kernel']['median_ms'], 'kernel_GB_per_s': out['kernel']['GB_per_s'],
                                                'copy_GB_per_s': out['copy']['GB_per_s'],
                                                'crop_cost_share': {k: v['crop_cost_share'] for k, v in out['strides'].items()}}}))
        return
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (a.frames, a.size, a.size, 3), generator=g, dtype=torch.uint8)
    xn = (((u8.float() / 255) - torch.tensor(video.DEFAULT_MEAN)) / torch.tensor(video.DEFAULT_STD)).permute(0, 3, 1, 2).contiguous()
    u8, xn = u8.cuda(), xn.cuda()
    if a.explain:
        out = {'frames': a.frames, 'size': a.size, 'T': a.T, 'depth': a.depth, 'dtype': a.dtype, 'frame_batch': a.frame_batch,
               'window_batch': a.window_batch, 'reps': a.reps, 'warmup': a.warmup, 'explain': explain_bench(a, model, u8, xn)}
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, 'w') as f:
                json.dump(out, f, indent=1)
        print(json.dumps({'video_explain_bench': {k: v['loop_over_explain'] for k, v in out['explain'].items()}}))
        return
    out = {'frames': a.frames, 'size': a.size, 'T': a.T, 'depth': a.depth, 'dtype': a.dtype, 'frame_batch': a.frame_batch,
           'window_batch': a.window_batch, 'reps': a.reps, 'warmup': a.warmup, 'strides': {}}
    for stride in [int(s) for s in a.strides.split(',')]:
        scorer = video.VideoScorer(model, stride=stride, frame_batch=a.frame_batch, window_batch=a.window_batch)
        starts = video.window_starts(a.frames, a.T, stride, True)
        W = len(starts)
        tab = (torch.tensor(starts).view(-1, 1) + torch.arange(a.T).view(1, -1)).cuda()
        res = {}

        def run_scorer():
            res['a'] = scorer.score(u8).window_logits

        def run_clips():
            with torch.no_grad():
                res['b'] = torch.cat([model(xn[tab[i:i + a.window_batch]]) for i in range(0, W, a.window_batch)])
        ta, tb = [], []
        for r in range(a.warmup + a.reps):
            x, y = timed(run_scorer), timed(run_clips)
            if r >= a.warmup:
                ta.append(x)
                tb.append(y)
        diff = float((res['a'] - res['b']).abs().max())
        # one instrumented run of (a): events around the three phases and the two new kernels (ops.prof)
        ops.kernel_profile = []
        stem0, gather0, ft0 = scorer._stem, ops.tokens_gather_fwd, model.vit.forward_tokens

        def wrap(name, fn):
            def f(*p, **k):
                with ops.prof(name):
                    return fn(*p, **k)
            return f
        try:
            scorer._stem = wrap('phase:stem', stem0)
            ops.tokens_gather_fwd = wrap('phase:tokens', gather0)
            model.vit.forward_tokens = wrap('phase:transformer', ft0)
            run_scorer()
            torch.cuda.synchronize()
            split = {}
            for name, e0, e1, nbytes, flops in ops.kernel_profile:
                if name.startswith('phase:') or name in ('conv1_fwd_u8', 'tokens_gather_fwd'):
                    d = split.setdefault(name.replace('phase:', ''), {'ms': 0.0, 'bytes': 0})
                    d['ms'] += e0.elapsed_time(e1)
                    d['bytes'] += nbytes
        finally:
            ops.kernel_profile = None
            scorer._stem, ops.tokens_gather_fwd = stem0, gather0
            del model.vit.forward_tokens                   # the instance attribute; the method is back
        sa, sb = stats(ta), stats(tb)
        rec = {'windows': W, 'scorer': sa, 'clip_path': sb, 'scorer_windows_per_s': W / sa['median_ms'] * 1e3,
               'clip_path_windows_per_s': W / sb['median_ms'] * 1e3, 'speedup': sb['median_ms'] / sa['median_ms'],
               'clip_path_spread': (sb['max_ms'] - sb['min_ms']) / sb['median_ms'],
               'scorer_spread': (sa['max_ms'] - sa['min_ms']) / sa['median_ms'], 'max_abs_logit_diff': diff, 'split_ms': split}
        out['strides'][str(stride)] = rec
        print('stride %d: %d windows | scorer %.1f ms (%.1f-%.1f) = %.1f windows/s | clip path %.1f ms (%.1f-%.1f) = %.1f windows/s'
              ' | x%.2f | max |logit diff| %.2e' % (stride, W, sa['median_ms'], sa['min_ms'], sa['max_ms'], rec['scorer_windows_per_s'],
                                                   sb['median_ms'], sb['min_ms'], sb['max_ms'], rec['clip_path_windows_per_s'],
                                                   rec['speedup'], diff), flush=True)
        print('          split of one instrumented scorer run: ' +
              ', '.join('%s %.2f ms' % (k, v['ms']) for k, v in split.items()), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps({'video_bench': {k: {'scorer_windows_per_s': v['scorer_windows_per_s'],
                                          'clip_path_windows_per_s': v['clip_path_windows_per_s']}
                                      for k, v in out['strides'].items()}}))


if __name__ == '__main__':
    main()
