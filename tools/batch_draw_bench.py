"""The input side of a training step drawn on the device (DESIGN.md "Batch draw"), measured on the MI355X.

    python tools/batch_draw_bench.py [--clips 32] [--frames 8] [--size 224] [--bank-files 4096] [--reps 30] [--out FILE]

A clips.JpegBank of --bank-files files of --size x --size (8 distinct frames encoded on the device at quality 90 with a restart
marker per MCU row, repeated: videos of 32 consecutive places), from which every batch takes --clips clips of --frames frames,
cropped and resized to --size, recompressed and perturbed.  Two input sides, timed in alternation:

  host    today's: torch.randint for the clips, clips.random_boxes / random_views / random_qualities / random_perturbations on
          the host, then ops.decode_frames(bank, S, boxes, index=...), ops.jpeg_roundtrip_u8 and ops.perturb_u8 on the host
          tables, which each validates and uploads
  draw    ops.draw_clips(bank, plan, S, out=...): one call, no host table -- eager, and as a replayed torch.cuda.graph

For each: the host's wall time until the call has returned (the stream drained before, not after: what the Python thread
spends per batch), and the device time between two events around it.  The draw kernel alone is timed as a captured graph of
--chain launches of ops.batch_draw, replayed: device time per launch, the gaps between graph nodes included; its kernel time
without them is rocprofv3's (`rocprofv3 --kernel-trace --stats -d DIR -- python tools/batch_draw_bench.py --reps 3`).
Before anything is timed the draw side's bytes are compared with the existing calls on clips.batch_draw_host's tables.

    python tools/batch_draw_bench.py --restartless [...]

instead (DESIGN.md "JPEG bank, split"): the same bank from files WITHOUT restart markers, and ops.draw_clips on it with
with_split(128) and with with_split(None), eager and as replayed graphs, in alternation; the two give the same bytes, which
is checked at two steps first."""
import argparse
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
VIDEO_FRAMES = 32


def smooth_image(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8)


def stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def measure(fn):
    """(host ms until fn has returned, device ms between events around it), the stream drained before"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    e1.record()
    e1.synchronize()
    return host, e0.elapsed_time(e1)


def restartless_main(a):
    """--restartless: draw_clips on a bank of restart-less files, with and without the bank's split"""
    B, T, S, N = a.clips, a.frames, a.size, a.bank_files
    dev = torch.device('cuda', torch.cuda.current_device())
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)]).to(dev)
    headers = [clips.jpeg_parse(f) for f in ops.jpeg_encode_u8(src, 90, '420', 0).files()]
    plain = clips.jpeg_bank([headers[i % DISTINCT] for i in range(N)])
    split = plain.with_split(clips.JPEG_SPLIT_DEFAULT)
    plain.on(dev)
    V = N // VIDEO_FRAMES
    videos = torch.tensor([[v * VIDEO_FRAMES, VIDEO_FRAMES, v & 1] for v in range(V)], dtype=torch.int32)
    banks = {'one_lane': plain, 'split': split}
    plans = {k: clips.BatchPlan(plain, videos, T=T, B=B, seed=2023).on(dev) for k in banks}
    outs = {k: torch.empty((B, T, S, S, 3), dtype=torch.uint8, device=dev) for k in banks}
    for step in (0, 1):                                             # the bytes first
        got = {k: ops.draw_clips(banks[k], plans[k], S, out=outs[k]) for k in banks}
        clips.check_jpeg_bank_status(got['split'][3])
        if not all(torch.equal(x, y) for x, y in zip(got['split'], got['one_lane'])):
            raise SystemExit('step %d: draw_clips on the split bank is not draw_clips on the bank without a split' % step)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in banks:
            ops.draw_clips(banks[k], plans[k], S, out=outs[k])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs = {}
    for k in banks:
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k], capture_error_mode='thread_local'):
            ops.draw_clips(banks[k], plans[k], S, out=outs[k])
    torch.cuda.synchronize()
    sides = [(k + '_eager', (lambda k=k: ops.draw_clips(banks[k], plans[k], S, out=outs[k]))) for k in banks]
    sides += [(k + '_graph', graphs[k].replay) for k in banks]
    times = {name: ([], []) for name, _ in sides}
    for r in range(a.warmup + a.reps):
        for name, fn in sides[::1 if r % 2 == 0 else -1]:
            host, device = measure(fn)
            if r >= a.warmup:
                times[name][0].append(host)
                times[name][1].append(device)
    res = {'clips': B, 'frames': T, 'size': S, 'bank_files': N, 'chunk_bytes': split.split, 'chunk_rows': split.chunk_rows,
           'seg_bytes_max': split.seg_bytes_max}
    lines = ['batch draw, restart-less bank: %d clips of %d frames at %d x %d from %d files, longest scan %d bytes, split %d with %d '
             'state rows per segment' % (B, T, S, S, N, split.seg_bytes_max, split.split, split.chunk_rows)]
    for name, _ in sides:
        res[name] = {'host': stats(times[name][0]), 'device': stats(times[name][1])}
        h, d = res[name]['host'], res[name]['device']
        lines.append('  %-18s host %.3f ms (%.3f-%.3f) | device %.3f ms (%.3f-%.3f)'
                     % (name, h['median_ms'], h['min_ms'], h['max_ms'], d['median_ms'], d['min_ms'], d['max_ms']))
    print('\n'.join(lines), flush=True)
    line = json.dumps({'batch_draw_restartless_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=32)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--bank-files', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--chain', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--restartless', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('batch_draw_bench.py measures on a GPU; none is visible')
    if a.restartless:
        return restartless_main(a)
    B, T, S, N = a.clips, a.frames, a.size, a.bank_files
    dev = torch.device('cuda', torch.cuda.current_device())
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)]).to(dev)
    files = ops.jpeg_encode_u8(src, 90, '420', 'row').files()
    headers = [clips.jpeg_parse(f) for f in files]                  # parsed once: the bank's files are these 8, repeated
    bank = clips.jpeg_bank([headers[i % DISTINCT] for i in range(N)])
    bank.on(dev)
    V = N // VIDEO_FRAMES
    videos = torch.tensor([[v * VIDEO_FRAMES, VIDEO_FRAMES, v & 1] for v in range(V)], dtype=torch.int32)
    plan = clips.BatchPlan(bank, videos, T=T, B=B, seed=2023)
    seed = plan.seed

    # the bytes first: draw_clips against the existing calls on the definition's host tables, at two steps
    plan.on(dev)
    out = torch.empty((B, T, S, S, 3), dtype=torch.uint8, device=dev)
    for step in (0, 1):
        d = clips.batch_draw_host(plan, step)
        want = ops.decode_frames(bank, S, d.boxes, index=d.index)
        want = ops.jpeg_roundtrip_u8(want, d.quality)
        want = ops.perturb_u8(want.view(B, T, S, S, 3), d.perturb, plan.taps, seed)
        got, view, label, status = ops.draw_clips(bank, plan, S, out=out)
        clips.check_jpeg_bank_status(status)
        if not (torch.equal(got, want) and torch.equal(view.cpu(), d.view) and torch.equal(label.cpu(), d.label)):
            raise SystemExit('step %d: draw_clips is not the chain of existing calls on the host tables' % step)

    gen = torch.Generator().manual_seed(1)
    starts = VIDEO_FRAMES - (T - 1)

    def host_side():
        v = torch.randint(0, V, (B,), generator=gen)
        first = v * VIDEO_FRAMES + torch.randint(0, starts, (B,), generator=gen)
        index = (first[:, None] + torch.arange(T)[None, :]).reshape(-1)
        boxes = clips.per_frame_boxes(clips.random_boxes(B, S, S, generator=gen), T)
        flips = clips.random_views(B, S, S, S, generator=gen)
        quality = clips.random_qualities(B, generator=gen)
        table, taps = clips.random_perturbations(B, generator=gen)
        u8 = ops.decode_frames(bank, S, boxes, index=index).view(B, T, S, S, 3)
        u8 = ops.jpeg_roundtrip_u8(u8, quality)
        u8 = ops.perturb_u8(u8, table, taps, seed)
        return u8, flips.to(dev, non_blocking=True), (v & 1).to(dev, non_blocking=True)

    def draw_side():
        return ops.draw_clips(bank, plan, S, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draw_side()
        ops.batch_draw(plan)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    whole = torch.cuda.CUDAGraph()
    with torch.cuda.graph(whole, capture_error_mode='thread_local'):
        draw_side()
    chain = torch.cuda.CUDAGraph()
    with torch.cuda.graph(chain, capture_error_mode='thread_local'):
        for _ in range(a.chain):
            ops.batch_draw(plan)
    torch.cuda.synchronize()

    sides = (('host', host_side), ('draw_eager', draw_side), ('draw_graph', whole.replay), ('draw_kernel_chain', chain.replay))
    times = {name: ([], []) for name, _ in sides}
    for r in range(a.warmup + a.reps):
        for name, fn in sides[::1 if r % 2 == 0 else -1]:           # in alternation, either end first in turn
            host, device = measure(fn)
            if r >= a.warmup:
                times[name][0].append(host)
                times[name][1].append(device)
    step = plan.step
    res = {'clips': B, 'frames': T, 'size': S, 'bank_files': N, 'videos': V, 'chain': a.chain, 'steps_drawn': step,
           'block_ints': int(plan.block.numel())}
    lines = ['batch draw: %d clips of %d frames at %d x %d from a bank of %d files (%d videos), draw block of %d ints'
             % (B, T, S, S, N, V, plan.block.numel())]
    for name, _ in sides:
        res[name] = {'host': stats(times[name][0]), 'device': stats(times[name][1])}
        h, d = res[name]['host'], res[name]['device']
        lines.append('  %-18s host %.3f ms (%.3f-%.3f) | device %.3f ms (%.3f-%.3f)'
                     % (name, h['median_ms'], h['min_ms'], h['max_ms'], d['median_ms'], d['min_ms'], d['max_ms']))
    per = res['draw_kernel_chain']['device']
    res['draw_kernel_us_per_launch_in_graph'] = {k.replace('_ms', '_us'): v * 1e3 / a.chain for k, v in per.items()}
    lines.append('  the draw kernel in a graph of %d launches: %.2f us per launch (%.2f-%.2f), gaps between nodes included'
                 % (a.chain, per['median_ms'] * 1e3 / a.chain, per['min_ms'] * 1e3 / a.chain, per['max_ms'] * 1e3 / a.chain))
    print('\n'.join(lines), flush=True)
    line = json.dumps({'batch_draw_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
