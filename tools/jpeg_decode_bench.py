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
"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--split', action='store_true')
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cache', default=None)
    ap.add_argument('--encode-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
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
