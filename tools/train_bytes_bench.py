#!/usr/bin/env python
"""Training from bytes against training from float32 clips (DESIGN.md "Training from bytes").

The C2 training step (B = 32 clips x T = 8 frames x 224^2, depth 12, bf16, FusedSGD on the fused bucket) on

    float_resident   float32 NCHW clips already on the device                     (what bench.py times)
    float_resident2  the same again: the A/A repeat that shows the spread
    u8_resident      uint8 NHWC clips already on the device
    float_host       float32 clips with the reference loop's host boundary: pinned, double-buffered H2D copy of the next
                     batch under the current step, loss.item() every step (bench.py's with_host_boundary leg)
    u8_host          uint8 clips with the same host boundary
    u8_view_host     uint8 256^2 sources with random crop / flip views, same host boundary

in ONE process, legs alternating, `--repeats` rounds of `--steps` steps each; the median over the rounds is reported.
Every leg runs as the parent commit's step does except for the input.  One JSON line at the end.

    python tools/train_bytes_bench.py [--repeats 5] [--steps 10] [--warmup 3] [--out profiles/r10_train_bytes.txt]
    python tools/train_bytes_bench.py --profile-steps 3      # a few steps of the float and the byte leg, for one
                                                             # `rocprofv3 --kernel-trace --stats -- python ...` run

Run each invocation under its own `timeout`.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--source', type=int, default=256, help='side of the larger source frames of the view leg')
    ap.add_argument('--depth', type=int, default=12)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--profile-steps', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips, parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr

    dev = torch.device('cuda', 0)
    B, T, S, Hs = a.batch, a.frames, a.size, a.source
    # the grid the entry flow makes of an S x S crop
    h = ((S - 3) // 2 + 1) - 2
    for _ in range(3):
        h = (h - 1) // 2 + 1
    torch.manual_seed(0)
    model = XceptionVidTr(num_frames=T, grid=h, depth=a.depth, compute_dtype=torch.bfloat16).to(dev).train()
    model.set_crop_side(S)
    live = [p for _, p in parallel.live_named_parameters(model)]
    bucket = parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
    opt = parallel.FusedSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=0, zero_grad=True)
    crit = torch.nn.BCEWithLogitsLoss()
    g = torch.Generator().manual_seed(1)

    host = {
        'float': [torch.randn((B, T, 3, S, S), generator=g).pin_memory() for _ in range(2)],
        'u8': [torch.randint(0, 256, (B, T, S, S, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(2)],
        'u8_view': [torch.randint(0, 256, (B, T, Hs, Hs, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(2)],
    }
    views = [clips.random_views(B, Hs, Hs, S, g).pin_memory() for _ in range(2)]
    labels = [(torch.rand((B,), generator=g) > 0.5).float().pin_memory() for _ in range(2)]
    dlab = [t.to(dev) for t in labels]
    copy_stream = torch.cuda.Stream(device=dev)

    def step(x, y, view=None):
        opt.zero_grad()
        logits = model(x, view=view) if view is not None else model(x)
        loss = crit(logits.view(-1), y)
        loss.backward()
        opt.step()
        return loss

    def resident(kind, n):
        x = [t.to(dev) for t in host[kind]]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(n):
            step(x[i % 2], dlab[i % 2])
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e3

    def host_boundary(kind, n):
        dbuf = [torch.empty(t.shape, dtype=t.dtype, device=dev) for t in host[kind]]
        dl = [torch.empty((B,), device=dev) for _ in range(2)]
        ready = [torch.cuda.Event() for _ in range(2)]

        def upload(i):                      # image.cuda() / labels.cuda() of the NEXT batch, under the current step's kernels
            with torch.cuda.stream(copy_stream):
                dbuf[i % 2].copy_(host[kind][i % 2], non_blocking=True)
                dl[i % 2].copy_(labels[i % 2], non_blocking=True)
                ready[i % 2].record(copy_stream)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        running = 0.0
        upload(0)
        for i in range(n):
            torch.cuda.current_stream(dev).wait_event(ready[i % 2])
            if i + 1 < n:
                upload(i + 1)               # its buffer was last read by step i - 1, complete since that step's .item()
            loss = step(dbuf[i % 2], dl[i % 2], views[i % 2] if kind == 'u8_view' else None)
            running += loss.item()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e3

    legs = [('float_resident', lambda n: resident('float', n)), ('u8_resident', lambda n: resident('u8', n)),
            ('float_resident2', lambda n: resident('float', n)), ('float_host', lambda n: host_boundary('float', n)),
            ('u8_host', lambda n: host_boundary('u8', n)), ('u8_view_host', lambda n: host_boundary('u8_view', n))]

    if a.profile_steps:
        for name in ('float_resident', 'u8_resident', 'u8_view_host'):
            dict(legs)[name](a.profile_steps)
        print(json.dumps({'profiled_steps_per_leg': a.profile_steps}))
        return

    for name, fn in legs:
        fn(a.warmup)
    times = {name: [] for name, _ in legs}
    for r in range(a.repeats):
        for name, fn in legs:               # alternating: every leg once per round
            times[name].append(fn(a.steps))
        print('round %d: %s' % (r, ' '.join('%s=%.2f' % (k, v[-1]) for k, v in times.items())), flush=True)
    res = {'config': dict(batch=B, frames=T, size=S, source=Hs, depth=a.depth, dtype='bf16', steps=a.steps, repeats=a.repeats),
           'median_ms_per_step': {k: round(statistics.median(v), 3) for k, v in times.items()},
           'min_ms_per_step': {k: round(min(v), 3) for k, v in times.items()},
           'max_ms_per_step': {k: round(max(v), 3) for k, v in times.items()},
           'h2d_bytes_per_step': {'float': B * T * 3 * S * S * 4, 'u8': B * T * 3 * S * S, 'u8_view': B * T * 3 * Hs * Hs}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            for r in range(a.repeats):
                f.write('round %d: %s\n' % (r, ' '.join('%s=%.3f' % (k, v[r]) for k, v in times.items())))
            f.write(line + '\n')


if __name__ == '__main__':
    main()
