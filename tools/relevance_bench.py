#!/usr/bin/env python3
"""Relevance maps (DESIGN.md "Relevance maps"): the two rollout kernels against the training backward kernels on the same
shapes, and one whole relevance() call against one training step at the same batch (run on the GPU box).

    python tools/relevance_bench.py [--batch 32] [--frames 8] [--size 224] [--depth 12] [--json out.json]

Defaults: C2 (bf16, 32 clips x 8 frames, 224^2 -> 14x14 grid, P = 197, 8 heads x 64).  Kernel times are the mean of 20
launches after one warm-up, bracketed by events; step and call times the median of 5 after 2 warm-ups.
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
from istvt_amd import ops, parallel  # noqa: E402
from istvt_amd.network.vivit.vivit import XceptionVidTr  # noqa: E402


def timeit(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3          # us


def wall(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]                  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--depth', type=int, default=12)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dt = torch.bfloat16
    heads, dh = 8, 64
    inner = heads * dh
    from oracle import istvt_ref as R
    grid = R.stem_out_side(a.size)
    B, F, P = a.batch, a.frames + 1, grid * grid + 1
    out = {'batch': B, 'frames': a.frames, 'size': a.size, 'grid': grid, 'P': P, 'depth': a.depth, 'dtype': 'bf16'}
    g = torch.Generator().manual_seed(0)

    # spatial: BF = B*F frames
    BF = B * F
    qkv = ops.empty_rows(BF * P, 3 * inner, dt, 'cuda')
    qkv.copy_((torch.randn((BF * P, 3 * inner), generator=g) * 0.6).to(dt))
    o, lse = ops.attn_spatial_fwd(qkv, BF, P, heads, dh)
    do = torch.randn(o.shape, generator=g).to(dt).cuda()
    d2 = ops.empty_rows(BF * P, inner, dt, 'cuda')
    d2.copy_(do)
    r_full = torch.rand((BF, P), generator=g).cuda()
    r_e0 = torch.zeros((BF, P), device='cuda')
    r_e0[:, 0] = 1
    out['spatial_bwd_us'] = timeit(lambda: ops.attn_spatial_bwd(qkv, o, d2, lse, BF, P, heads, dh))
    out['spatial_rel_us'] = timeit(lambda: ops.attn_spatial_relevance(qkv, d2, lse, r_full, BF, P, heads, dh))
    out['spatial_rel_e0_us'] = timeit(lambda: ops.attn_spatial_relevance(qkv, d2, lse, r_e0, BF, P, heads, dh))
    out['spatial_ratio'] = out['spatial_rel_us'] / out['spatial_bwd_us']
    out['spatial_rel_tflops'] = 4.0 * BF * heads * P * P * dh / (out['spatial_rel_us'] * 1e-6) / 1e12
    del qkv, o, lse, do, d2

    # temporal: B clips x P positions over F frames, the model's pre-differenced bf16 form (diff = 2)
    M = B * F * P
    qkv = ops.empty_rows(M, 3 * inner, dt, 'cuda')
    qkv.copy_((torch.randn((M, 3 * inner), generator=g) * 0.6).to(dt))
    do = ops.empty_rows(M, inner, dt, 'cuda')
    do.copy_(torch.randn((M, inner), generator=g).to(dt))
    r_t = torch.rand((B * P, F), generator=g).cuda()
    qk, v = qkv[:, :2 * inner], qkv[:, 2 * inner:]
    out['temporal_bwd_us'] = timeit(lambda: ops.attn_temporal_bwd(qk, v, do, B, F, P, heads, dh, diff=2, packed=True))
    out['temporal_rel_us'] = timeit(lambda: ops.attn_temporal_relevance(qkv, do, r_t, B, F, P, heads, dh, 2))
    out['temporal_ratio'] = out['temporal_rel_us'] / out['temporal_bwd_us']
    out['temporal_rel_tbs'] = 4 * M * inner * 2 / (out['temporal_rel_us'] * 1e-6) / 1e12
    del qkv, do, qk, v

    # whole call vs one training step (fused bucket + FusedSGD, eager), same batch
    torch.manual_seed(0)
    model = XceptionVidTr(num_frames=a.frames, grid=grid, depth=a.depth, compute_dtype=dt).cuda().train()
    live = [p for _, p in parallel.live_named_parameters(model)]
    bucket = parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
    opt = parallel.FusedSGD(bucket, lr=1e-3, momentum=0.9, zero_grad=True)
    x = torch.randn((B, a.frames, 3, a.size, a.size), generator=g).cuda()
    y = (torch.rand((B,), generator=g) > 0.5).float().cuda()

    def step():
        opt.zero_grad()
        logits = model(x)
        torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), y).backward()
        opt.step()
    out['train_step_ms'] = wall(step)
    out['relevance_ms'] = wall(lambda: model.relevance(x))
    out['relevance_ratio'] = out['relevance_ms'] / out['train_step_ms']
    for k, v in out.items():
        print('%-20s %s' % (k, ('%.3f' % v) if isinstance(v, float) else v), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
