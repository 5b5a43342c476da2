#!/usr/bin/env python
"""The fused optimizer step with parameter groups, clipping and the gradient-norm pass against the plain step
(DESIGN.md section 14).

The real C2 parameter layout -- live_named_parameters(XceptionVidTr(num_frames=8, grid=14)): 252 parameters, 89,033,873
elements -- in one GradBucket; for FusedSGD and FusedAdamW each, event-timed and alternating in ONE process:

    plain      the default construction: the one-group kernel every training entry point runs
    plain2     the same again: the A/A repeat whose difference from `plain` is the spread of this box
    two        two groups, stem | transformer (2 segments)
    nodecay    no weight decay on biases and norm parameters (the segments alternate: ~250)
    norm       istvt_grad_norm alone (one read of the bucket)
    clipped    max_grad_norm on one group: the norm pass + the step that reads its scale from the step-info block

`--rounds` rounds of `--steps` steps per leg; median / min / max over the rounds, microseconds per step, and the GB/s the
bytes each kernel has to move (SGD 5 x 4 B, AdamW 7 x 4 B, norm 4 B per element; no fused zero-grad) make of it.

    python tools/optim_bench.py [--rounds 7] [--steps 20] [--warmup 3] [--out profiles/r13_fused_optim.txt]

Run it under its own `timeout`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def c2_layout():
    """(name, shape) of the live parameters at C2, without allocating them"""
    import torch
    from istvt_amd import parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    with torch.device('meta'):
        model = XceptionVidTr(num_frames=8, grid=14)
    return [(name, tuple(p.shape)) for name, p in parallel.live_named_parameters(model)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import _lib, ops, parallel
    if not torch.cuda.is_available():
        raise SystemExit('optim_bench needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    layout = c2_layout()
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    result = {}
    for kind in ('sgd', 'adamw'):
        params = [torch.nn.Parameter(torch.randn(shape, device=dev, generator=gen) * 0.02) for _, shape in layout]
        names = [n for n, _ in layout]
        bucket = parallel.GradBucket(params, flatten_params=True)
        n = bucket.numel
        grad = torch.randn(n, device=dev, generator=gen) * 1e-3
        stem = [p for nm, p in zip(names, params) if nm.startswith('xcep.')]
        no_decay = [p for p in params if p.dim() <= 1]

        def make(**kw):
            if kind == 'sgd':
                return parallel.FusedSGD(bucket, lr=1e-3, momentum=0.9, weight_decay=1e-2, **kw)
            return parallel.FusedAdamW(bucket, lr=1e-3, weight_decay=1e-2, **kw)

        opts = {'plain': make(), 'plain2': make(),
                'two': make(param_groups=[{'params': stem, 'lr': 1e-4}]),
                'nodecay': make(param_groups=[{'params': no_decay, 'weight_decay': 0.0}]),
                'clipped': make(max_grad_norm=1.0)}
        segs = {k: (1 if o._seg is None else o._seg[0].numel()) for k, o in opts.items()}
        lib = _lib.lib()
        ws = torch.empty(lib.istvt_grad_norm_ws_elems(n), dtype=torch.float64, device=dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)

        def norm_alone():
            _lib.check(lib.istvt_grad_norm(bucket.flat.data_ptr(), n, 1.0, 0.0, 0, ws.data_ptr(), ws.numel(), info.data_ptr(),
                                           ops._stream()), 'istvt_grad_norm')

        legs = {k: o.step for k, o in opts.items()}
        legs['norm'] = norm_alone
        order = ['plain', 'two', 'nodecay', 'norm', 'clipped', 'plain2']
        bytes_per = {'norm': 4}
        per_elem = 20 if kind == 'sgd' else 28
        times = {k: [] for k in order}
        bucket.flat.copy_(grad)
        for k in order:
            for _ in range(a.warmup):
                legs[k]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k in order:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    legs[k]()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) * 1e3 / a.steps)
        assert bool(torch.isfinite(bucket.flat_params).all())
        say('%s: %d parameters, %d elements, norm of the bucket %.6g' % (kind, len(params), n, info[:1].view(torch.float32).item()))
        say('  %-8s %9s %9s %9s %9s %8s' % ('leg', 'segments', 'median us', 'min us', 'max us', 'GB/s'))
        result[kind] = {}
        for k in order:
            med = statistics.median(times[k])
            moved = n * (bytes_per.get(k, per_elem) + (4 if k == 'clipped' else 0))
            say('  %-8s %9s %9.1f %9.1f %9.1f %8.0f' % (k, '-' if k == 'norm' else segs[k], med, min(times[k]), max(times[k]),
                                                       moved / med / 1e3))
            result[kind][k] = {'median_us': round(med, 2), 'min_us': round(min(times[k]), 2), 'max_us': round(max(times[k]), 2)}
        del opts, legs, params, bucket, grad
        torch.cuda.empty_cache()
    say(json.dumps({'optim_bench': result, 'rounds': a.rounds, 'steps': a.steps}))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
