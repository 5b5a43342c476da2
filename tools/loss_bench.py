#!/usr/bin/env python
"""The tail of a training step between the logits and the start of the model's backward, plus the matching head of the
backward: the torch criterion with the accuracy count and two HostScalar reads -- what bench.py's
with_host_boundary leg does every step -- against the fused criterion with a device meter.

At B = 32 and B = 1, on (B, 1) float32 leaf logits, event-timed and alternating in ONE process:

    torch       BCEWithLogitsLoss + (logits > 0) == labels count + HostScalar(loss), HostScalar(count) + backward to the
                logits + both reads
    fused       loss.BCEWithLogitsLoss(meter=TrainMeter) + backward to the logits; nothing is read
    fused_snap  the same with meter.snapshot() taken AND read every step (the loop only prints now and then)
    torch2      `torch` again: the A/A repeat whose difference from `torch` is the spread of this box

`device us` is event time per step over `--steps` steps back to back, `host us` the host's wall time per step for enqueueing
them (reads included where a leg has them).  Then the forward kernel alone, all outputs and a meter, at n = 32 and 2^20.

    python tools/loss_bench.py [--rounds 9] [--steps 200] [--warmup 20] [--out profiles/r15_fused_loss.txt]

Run it under its own `timeout`.
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
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import loss as L
    from istvt_amd import ops, parallel
    if not torch.cuda.is_available():
        raise SystemExit('loss_bench needs a GPU: a time taken anywhere else says nothing')
    dev = torch.device('cuda', 0)
    gen = torch.Generator().manual_seed(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    result = {}
    for B in (32, 1):
        logits = (torch.randn((B, 1), generator=gen) * 2).to(dev).requires_grad_()
        lab = (torch.rand((B,), generator=gen) > 0.5).float().to(dev)
        crit_t = torch.nn.BCEWithLogitsLoss()
        meter = L.TrainMeter(dev)
        crit_f = L.BCEWithLogitsLoss(meter=meter)
        sink = {}

        def leg_torch():
            logits.grad = None
            loss = crit_t(logits.view(-1), lab)
            hl = parallel.HostScalar(loss)
            ha = parallel.HostScalar(torch.sum((logits.detach().view(-1) > 0).float() == lab))
            loss.backward()
            sink['loss'], sink['acc'] = float(hl), int(ha)

        def leg_fused():
            logits.grad = None
            crit_f(logits.view(-1), lab).backward()

        def leg_fused_snap():
            logits.grad = None
            crit_f(logits.view(-1), lab).backward()
            snap = meter.snapshot()
            sink['loss'], sink['acc'] = snap.batch_loss_sum, snap.counts['correct']

        legs = {'torch': leg_torch, 'fused': leg_fused, 'fused_snap': leg_fused_snap, 'torch2': leg_torch}
        order = list(legs)
        dev_us = {k: [] for k in order}
        host_us = {k: [] for k in order}
        for k in order:
            for _ in range(a.warmup):
                legs[k]()
        torch.cuda.synchronize()
        # the two criteria agree before anything is timed
        leg_torch()
        g_t = logits.grad.clone()
        leg_fused()
        ref = L.bce_logits_ref(logits.detach().view(-1), lab)
        assert abs(sink['loss'] - float(ref['reduced'])) <= 2e-5 * abs(float(ref['reduced']))
        assert float((logits.grad - g_t).norm()) <= 2e-5 * float(g_t.norm())
        for _ in range(a.rounds):
            for k in order:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                t0.record()
                for _ in range(a.steps):
                    legs[k]()
                t1.record()
                h1 = time.perf_counter()
                t1.synchronize()
                dev_us[k].append(t0.elapsed_time(t1) * 1e3 / a.steps)
                host_us[k].append((h1 - h0) * 1e6 / a.steps)
        say('B = %d: %d rounds of %d steps, microseconds per step' % (B, a.rounds, a.steps))
        say('  %-10s %12s %9s %9s %12s' % ('leg', 'device med', 'min', 'max', 'host med'))
        result['B%d' % B] = {}
        for k in order:
            say('  %-10s %12.1f %9.1f %9.1f %12.1f' % (k, statistics.median(dev_us[k]), min(dev_us[k]), max(dev_us[k]),
                                                      statistics.median(host_us[k])))
            result['B%d' % B][k] = {'device_us': round(statistics.median(dev_us[k]), 2), 'min_us': round(min(dev_us[k]), 2),
                                    'max_us': round(max(dev_us[k]), 2), 'host_us': round(statistics.median(host_us[k]), 2)}
        aa = abs(statistics.median(dev_us['torch']) - statistics.median(dev_us['torch2']))
        say('  A/A spread (torch against torch2) %.1f us; fused - torch = %+.1f us'
            % (aa, statistics.median(dev_us['fused']) - statistics.median(dev_us['torch'])))

    say('the forward kernel alone (per-sample loss, reduced loss, gradient and meter), back to back, microseconds per call')
    result['kernel'] = {}
    for n in (32, 1 << 20):
        z = (torch.randn(n, generator=gen) * 2).to(dev)
        y = (torch.rand(n, generator=gen) > 0.5).to(dev)
        block = torch.zeros(ops.METER_WORDS, dtype=torch.int64, device=dev)
        calls = 200 if n == 32 else 20

        def kernel():
            ops.bce_logits(z, y, None, 1.0, 0.0, 'mean', 0.0, want_loss=True, want_reduced=True, want_grad=True, meter=block)
        for _ in range(5):
            kernel()
        times = []
        for _ in range(a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(calls):
                kernel()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1) * 1e3 / calls)
        say('  n = %-8d median %9.1f  min %9.1f  max %9.1f' % (n, statistics.median(times), min(times), max(times)))
        result['kernel']['n%d' % n] = {'median_us': round(statistics.median(times), 2), 'min_us': round(min(times), 2)}
    say(json.dumps({'loss_bench': result, 'rounds': a.rounds, 'steps': a.steps}))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
