#!/usr/bin/env python3
"""The fused BatchNorm-backward + 1x1-convolution backward (ops.pw_bwd) against the three launches it replaces, at
block1's two shapes of the C2 training step (run on the GPU box):

    python tools/pw_bwd_bench.py [--rows 3041536] [--rounds 9] [--out profiles/r20_pw_bwd.txt]

Both forms run alternately in one process, each timed with device events around its launches (the parent form: the
BatchNorm-backward apply, the weight gradient with its slab reduce, the input gradient).  Prints the median and the
min..max range over the rounds and the achieved TB/s over the ALGORITHMIC bytes of the fused form
(dz, u, d read; dd written), which both forms are charged with.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import ops, stem  # noqa: E402

PEAK_TBS = 6.3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return e0, e1, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=256 * 109 * 109)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error('--rounds: at least 7')
    M, dt, dev = a.rows, torch.bfloat16, torch.device('cuda')
    lines = ['pw_bwd_bench: M = %d rows, %d rounds, fused and three-launch form alternating in one process (%s)'
             % (M, a.rounds, torch.cuda.get_device_name(0))]
    for cin, cout in ops.PW_BWD_PAIRS:
        torch.manual_seed(cin)
        dz = torch.randn(M, cout, device=dev).to(dt)
        u = (torch.randn(M, cout, device=dev) * 1.5 + 0.25).to(dt)
        d = torch.randn(M, cin, device=dev).to(dt)
        w = ops.empty_rows(cout, cin, dt, dev, True)                    # line-aligned rows, as ops.weight_as(pad=True) gives
        w.copy_((torch.randn(cout, cin, device=dev) / cin ** 0.5).to(dt))
        gamma, beta = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
        st = stem.bn_forward_stats(u, M, cout, gamma, beta, torch.zeros(cout, device=dev), torch.ones(cout, device=dev), True)
        stats = stem._bn_backward_sums(dz, u, st, M, cout, None)        # reduced once; both forms read replica 0
        out = torch.zeros((cout, cin), device=dev)
        dg, db = torch.zeros(cout, device=dev), torch.zeros(cout, device=dev)
        assert ops.pw_bwd_fusable(dz, d, w)

        def fused():
            return ops.pw_bwd(dz, u, st.pack, gamma, stats, d, w, out, dg, db, True)

        def parent():
            du = stem._bn_backward_apply(dz, u, st, gamma, M, cout, stats, dg, db, True)
            ops.linear_wgrad(du, d, out=out)
            return ops.linear_dgrad(du, w, blocked=False)

        fused(); parent(); torch.cuda.synchronize()                     # warm-up: allocator, transposed operand
        ev = {'fused': [], 'parent': []}
        for _ in range(a.rounds):
            for name, fn in (('fused', fused), ('parent', parent)):
                e0, e1, r = timed(fn)
                del r
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
        alg = (2 * M * cout + 2 * M * cin) * 2
        par = (3 * M * cout + 2 * (M * cout + M * cin)) * 2             # what the three launches move (slabs aside)
        lines.append('(Cin, Cout) = (%d, %d): algorithmic bytes %.0f MB (three launches move %.0f MB: ratio %.2f)'
                     % (cin, cout, alg / 1e6, par / 1e6, alg / par))
        for k in ('fused', 'parent'):
            t = ms[k]
            med = statistics.median(t)
            lines.append('  %-6s median %8.1f us  range %8.1f .. %8.1f us  %5.2f TB/s over the algorithmic bytes (%.0f %% of %.1f)'
                         % (k, med * 1e3, min(t) * 1e3, max(t) * 1e3, alg / (med * 1e-3) / 1e12,
                            100 * alg / (med * 1e-3) / 1e12 / PEAK_TBS, PEAK_TBS))
        gain = statistics.median(ms['parent']) - statistics.median(ms['fused'])
        spread = max(ms['parent']) - min(ms['parent'])
        lines.append('  fused is %.1f us %s than the three launches; their own min-max range is %.1f us -> %s'
                     % (abs(gain) * 1e3, 'faster' if gain > 0 else 'SLOWER', spread * 1e3,
                        'a gain beyond the range' if gain > spread else 'NOT below the parent by more than its range'))
        del dz, u, d
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'a') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
