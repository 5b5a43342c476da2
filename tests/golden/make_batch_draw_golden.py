"""Writes tests/golden/B1_batch_draw.json: the arguments of one small clips.BatchPlan and the tables clips.batch_draw_host
draws from it at three steps, 2^32 - 1 and 2^32 among them (the carry into the counter's second word).  The record pins the
definition (DESIGN.md "Batch draw"): tests/test_batch_draw_cpu.py rebuilds the plan from the arguments and compares.

    python tests/golden/make_batch_draw_golden.py

The plan: four videos of 3, 4, 7 and 12 frames over a bank of 26 places of two image sizes, ragged base boxes with a 1 x 1 box
and a box equal to its image among them, T = 3, K = 16."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

STEPS = (7, 2 ** 32 - 1, 2 ** 32)


def plan_arguments():
    sizes = [[24, 40]] * 14 + [[17, 33]] * 12
    base = []
    for i, (h, w) in enumerate(sizes):
        y0, x0 = i % 5, (3 * i) % 7
        base.append([y0, x0, h - y0 - (i % 3), w - x0 - (2 * i) % 5])
    base[1] = [5, 7, 1, 1]
    base[4] = [0, 0, 24, 40]                                      # equal to its image
    base[20] = [0, 0, 17, 33]
    base[9] = [3, 2, 2, 30]                                       # a sliver
    return dict(sizes=sizes, videos=[[0, 3, 0], [3, 4, 1], [7, 7, 0], [14, 12, 1]], T=3, B=5, stride=1, base=base, K=16,
                flip_p=0.5, jpeg=[0.5, 30, 95], perturb_p=0.5, seed=0x9E3779B97F4A7C15)


def build(clips, args, **over):
    import torch
    a = dict(args, **over)
    perturb = None if a['perturb_p'] is None else (a['perturb_p'], ('brightness', 'contrast', 'saturation', 'noise', 'blur',
                                                                    'pixelate'), None)
    return clips.BatchPlan([tuple(s) for s in a['sizes']], a['videos'], T=a['T'], B=a['B'], stride=a['stride'],
                           base=torch.tensor(a['base'], dtype=torch.int32), K=a['K'], flip_p=a['flip_p'],
                           jpeg=None if a['jpeg'] is None else tuple(a['jpeg']), perturb=perturb, seed=a['seed'])


def main():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    args = plan_arguments()
    plan = build(clips, args)
    record = dict(plan=args, shapes=plan.shapes.tolist(), kinds=plan.kinds.tolist(), steps={})
    for s in STEPS:
        d = clips.batch_draw_host(plan, s)
        record['steps'][str(s)] = {k: getattr(d, k).tolist() for k in ('index', 'boxes', 'quality', 'view', 'perturb', 'label')}
    with open(os.path.join(HERE, 'B1_batch_draw.json'), 'w') as fh:
        json.dump(record, fh, indent=None, separators=(',', ':'))
        fh.write('\n')


if __name__ == '__main__':
    main()
