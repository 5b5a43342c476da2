#!/usr/bin/env python3
"""Capture golden vector G10 (relevance maps, DESIGN.md "Relevance maps") from the *reference's own modules*.

Runs ONLY in the build container, where the reference is mounted, in the style of make_golden.py (which it does not
touch).  Drives the reference DSTTr with the ``g4.`` recipe (T = 4 and 8, B = 2) in float64, records every
``softmax`` output A and its gradient G = dy/dA (y = sum_b logits[b, 0]) by wrapping ``torch.Tensor.softmax`` during the
forward, and rolls them out:

    Abar_l = mean_h max(0, A_{l,h} * G_{l,h});   r = e_0;  r <- r + r Abar_l  for l = L-1 .. 0

per (clip, frame) over tokens (spatial) and per (clip, position) over frames (temporal).  Stores only OUTPUTS:
logits, cam_s, cam_t, r_s, r_t and a row subsample of every layer's Abar^S / Abar^T.

    python tests/golden/make_relevance_golden.py
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = os.environ.get('ISTVT_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

import torch  # noqa: E402

import recipe  # noqa: E402

torch.set_num_threads(os.cpu_count() or 1)

# network.vivit.vivit imports network.models_copy, whose third-party imports are absent: a stand-in (DSTTr never uses it)
_stub = types.ModuleType('network.models_copy')
_stub.model_selection = lambda *a, **k: None
sys.modules['network.models_copy'] = _stub
import network.vivit.vivit as ref_vivit  # noqa: E402

DIM, HEADS, DH = 64, 2, 32
GRID = 19
P = GRID * GRID + 1
# row subsample of the stored Abar: spatial query rows [::S_ROWS] of the first and last frame, temporal positions [::T_POS]
S_ROWS, T_POS = 61, 37


class SoftmaxCapture:
    """wraps torch.Tensor.softmax for the duration of a forward: every output is kept (and retains its gradient)"""

    def __init__(self):
        self.outs = []

    def __enter__(self):
        self.orig = torch.Tensor.softmax
        outs = self.outs

        def softmax(t, *args, **kwargs):
            y = self.orig(t, *args, **kwargs)
            y.retain_grad()
            outs.append(y)
            return y
        torch.Tensor.softmax = softmax
        return self

    def __exit__(self, *exc):
        torch.Tensor.softmax = self.orig
        return False


def rollout(outs, F):
    """-> (r_s (B, F, P), r_t (B, P, F), [Abar^S per layer], [Abar^T per layer]) from the captured softmax outputs:
    spatial ones are [B, H, F, P, P], temporal ones [B, H, P, F, F]; the layer order is the call order"""
    sp = [a for a in outs if a.shape[-1] == P and a.shape[2] == F]
    tp = [a for a in outs if a.shape[-1] == F and a.shape[2] == P]
    assert len(sp) == len(tp) == len(outs) // 2, [tuple(a.shape) for a in outs]
    abar_s = [(a.detach() * a.grad).clamp_min(0).mean(dim=1) for a in sp]        # [B, F, P, P]
    abar_t = [(a.detach() * a.grad).clamp_min(0).mean(dim=1) for a in tp]        # [B, P, F, F]
    B = sp[0].shape[0]
    r_s = torch.zeros(B, F, P, dtype=torch.float64)
    r_s[..., 0] = 1
    r_t = torch.zeros(B, P, F, dtype=torch.float64)
    r_t[..., 0] = 1
    for l in reversed(range(len(sp))):
        r_s = r_s + torch.einsum('bfi,bfij->bfj', r_s, abar_s[l])
        r_t = r_t + torch.einsum('bni,bnij->bnj', r_t, abar_t[l])
    return r_s, r_t, abar_s, abar_t


def main():
    out = {}
    for T in (4, 8):
        F = T + 1
        mod = ref_vivit.DSTTr(GRID, 1, 1, T, dim=DIM, depth=2, heads=HEADS, dim_head=DH, in_channels=DIM, scale_dim=2)
        sd = mod.state_dict()
        vals = recipe.fill_state_dict(sd, 'g4.')
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()})
        mod = mod.double().eval()
        x = torch.from_numpy(recipe.input_value('g4.x.T%d' % T, (2, T, DIM, GRID, GRID))).double()
        with SoftmaxCapture() as cap:
            y = mod(x)
        y[:, 0].sum().backward()
        r_s, r_t, abar_s, abar_t = rollout(cap.outs, F)
        tag = 'T%d.' % T
        out[tag + 'logits'] = y.detach().numpy()
        out[tag + 'r_s'] = r_s.numpy()
        out[tag + 'r_t'] = r_t.numpy()
        out[tag + 'cam_s'] = r_s[:, 1:, 1:].numpy()
        out[tag + 'cam_t'] = r_t[:, 1:, 1:].transpose(1, 2).numpy()
        for l, (a_s, a_t) in enumerate(zip(abar_s, abar_t)):
            out[tag + 'abar_s.%d' % l] = a_s[:, [0, F - 1], ::S_ROWS].numpy()
            out[tag + 'abar_t.%d' % l] = a_t[:, ::T_POS].numpy()
    path = os.path.join(HERE, 'G10_relevance.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
