"""Relevance maps (DESIGN.md "Relevance maps"), CPU side: the float64 restatement of gradient-weighted attention rollout
the GPU tests check against, pinned to G10 (captured from the reference's own modules by
tests/golden/make_relevance_golden.py); and host logic that needs no GPU."""
import os
import threading

import numpy as np
import pytest
import torch

import recipe
from oracle import istvt_ref as R

torch.set_num_threads(min(16, os.cpu_count() or 1))
DIM, HEADS, DH, GRID = 64, 2, 32, 19


class SoftmaxCapture:
    """every torch.Tensor.softmax output made inside the block, each retaining its gradient"""

    def __init__(self):
        self.outs = []

    def __enter__(self):
        self.orig = torch.Tensor.softmax
        outs, orig = self.outs, self.orig

        def softmax(t, *args, **kwargs):
            y = orig(t, *args, **kwargs)
            if y.requires_grad:
                y.retain_grad()
            outs.append(y)
            return y
        torch.Tensor.softmax = softmax
        return self

    def __exit__(self, *exc):
        torch.Tensor.softmax = self.orig
        return False


def rollout(outs, F, P):
    """captured softmax outputs (spatial [B, H, F, P, P], temporal [B, H, P, F, F], in layer order) -> r_s (B, F, P),
    r_t (B, P, F), Abar^S and Abar^T per layer"""
    sp = [a for a in outs if a.shape[-1] == P and a.shape[2] == F]
    tp = [a for a in outs if a.shape[-1] == F and a.shape[2] == P]
    assert len(sp) == len(tp) and len(sp) + len(tp) == len(outs), [tuple(a.shape) for a in outs]
    abar_s = [(a.detach() * a.grad).clamp_min(0).mean(dim=1) for a in sp]
    abar_t = [(a.detach() * a.grad).clamp_min(0).mean(dim=1) for a in tp]
    B = sp[0].shape[0]
    r_s = torch.zeros(B, F, P, dtype=torch.float64)
    r_s[..., 0] = 1
    r_t = torch.zeros(B, P, F, dtype=torch.float64)
    r_t[..., 0] = 1
    for l in reversed(range(len(sp))):
        r_s = r_s + torch.einsum('bfi,bfij->bfj', r_s, abar_s[l])
        r_t = r_t + torch.einsum('bni,bnij->bnj', r_t, abar_t[l])
    return r_s, r_t, abar_s, abar_t


def oracle_relevance(fwd, F, P, index=0):
    """fwd() -> logits (a float64 oracle forward); -> (logits, r_s, r_t, abar_s, abar_t) of y = sum_b logits[b, index]"""
    with SoftmaxCapture() as cap:
        y = fwd()
    y[:, index].sum().backward()
    return (y.detach(),) + rollout(cap.outs, F, P)


def relerr(a, b):
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize('T', [4, 8])
def test_rollout_restatement_matches_g10(golden_dir, T):
    g = np.load(os.path.join(golden_dir, 'G10_relevance.npz'))
    F, P = T + 1, GRID * GRID + 1
    shapes = R.dsttr_param_shapes(T, GRID, dim=DIM, depth=2, heads=HEADS, dim_head=DH, scale_dim=2)
    p = {k: torch.from_numpy(recipe.param_value('g4.' + k, s)).double() for k, s in shapes.items()}
    x = torch.from_numpy(recipe.input_value('g4.x.T%d' % T, (2, T, DIM, GRID, GRID))).double().requires_grad_(True)
    logits, r_s, r_t, abar_s, abar_t = oracle_relevance(lambda: R.dsttr_forward(p, x, depth=2, heads=HEADS), F, P)
    tag = 'T%d.' % T
    assert relerr(logits, g[tag + 'logits']) < 1e-9
    assert relerr(r_s, g[tag + 'r_s']) < 1e-9
    assert relerr(r_t, g[tag + 'r_t']) < 1e-9
    assert relerr(r_s[:, 1:, 1:], g[tag + 'cam_s']) < 1e-9
    assert relerr(r_t[:, 1:, 1:].transpose(1, 2), g[tag + 'cam_t']) < 1e-9
    for l in range(2):
        assert relerr(abar_s[l][:, [0, F - 1], ::61], g[tag + 'abar_s.%d' % l]) < 1e-9
        assert relerr(abar_t[l][:, ::37], g[tag + 'abar_t.%d' % l]) < 1e-9


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _small_dsttr():
    from istvt_amd.network.vivit.vivit import DSTTr
    return DSTTr(4, 1, 1, 2, dim=64, depth=1, heads=2, dim_head=32, in_channels=64, scale_dim=2)


def test_relevance_restores_flags_after_an_error(pkg):
    from istvt_amd import explain, functional as Fn
    m = _small_dsttr()
    m.train()
    m.mlp_head.eval()                                   # a mixed state comes back as it was
    attn = [mod for mod in m.modules() if hasattr(mod, 'attn_fp8')]
    assert attn
    for mod in attn:
        mod.attn_fp8 = True
    m.space_token.requires_grad_(False)
    modes = {n: mod.training for n, mod in m.named_modules()}
    req = {n: q.requires_grad for n, q in m.named_parameters()}
    feats = torch.randn(1, 2, 16, 64)                   # CPU features: the HIP path refuses them inside the call
    with pytest.raises(RuntimeError):
        explain.relevance_features(m, feats)
    assert {n: mod.training for n, mod in m.named_modules()} == modes
    assert {n: q.requires_grad for n, q in m.named_parameters()} == req
    assert all(mod.attn_fp8 for mod in attn)
    assert Fn.relevance_context() is None
    assert all(q.grad is None for q in m.parameters())


def test_relevance_rejects_other_models(pkg):
    from istvt_amd import explain
    with pytest.raises(TypeError):
        explain.relevance(torch.nn.Linear(2, 2), torch.zeros(1, 2))


def test_relevance_mode_is_thread_local_and_nests(pkg):
    from istvt_amd import functional as Fn
    seen = []
    a, b = object(), object()
    with Fn.relevance_mode(a):
        assert Fn.relevance_context() is a
        t = threading.Thread(target=lambda: seen.append(Fn.relevance_context()))
        t.start()
        t.join()
        with Fn.relevance_mode(b):
            assert Fn.relevance_context() is b
        assert Fn.relevance_context() is a
    assert Fn.relevance_context() is None
    assert seen == [None]


def test_heatmaps_host_checks(pkg):
    from istvt_amd import explain
    with pytest.raises(RuntimeError, match='square'):
        explain.heatmaps(torch.zeros(1, 2, 10))
    with pytest.raises(RuntimeError):
        explain.heatmaps(torch.zeros(1, 2, 4, 4))       # CPU tensor: no CPU path


def test_result_views(pkg):
    from istvt_amd.explain import Relevance
    B, F, P = 2, 3, 5
    r_s = torch.arange(B * F * P, dtype=torch.float32).view(B, F, P)
    r_t = torch.arange(B * P * F, dtype=torch.float32).view(B, P, F) + 1000
    res = Relevance(r_s, r_t, torch.zeros(B, 1))
    for b in range(B):
        for t in range(F - 1):
            for n in range(1, P):
                assert res.cam_s[b, t, n - 1] == r_s[b, t + 1, n]
                assert res.cam_t[b, t, n - 1] == r_t[b, n, t + 1]
