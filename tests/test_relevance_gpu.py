"""Relevance maps (DESIGN.md "Relevance maps") on a real MI355X: the two rollout kernels and the heat-map kernel against
float64 restatements, the model-level maps against G10 and the float64 oracle, and the guarantee that a relevance()
call leaves a training run bit for bit as it was."""
import os

import numpy as np
import pytest
import torch

import recipe
from test_relevance_cpu import oracle_relevance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def relerr(a, b):
    a = torch.as_tensor(a.detach().cpu() if torch.is_tensor(a) else np.asarray(a), dtype=torch.float64)
    b = torch.as_tensor(b.detach().cpu() if torch.is_tensor(b) else np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# one rounding of a bfloat16 operand (what the attention checks allow a bf16 result against a restatement on the same
# bf16 inputs); float32: 1e-4
TOL = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -8}


def _rand(shape, g, dtype, scale=1.0):
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).cuda()


# ---- kernels ---------------------------------------------------------------------------------------------------------
def _spatial_ref(qkv, dout, r, BF, P, heads, dh):
    """float64: r + (1/H) sum_h r E_h per frame, A recomputed in full (softmax of q k^T / sqrt(dh))"""
    inner = heads * dh
    q, k, v = (qkv[:, i * inner:(i + 1) * inner].double().view(BF, P, heads, dh).transpose(1, 2) for i in range(3))
    do = dout.double().view(BF, P, heads, dh).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
    e = (a * (do @ v.transpose(-1, -2))).clamp_min(0)                 # [BF, H, P, P]
    rr = r.double()
    return rr + torch.einsum('fi,fhij->fj', rr, e) / heads


# every (P, heads, dh) on one frame; the 288-frame batch (C2: 32 clips x 9 frames) at the C2 head shape and one other
SPATIAL_CASES = [(P, h, d, 1) for P in (50, 197, 362) for h in (2, 8) for d in (32, 64)] + \
    [(P, 8, 64, 288) for P in (50, 197, 362)] + [(197, 2, 32, 288)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('P,heads,dh,BF', SPATIAL_CASES)
def test_spatial_relevance_kernel(pkg, P, heads, dh, BF, dtype):
    from istvt_amd import ops
    g = torch.Generator().manual_seed(P * 100 + heads * 10 + dh + BF)
    inner = heads * dh
    qkv = ops.empty_rows(BF * P, 3 * inner, dtype, 'cuda')            # the forward's row-strided layout
    qkv.copy_(_rand((BF * P, 3 * inner), g, dtype, 0.6))
    dout = _rand((BF * P, inner), g, dtype)
    r = torch.rand((BF, P), generator=g).cuda()
    r[:, 0] += 1.0
    _, lse = ops.attn_spatial_fwd(qkv, BF, P, heads, dh)
    out = ops.attn_spatial_relevance(qkv, dout, lse, r, BF, P, heads, dh)
    ref = _spatial_ref(qkv, dout, r, BF, P, heads, dh)
    err = float((out.double() - ref).norm() / ref.norm())
    inc = float(((out.double() - r.double()) - (ref - r.double())).norm() / (ref - r.double()).norm())
    print('spatial P=%d H=%d dh=%d BF=%d %s: %.2e of |r_out|, %.2e of the increment' % (P, heads, dh, BF, dtype, err, inc))
    assert err <= TOL[dtype]
    assert inc <= 10 * TOL[dtype]
    again = ops.attn_spatial_relevance(qkv, dout, lse, r, BF, P, heads, dh)
    assert torch.equal(out, again)


def _temporal_ref(qkv, dout, r, B, F, P, heads, dh, diff):
    inner = heads * dh

    def split(t):                                                     # rows (b, f, n) -> [B, P, H, F, dh]
        return t.double().view(B, F, P, heads, dh).permute(0, 2, 3, 1, 4)
    q, k, v = (split(qkv[:, i * inner:(i + 1) * inner]) for i in range(3))
    if diff == 1:
        q = torch.cat((q[..., :2, :], q[..., 2:, :] - q[..., 1:-1, :]), dim=-2)
        k = torch.cat((k[..., :2, :], k[..., 2:, :] - k[..., 1:-1, :]), dim=-2)
    do = split(dout)
    a = torch.softmax(q @ k.transpose(-1, -2) * dh ** -0.5, dim=-1)
    e = (a * (do @ v.transpose(-1, -2))).clamp_min(0)                 # [B, P, H, F, F]
    rr = r.double().view(B, P, F)
    return (rr + torch.einsum('bni,bnhij->bnj', rr, e) / heads).view(B * P, F)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('diff', [0, 1, 2])
@pytest.mark.parametrize('F', [5, 7, 9, 17])
def test_temporal_relevance_kernel(pkg, F, diff, dtype):
    from istvt_amd import ops
    g = torch.Generator().manual_seed(F * 10 + diff)
    for (B, P, heads, dh) in ((2, 50, 2, 32), (3, 197, 8, 64)):
        inner = heads * dh
        M = B * F * P
        qkv = ops.empty_rows(M, 3 * inner, dtype, 'cuda')
        qkv.copy_(_rand((M, 3 * inner), g, dtype, 0.6))
        dout = _rand((M, inner), g, dtype)
        r = torch.rand((B * P, F), generator=g).cuda()
        r[:, 0] += 1.0
        out = ops.attn_temporal_relevance(qkv, dout, r, B, F, P, heads, dh, diff)
        ref = _temporal_ref(qkv, dout, r, B, F, P, heads, dh, diff)
        err = float((out.double() - ref).norm() / ref.norm())
        inc = float(((out.double() - r.double()) - (ref - r.double())).norm() / (ref - r.double()).norm())
        print('temporal F=%d diff=%d H=%d dh=%d %s: %.2e of |r_out|, %.2e of the increment' % (F, diff, heads, dh, dtype, err, inc))
        assert err <= TOL[dtype]
        assert inc <= 10 * TOL[dtype]
        assert torch.equal(out, ops.attn_temporal_relevance(qkv, dout, r, B, F, P, heads, dh, diff))


@pytest.mark.parametrize('g_in', [19, 14])
def test_heatmaps_match_interpolate_and_min_max(pkg, g_in):
    from istvt_amd import explain
    cam = torch.rand((2, 3, g_in, g_in), generator=torch.Generator().manual_seed(g_in), dtype=torch.float32) ** 3
    out = explain.heatmaps(cam.cuda(), scale=16).cpu()
    up = torch.nn.functional.interpolate(cam.view(-1, 1, g_in, g_in), scale_factor=16, mode='bilinear', align_corners=False)
    up = up.view(2, 3, g_in * 16, g_in * 16)
    mn = up.amin(dim=(-1, -2), keepdim=True)
    mx = up.amax(dim=(-1, -2), keepdim=True)
    ref = (up - mn) / (mx - mn)
    assert out.shape == (2, 3, g_in * 16, g_in * 16)
    assert float((out - ref).abs().max()) <= 1e-6
    flat = explain.heatmaps(cam.view(2, 3, -1).cuda(), scale=16).cpu()          # the (B, T, g*g) form of cam_s / cam_t
    assert torch.equal(flat, out)


# ---- model ----------------------------------------------------------------------------------------------------------
DIM, HEADS, DH, GRID = 64, 2, 32, 19


def _g4_dsttr(T, dtype=torch.float32):
    from istvt_amd.network.vivit.vivit import DSTTr
    m = DSTTr(GRID, 1, 1, T, dim=DIM, depth=2, heads=HEADS, dim_head=DH, in_channels=DIM, scale_dim=2, compute_dtype=dtype)
    sd = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in recipe.fill_state_dict(sd, 'g4.').items()})
    x = torch.from_numpy(recipe.input_value('g4.x.T%d' % T, (2, T, DIM, GRID, GRID)))
    feats = x.flatten(3).transpose(2, 3).contiguous()                 # (b, t, hw, c)
    return m.cuda(), feats.cuda()


@pytest.mark.parametrize('T', [4, 8])
def test_dsttr_relevance_matches_g10(pkg, golden_dir, T):
    g = np.load(os.path.join(golden_dir, 'G10_relevance.npz'))
    m, feats = _g4_dsttr(T)
    res = m.relevance_features(feats, index=0)
    tag = 'T%d.' % T
    errs = {k: relerr(getattr(res, k), g[tag + k]) for k in ('cam_s', 'cam_t', 'r_s', 'r_t', 'logits')}
    print('G10 T=%d' % T, errs)
    assert max(errs.values()) <= 1e-3, errs
    # dead-row elimination skips the last layer's frames 1..T (their dA is 0): identical maps
    m.transformer.dead_row_elimination = True
    res2 = m.relevance_features(feats, index=0)
    for k in ('r_s', 'r_t', 'logits'):
        assert torch.equal(getattr(res, k), getattr(res2, k)), k
    # each clip of the batch is the clip run alone
    solo = m.relevance_features(feats[1:2], index=0)
    for k in ('r_s', 'r_t'):
        assert relerr(getattr(solo, k)[0], getattr(res, k)[1]) <= 1e-5, k


def _native(depth, B, dtype=torch.float32):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=6, grid=19, depth=depth, compute_dtype=dtype)
    sd = model.state_dict()
    model.load_state_dict({k: torch.from_numpy(recipe.cond_param_value(k, tuple(v.shape))) for k, v in sd.items()})
    x = torch.from_numpy(recipe.correlated_frames('g5c.x', (B, 6, 3, 300, 300)))
    return model.cuda().train(), x


@pytest.mark.parametrize('depth,B', [(2, 2), (12, 1)])
def test_native_relevance_vs_oracle(pkg, depth, B):
    from oracle import istvt_ref as R
    model, x = _native(depth, B)
    res = model.relevance(x.cuda(), index=0)
    assert model.training                                             # the mode came back
    p = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    with torch.no_grad():
        f = R.stem_forward(p, x.double().flatten(0, 1), 'xcep.model.', training=False)
    f = f.view(B, 6, *f.shape[1:]).requires_grad_(True)
    logits, r_s, r_t, _, _ = oracle_relevance(lambda: R.dsttr_forward(p, f, 'vit.', depth=depth, heads=8), 7, 362)
    errs = {'logits': relerr(res.logits, logits), 'r_s': relerr(res.r_s, r_s), 'r_t': relerr(res.r_t, r_t),
            'cam_s': relerr(res.cam_s, r_s[:, 1:, 1:]), 'cam_t': relerr(res.cam_t, r_t[:, 1:, 1:].transpose(1, 2))}
    print('native depth=%d B=%d' % (depth, B), errs)
    assert max(errs.values()) <= 1e-3, errs


def _cos_per_map(a, b):
    a, b = a.double().flatten(2), b.double().flatten(2)
    return (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


# Per-map cosine of the bfloat16 model's maps against the float32 model's, native geometry, depth 2, G5c-conditioned
# input.  Measured on MI355X: worst spatial map 0.99934, worst temporal map 0.99999.  The floor allows 15x the measured
# worst deficit (1 - 0.99934 = 6.6e-4).
BF16_MAP_COS_FLOOR = 0.99


def test_bf16_maps_track_fp32(pkg):
    model, x = _native(2, 2)
    res32 = model.relevance(x.cuda())
    model.set_compute_dtype(torch.bfloat16)
    res16 = model.relevance(x.cuda())
    cs, ct = _cos_per_map(res16.cam_s, res32.cam_s), _cos_per_map(res16.cam_t, res32.cam_t)
    print('bf16 vs fp32 per-map cosine: spatial min %.5f, temporal min %.5f' % (float(cs.min()), float(ct.min())))
    assert float(cs.min()) >= BF16_MAP_COS_FLOOR and float(ct.min()) >= BF16_MAP_COS_FLOOR


# ---- no side effects ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphs'])
def test_relevance_call_leaves_training_untouched(pkg, graphs):
    from istvt_amd import parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    T, side, B = 4, 96, 2
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn((B, T, 3, side, side), generator=g).cuda() for _ in range(2)]
    ys = [(torch.rand((B,), generator=g) > 0.5).float().cuda() for _ in range(2)]
    runs = []
    for call in (False, True):
        torch.manual_seed(5)
        model = XceptionVidTr(num_frames=T, grid=6, depth=2, compute_dtype=torch.bfloat16).cuda().train()
        live = [p for _, p in parallel.live_named_parameters(model)]
        bucket = parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
        opt = parallel.FusedSGD(bucket, lr=1e-2, momentum=0.9, zero_grad=True)
        if graphs:
            model.enable_step_graphs(True, warmup=1)
        logits = None
        for i in range(4):
            if i == 2 and call:
                model.set_attn_fp8(True)
                keys = set(model._step_graphs.entries) if graphs else None
                stats = dict(model._step_graphs.stats) if graphs else None
                grads = [p.grad.clone() for p in live]
                res = model.relevance(xs[0])
                torch.cuda.synchronize()
                assert torch.isfinite(res.r_s).all() and torch.isfinite(res.r_t).all()
                assert all(torch.equal(p.grad, g0) for p, g0 in zip(live, grads))
                assert all(m.attn_fp8 for m in model.modules() if hasattr(m, 'attn_fp8'))
                model.set_attn_fp8(False)
                assert model.training
                if graphs:
                    assert set(model._step_graphs.entries) == keys and model._step_graphs.stats == stats
            opt.zero_grad()
            logits = model(xs[i % 2])
            torch.nn.functional.binary_cross_entropy_with_logits(logits.view(-1), ys[i % 2]).backward()
            opt.step()
        torch.cuda.synchronize()
        if graphs:
            st = model._step_graphs.stats
            assert st['recaptures'] == 0, st
        state = {k: v.clone() for k, v in model.state_dict().items()}
        opt_state = [opt.momentum_buffer.clone()]
        runs.append((logits.detach().clone(), bucket.flat_params.detach().clone(), state, opt_state))
        if graphs:
            model.enable_step_graphs(False)
    (la, pa, sa, oa), (lb, pb, sb, ob) = runs
    assert torch.equal(la, lb)
    assert torch.equal(pa, pb)
    for k, v in sa.items():                                           # parameters, BatchNorm buffers and counters
        assert torch.equal(v, sb[k]), k
    assert len(oa) == len(ob) and all(torch.equal(a, b) for a, b in zip(oa, ob))
