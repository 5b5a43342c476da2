"""Explaining whole videos (DESIGN.md "Explaining whole videos") on a real MI355X: the fuse and overlay kernels against
float64 restatements, VideoScorer.explain against the clip-level relevance path, the float64 oracle and its own score(),
and the promise that the call leaves the model, a training run and a stream in progress as it found them."""
import pytest
import torch

import recipe
from test_relevance_cpu import oracle_relevance
from test_relevance_gpu import _cos_per_map, _native, BF16_MAP_COS_FLOOR
from test_video_explain_cpu import fuse_ref
from test_video_gpu import _video, _windows, pkg, relerr, small  # noqa: F401  (pkg, small: fixtures)

pytestmark = pytest.mark.gpu


# ---- the fuse kernel --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', [6, 14, 19])
@pytest.mark.parametrize('T', [4, 8, 16])
def test_fuse_kernel_vs_float64(pkg, T, g):
    from istvt_amd import ops, video
    P, F, n = g * g + 1, T + 1, 3 * T + 5
    gen = torch.Generator().manual_seed(100 * T + g)
    for stride, tail in ((1, True), (3, True), (T, False), (T + 3, True), (T + 3, False)):
        starts = video.window_starts(n, T, stride, tail)
        W = len(starts)
        r_s, r_t = torch.rand((W, F, P), generator=gen), torch.rand((W, P, F), generator=gen)
        logits = torch.randn((W, 2), generator=gen)
        out = ops.relevance_fuse_windows(r_s.cuda(), r_t.cuda(), logits.cuda(), starts, n, index=1)
        again = ops.relevance_fuse_windows(r_s.cuda(), r_t.cuda(), logits.cuda(), torch.tensor(starts), n, index=1)
        ref = fuse_ref(r_s, r_t, logits, starts, n, index=1)
        errs = [relerr(o, r) for o, r in zip(out[:4], ref[:4])]
        print('fuse T=%d g=%d stride=%d tail=%s W=%d: relerr frame_s %.2e frame_t %.2e weight %.2e logit %.2e'
              % (T, g, stride, tail, W, *errs))
        assert max(errs) <= 1e-6
        assert out[4].dtype == torch.int32 and torch.equal(out[4].cpu(), ref[4])
        empty = ref[4] == 0
        assert bool(empty.any()) or stride <= T             # a stride larger than T leaves frames uncovered
        for o in out[:4]:
            assert float(o.cpu()[empty].abs().sum()) == 0.0
        assert all(torch.equal(a, b) for a, b in zip(out, again))
    with pytest.raises(ValueError):
        ops.relevance_fuse_windows(r_s.cuda(), r_t.cuda(), logits.cuda(), starts[::-1], n)
    with pytest.raises(ValueError):
        ops.relevance_fuse_windows(r_s.cuda(), r_t.cuda(), logits.cuda(), [s + n for s in starts], n)
    with pytest.raises(IndexError):
        ops.relevance_fuse_windows(r_s.cuda(), r_t.cuda(), logits.cuda(), starts, n, index=2)


# ---- the overlay kernel -----------------------------------------------------------------------------------------------
def _overlay_ref(frames, maps, lut, scale):
    """float64 on the CPU -> (bytes with k = floor(255 m), bytes with k = round(255 m) - 1, bytes with k = round(255 m),
    mask of the index-ambiguous pixels: 255 m within 1e-3 of an integer).  The frame's maximum is the first rendering's."""
    Fi = torch.nn.functional.interpolate
    N, S, g = frames.shape[0], frames.shape[1], maps.shape[-1]
    So = g * scale
    up = Fi(maps.double().view(N, 1, g, g), scale_factor=scale, mode='bilinear', align_corners=False)[:, 0]
    mn, mx = up.amin(dim=(1, 2), keepdim=True), up.amax(dim=(1, 2), keepdim=True)
    km = 255 * (up - mn) / (mx - mn)
    near = km.round()
    amb = (km - near).abs() < 1e-3
    img = frames.double() / 255
    if So != S:
        img = Fi(img.permute(0, 3, 1, 2), size=(So, So), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    table = lut.double() / 255

    def cam(k):
        return table[k.long().clamp(0, 255)] + img
    base = cam(km.floor())
    top = base.amax(dim=(1, 2, 3), keepdim=True)
    return tuple((255 * c / top).floor().clamp(max=255) for c in (base, cam(near - 1), cam(near))) + (amb,)


def _check_overlay(out, frames, maps, lut, scale, what, share=0.02):
    base, lo, hi, amb = _overlay_ref(frames, maps, lut, scale)
    o = out.cpu().double()
    d = (o - base).abs()
    clear = ~amb
    worst = float(d[clear].max())
    d_amb = torch.minimum((o - lo).abs(), (o - hi).abs())[amb]
    worst_amb = float(d_amb.max()) if d_amb.numel() else 0.0
    frac = float(amb.double().mean())
    print('overlay %s: max byte difference %.0f (clear pixels), %.0f (ambiguous, best neighbour), ambiguous share %.4f, '
          'bytes equal %.4f' % (what, worst, worst_amb, frac, float((d == 0).double().mean())))
    assert worst <= 1
    assert worst_amb <= 1
    if share is not None:
        assert frac <= share


@pytest.mark.parametrize('g,S', [(6, 96), (14, 224), (19, 304), (19, 300)])
def test_overlay_kernel_vs_float64(pkg, g, S):
    from istvt_amd import explain
    gen = torch.Generator().manual_seed(g)
    N = 3
    maps = torch.rand((N, g, g), generator=gen)
    frames = torch.randint(0, 256, (N, S, S, 3), generator=gen, dtype=torch.uint8)
    lut = explain.jet_lut()
    out = explain.overlay(frames.cuda(), maps.cuda(), scale=16)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (N, g * 16, g * 16, 3)
    _check_overlay(out, frames, maps, lut, 16, 'g=%d S=%d' % (g, S))
    assert torch.equal(out, explain.overlay(frames.cuda(), maps.cuda().view(N, g * g), scale=16, lut=lut.cuda()))
    # a custom table (the columns swapped: BGR frames)
    swapped = lut[:, [2, 1, 0]].contiguous()
    _check_overlay(explain.overlay(frames.cuda(), maps.cuda(), lut=swapped.cuda()), frames, maps, swapped, 16,
                   'g=%d S=%d swapped table' % (g, S))
    # a non-contiguous view of a frame batch gives the bytes of its contiguous copy; so does a view at an odd byte offset
    wide = torch.randint(0, 256, (N, S, S + 8, 3), generator=gen, dtype=torch.uint8).cuda()
    view = wide[:, :, 3:3 + S]
    assert not view.is_contiguous()
    assert torch.equal(explain.overlay(view, maps.cuda()), explain.overlay(view.contiguous(), maps.cuda()))
    flat = torch.empty((N * S * S * 3 + 1,), dtype=torch.uint8, device='cuda')
    odd = flat[1:].view(N, S, S, 3)
    odd.copy_(frames)
    assert odd.is_contiguous() and odd.data_ptr() % 2 == 1
    assert torch.equal(explain.overlay(odd, maps.cuda()), out)


def test_overlay_kernel_unaligned_size(pkg):
    """18 x 18 output (scale 3): a pixel count that is no multiple of a thread's 16 pixels, every access bytewise.  The
    byte rule of the cases above; the share of ambiguous pixels is not bounded here (324 pixels per frame)."""
    from istvt_amd import explain
    gen = torch.Generator().manual_seed(3)
    maps = torch.rand((5, 6, 6), generator=gen)
    lut = explain.jet_lut()
    for S in (18, 25):
        frames = torch.randint(0, 256, (5, S, S, 3), generator=gen, dtype=torch.uint8)
        out = explain.overlay(frames.cuda(), maps.cuda(), scale=3)
        assert tuple(out.shape) == (5, 18, 18, 3)
        _check_overlay(out, frames, maps, lut, 3, 'g=6 scale=3 S=%d' % S, share=None)


def test_overlay_refusals(pkg):
    from istvt_amd import explain
    frames = torch.zeros((2, 96, 96, 3), dtype=torch.uint8, device='cuda')
    maps = torch.rand((2, 6, 6)).cuda()
    with pytest.raises(RuntimeError, match='lut'):
        explain.overlay(frames, maps, lut=torch.zeros((256, 4), dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError, match='lut'):
        explain.overlay(frames, maps, lut=torch.zeros((256, 3), dtype=torch.float32, device='cuda'))
    with pytest.raises(RuntimeError, match='maps for'):
        explain.overlay(frames, maps[:1])
    with pytest.raises(RuntimeError):
        explain.overlay(frames.float(), maps)
    with pytest.raises(RuntimeError, match='square'):
        explain.overlay(frames, torch.rand((2, 35)).cuda())


# ---- the scorer's explain() -------------------------------------------------------------------------------------------
def _fields(ex):
    return dict(frame_s=ex.frame_s, frame_t=ex.frame_t, frame_weight=ex.frame_weight, frame_logit=ex.frame_logit)


@pytest.mark.parametrize('stride', [1, 3])
def test_window_maps(small, stride):
    from istvt_amd import explain, video
    model, u8, xn = small['model'], small['u8'], small['xn']
    T, n = 4, 11
    starts = video.window_starts(n, T, stride, True)
    scorer = video.VideoScorer(model, stride=stride)
    ex = scorer.explain(u8)
    assert model.training
    W = len(starts)
    assert ex.score.starts.tolist() == starts
    assert tuple(ex.windows.cam_s.shape) == tuple(ex.windows.cam_t.shape) == (W, T, 36)
    assert tuple(ex.frame_s.shape) == tuple(ex.frame_t.shape) == (n, 36) and ex.frame_s.dtype == torch.float32
    assert tuple(ex.frame_weight.shape) == tuple(ex.frame_logit.shape) == tuple(ex.count.shape) == (n,)
    assert torch.equal(model.explain_video(u8, stride=stride).frame_s, ex.frame_s)
    # the same windows gathered from the scorer's own stem pass, all in one batch on both sides: the same bits
    with video._eval_mode(model), torch.no_grad():
        feats = scorer._stem(u8, 'u8', torch.device('cuda', torch.cuda.current_device()))
    idx = torch.tensor([[s + t for t in range(T)] for s in starts]).cuda()
    ref = explain.relevance_features(model.vit, feats[idx])
    for k in ('cam_s', 'cam_t', 'r_s', 'r_t', 'logits'):
        same = torch.equal(getattr(ex.windows, k), getattr(ref, k))
        print('stride %d %s: bits equal to relevance_features on the gathered windows: %s (relerr %.3e)'
              % (stride, k, same, relerr(getattr(ex.windows, k), getattr(ref, k))))
        assert same, k
    # batches of two windows against one batch
    ex2 = video.VideoScorer(model, stride=stride, window_batch=2).explain(u8)
    for k in ('cam_s', 'cam_t'):
        e = relerr(getattr(ex2.windows, k), getattr(ex.windows, k))
        print('stride %d %s: window_batch=2 vs one batch relerr %.3e' % (stride, k, e))
        assert e <= 1e-5
    # the clip path on the host-normalised float windows (conv1 through im2col in float32)
    clip = model.relevance(_windows(xn, starts, T).cuda())
    for k in ('cam_s', 'cam_t'):
        e = relerr(getattr(ex.windows, k), getattr(clip, k))
        print('stride %d %s: vs model.relevance(windows) relerr %.3e' % (stride, k, e))
        assert e <= 1e-3


@pytest.mark.parametrize('stride', [1, 3])
def test_score_field_and_fused_maps(small, stride):
    from istvt_amd import video
    model, u8, xn = small['model'], small['u8'], small['xn']
    scorer = video.VideoScorer(model, stride=stride)
    ex, sc = scorer.explain(u8), scorer.score(u8)
    e = relerr(ex.score.window_logits, sc.window_logits)
    print('stride %d: explain().score.window_logits vs score(): relerr %.3e, bits equal: %s'
          % (stride, e, torch.equal(ex.score.window_logits, sc.window_logits)))
    assert e <= 1e-5
    assert torch.equal(ex.score.starts, sc.starts)
    assert relerr(ex.score.logit_mean, sc.logit_mean) <= 1e-5 and relerr(ex.score.prob_mean, sc.prob_mean) <= 1e-5
    ref = fuse_ref(ex.windows.r_s, ex.windows.r_t, ex.score.window_logits, ex.score.starts.tolist(), 11)
    for (k, v), r in zip(_fields(ex).items(), ref[:4]):
        e = relerr(v, r)
        print('stride %d %s: vs the float64 fusion of the call\'s own windows relerr %.3e' % (stride, k, e))
        assert e <= 1e-6
    assert torch.equal(ex.count.cpu(), ref[4]) and int(ex.count.min()) >= 1
    exf = scorer.explain(xn)                                  # the normalised float frames: the same bits
    for k, v in _fields(ex).items():
        assert torch.equal(v, _fields(exf)[k]), k
    assert torch.equal(ex.count, exf.count) and torch.equal(ex.windows.r_s, exf.windows.r_s)
    assert torch.equal(ex.score.window_logits, exf.score.window_logits)
    again = scorer.explain(u8.cuda())                         # device frames, a second run: the same bits
    for k, v in _fields(ex).items():
        assert torch.equal(v, _fields(again)[k]), k


def test_uncovered_frames(small):
    from istvt_amd import video
    ex = video.VideoScorer(small['model'], stride=6, cover_tail=False).explain(small['u8'])
    assert ex.score.starts.tolist() == [0, 6] and ex.count.tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0]
    dead = ex.count == 0
    for v in _fields(ex).values():
        assert float(v[dead].abs().sum()) == 0.0 and torch.isfinite(v).all()
    assert float(ex.frame_weight[~dead].min()) >= 0


def _native_video(n):
    """n correlated 300 x 300 frames as bytes; with mean 0.5 and std 1/6 the normalised values are the recipe's, clipped
    at 3 sigma and rounded to a byte"""
    x = torch.from_numpy(recipe.correlated_frames('g5c.x', (1, n, 3, 300, 300)))[0]
    u8 = (127.5 + 127.5 * x / 3).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return u8, dict(mean=(0.5, 0.5, 0.5), std=(1 / 6, 1 / 6, 1 / 6))


def test_native_fused_maps_vs_oracle(pkg):
    from oracle import istvt_ref as R
    from istvt_amd import video
    T, n = 6, 9
    model, _ = _native(2, 1)
    u8, norm = _native_video(n)
    ex = video.VideoScorer(model, stride=1, **norm).explain(u8)
    assert model.training and ex.score.starts.tolist() == [0, 1, 2, 3]
    p = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    xn = ((u8.double() / 255 - 0.5) * 6).permute(0, 3, 1, 2)
    with torch.no_grad():
        f = R.stem_forward(p, xn, 'xcep.model.', training=False)
    starts = [0, 1, 2, 3]
    r_s, r_t, logits = [], [], []
    for s in starts:                                          # window by window
        fw = f[s:s + T].unsqueeze(0).clone().requires_grad_(True)
        lg, rs, rt, _, _ = oracle_relevance(lambda: R.dsttr_forward(p, fw, 'vit.', depth=2, heads=8), 7, 362)
        r_s.append(torch.as_tensor(rs)), r_t.append(torch.as_tensor(rt)), logits.append(torch.as_tensor(lg))
    r_s, r_t, logits = torch.cat(r_s), torch.cat(r_t), torch.cat(logits)
    ref = fuse_ref(r_s, r_t, logits, starts, n)
    errs = {k: relerr(v, r) for (k, v), r in zip(_fields(ex).items(), ref[:4])}
    errs['window_logits'] = relerr(ex.score.window_logits, logits)
    print('native fused maps vs the float64 oracle:', errs)
    assert max(errs.values()) <= 1e-3, errs
    assert torch.equal(ex.count.cpu(), ref[4])


def test_bf16_fused_maps_track_fp32(pkg):
    from istvt_amd import video
    model, _ = _native(2, 1)
    u8, norm = _native_video(9)
    ex32 = video.VideoScorer(model, **norm).explain(u8)
    model.set_compute_dtype(torch.bfloat16)
    ex16 = video.VideoScorer(model, **norm).explain(u8)
    cs = _cos_per_map(ex16.frame_s[None], ex32.frame_s[None])
    ct = _cos_per_map(ex16.frame_t[None], ex32.frame_t[None])
    print('bf16 vs fp32 fused maps, per-map cosine: spatial min %.5f, temporal min %.5f' % (float(cs.min()), float(ct.min())))
    assert float(cs.min()) >= BF16_MAP_COS_FLOOR and float(ct.min()) >= BF16_MAP_COS_FLOOR


# ---- no side effects --------------------------------------------------------------------------------------------------
def test_explain_leaves_the_model_alone(small):
    from istvt_amd import video
    model, u8 = small['model'], small['u8']
    model.train()
    model.vit.mlp_head.eval()                                 # a mixed set of flags must come back as it was
    frozen = next(model.vit.parameters())
    frozen.requires_grad_(False)
    try:
        flags = [m.training for m in model.modules()]
        req = [p.requires_grad for p in model.parameters()]
        fp8 = [m.attn_fp8 for m in model.modules() if hasattr(m, 'attn_fp8')]
        grads = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
        before = {k: v.clone() for k, v in model.state_dict().items()}
        assert any('num_batches_tracked' in k for k in before) and any('running_var' in k for k in before)
        ex = video.VideoScorer(model).explain(u8)
        after = model.state_dict()
        assert set(after) == set(before) and all(torch.equal(after[k], v) for k, v in before.items())
        assert [m.training for m in model.modules()] == flags
        assert [p.requires_grad for p in model.parameters()] == req
        assert [m.attn_fp8 for m in model.modules() if hasattr(m, 'attn_fp8')] == fp8
        for p, g0 in zip(model.parameters(), grads):
            assert (p.grad is None) if g0 is None else torch.equal(p.grad, g0)
        assert not ex.frame_s.requires_grad and not ex.windows.r_s.requires_grad and not ex.score.window_logits.requires_grad
        with pytest.raises(IndexError):                       # an error inside the call restores everything too
            video.VideoScorer(model).explain(u8, index=1)
        assert [m.training for m in model.modules()] == flags
        assert [p.requires_grad for p in model.parameters()] == req
    finally:
        frozen.requires_grad_(True)
        model.vit.mlp_head.train()


@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphs'])
def test_explain_call_leaves_training_untouched(pkg, graphs):
    """the protocol of test_relevance_call_leaves_training_untouched with explain_video(frames) in the middle"""
    from istvt_amd import parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    T, side, B = 4, 96, 2
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn((B, T, 3, side, side), generator=g).cuda() for _ in range(2)]
    ys = [(torch.rand((B,), generator=g) > 0.5).float().cuda() for _ in range(2)]
    u8 = _video(7, side, 3)
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
                ex = model.explain_video(u8, stride=2)
                torch.cuda.synchronize()
                assert all(torch.isfinite(v).all() for v in _fields(ex).values())
                assert all(torch.equal(p.grad, g0) for p, g0 in zip(live, grads))
                assert all(m.attn_fp8 for m in model.modules() if hasattr(m, 'attn_fp8'))
                assert all(p.requires_grad for p in live)
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
        runs.append((logits.detach().clone(), bucket.flat_params.detach().clone(), state, opt.momentum_buffer.clone()))
        if graphs:
            model.enable_step_graphs(False)
    (la, pa, sa, oa), (lb, pb, sb, ob) = runs
    assert torch.equal(la, lb)
    assert torch.equal(pa, pb)
    for k, v in sa.items():                                   # parameters, BatchNorm buffers and counters
        assert torch.equal(v, sb[k]), k
    assert torch.equal(oa, ob)


def test_explain_does_not_disturb_a_stream(small):
    from istvt_amd import video
    model, u8 = small['model'], small['u8']
    outs = []
    for call in (False, True):
        scorer = video.VideoScorer(model, stride=3, frame_batch=4, window_batch=3, capacity=9)
        l1, s1 = scorer.push(u8[:6])
        if call:
            ex = scorer.explain(u8)
            assert ex.score.starts.tolist() == [0, 3, 6, 7]
        l2, s2 = scorer.push(u8[6:])
        l3, s3 = scorer.flush()
        outs.append((torch.cat([l1, l2, l3]), torch.cat([s1, s2, s3])))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][1].tolist() == [0, 3, 6, 7]


def test_explain_refusals(small):
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model, u8 = small['model'], small['u8']
    with pytest.raises(ValueError, match='shorter'):
        video.VideoScorer(model).explain(u8[:3])
    with pytest.raises(ValueError):
        video.VideoScorer(model).explain(u8.float())
    cpu = XceptionVidTr(num_frames=4, grid=6, depth=1)
    with pytest.raises(RuntimeError, match='ROCm device'):
        cpu.explain_video(u8)
    assert model.training
