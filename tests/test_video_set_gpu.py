"""Scoring a set of videos (DESIGN.md "Scoring a set of videos") on a real MI355X: score_videos against score() video by
video, bytes against floats, boxes against crops made beforehand, the model left alone, and the two reductions against
their float64 restatements."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
COUNTS = (4, 5, 9, 13)


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _video(n, side, seed, width=None):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, side, width or side, 3), generator=g, dtype=torch.uint8)


def _normalise(u8, mean, std):
    x = ((u8.float() / 255) - torch.tensor(mean)) / torch.tensor(std)
    return x.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope='module')
def small(pkg):
    """The `small` case of tests/test_video_gpu.py, rebuilt here: depth 2, T = 4, 96 x 96, float32, running statistics moved
    by one training forward, the model left in TRAIN mode; and four uint8 videos of 4, 5, 9 and 13 frames."""
    from oracle import istvt_ref as R
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    T, side, depth = 4, 96, 2
    grid = R.stem_out_side(side)
    shapes = {'xcep.model.' + k: v for k, v in R.stem_param_shapes().items()}
    shapes.update({'vit.' + k: v for k, v in R.dsttr_param_shapes(T, grid, depth=depth).items()})
    p = R.random_params(shapes, seed=0)
    x = torch.randn((2, T, 3, side, side), generator=torch.Generator().manual_seed(1))
    model = XceptionVidTr(num_frames=T, grid=grid, depth=depth)
    sd = model.state_dict()
    sd.update(p)
    model.load_state_dict(sd)
    model = model.cuda().train()
    with torch.no_grad():
        model(x.cuda())
    videos = [_video(n, side, 20 + i) for i, n in enumerate(COUNTS)]
    return dict(model=model, videos=videos)


@pytest.fixture(scope='module')
def per_video(small):
    """score() of every video at stride 3 and at stride 1: computed once, shared, left unchanged"""
    from istvt_amd import video
    return {stride: [video.VideoScorer(small['model'], stride=stride).score(v) for v in small['videos']] for stride in (1, 3)}


def _against_per_video(res, refs, tol, what):
    V = len(refs)
    off = res.offsets.tolist()
    assert off[0] == 0 and off[-1] == res.window_logits.shape[0] and len(off) == V + 1
    assert res.window_video.dtype == torch.int32 and res.offsets.dtype == torch.int32 and res.starts.dtype == torch.int64
    assert res.window_video.tolist() == [v for v in range(V) for _ in range(off[v + 1] - off[v])]
    bits = True
    for v, ref in enumerate(refs):
        mine = res.window_logits[off[v]:off[v + 1]]
        assert res.starts[off[v]:off[v + 1]].tolist() == ref.starts.tolist()
        e = (relerr(mine, ref.window_logits), relerr(res.logit_mean[v], ref.logit_mean), relerr(res.prob_mean[v], ref.prob_mean))
        bits = bits and torch.equal(mine, ref.window_logits)
        print('%s video %d: relerr vs score() window logits %.3e, logit_mean %.3e, prob_mean %.3e' % ((what, v) + e))
        assert max(e) < tol, (v, e)
    print('%s: window logits %s the bits of score()' % (what, 'are' if bits else 'are not'))


def test_batches_across_videos_and_reused_slots(small, per_video):
    """(a) frame batches of 5 over videos of 4, 5, 9, 13 frames and a bank of 9 slots for 31 frames"""
    from istvt_amd import video
    model, videos = small['model'], small['videos']
    scorer = video.VideoScorer(model, stride=3, frame_batch=5, window_batch=3, capacity=9)
    labels = [1, 0, 0, 1]
    res = scorer.score_videos(videos, labels=labels)
    assert res.window_logits.shape == (10, 1) and res.window_logits.dtype == torch.float32
    assert tuple(res.logit_mean.shape) == tuple(res.prob_mean.shape) == (4, 1)
    _against_per_video(res, per_video[3], 1e-5, 'capacity 9')
    mixed = [videos[0].cuda(), videos[1], videos[2].cuda(), videos[3]]
    for other in (scorer.score_videos(mixed), scorer.score_videos([v.cuda() for v in videos]),
                  model.score_videos(videos, stride=3, frame_batch=5, window_batch=3, capacity=9)):
        for a, b in zip(res[:6], other[:6]):
            assert torch.equal(a, b)
        assert other.metrics is None
    # room in the bank: full window batches that mix the videos
    roomy = video.VideoScorer(model, stride=3, frame_batch=5, window_batch=3).score_videos(videos)
    _against_per_video(roomy, per_video[3], 1e-5, 'default capacity')
    from test_video_set_cpu import same_metrics
    m = res.metrics
    same_metrics({k: getattr(m, k).item() for k in m._fields}, video.set_metrics_ref(res.logit_mean[:, 0], labels))
    with pytest.raises(ValueError, match='video 1 has 3 frames'):
        scorer.score_videos([videos[0], videos[1][:3].cuda()])


def test_bytes_equal_normalised_float(small, per_video):
    """(b) the same planned steps and the same kernels on both sides"""
    from istvt_amd import video
    videos = small['videos']
    scorer = video.VideoScorer(small['model'], stride=1, frame_batch=5, window_batch=3)
    a = scorer.score_videos(videos)
    b = scorer.score_videos([_normalise(v, *HALF) for v in videos])
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    _against_per_video(a, per_video[1], 1e-5, 'stride 1')


def _boxes(n, Hs, Ws, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randint(40, Hs + 1, (n,), generator=g)
    w = torch.randint(40, Ws + 1, (n,), generator=g)
    y0 = (torch.rand(n, generator=g) * (Hs - h + 1)).long().clamp(max=Hs).minimum(Hs - h)
    x0 = (torch.rand(n, generator=g) * (Ws - w + 1)).long().minimum(Ws - w)
    return torch.stack([y0, x0, h, w], dim=1).to(torch.int32)


def test_boxes_with_two_frame_sizes(small):
    """(c) 120 x 160 and 130 x 110 frames in one call, one of them on the host: the bits of score_videos on the crops"""
    from istvt_amd import ops, video
    full = [_video(5, 120, 31, width=160), _video(6, 130, 32, width=110)]
    boxes = [_boxes(5, 120, 160, 33), _boxes(6, 130, 110, 34)]
    scorer = video.VideoScorer(small['model'], stride=1, frame_batch=4, window_batch=2, side=96)
    crops = [ops.crop_resize_u8(f.cuda(), b, 96) for f, b in zip(full, boxes)]
    a = scorer.score_videos([full[0], full[1].cuda()], boxes=boxes)
    b = scorer.score_videos(crops)
    assert a.window_logits.shape == (5, 1) and a.offsets.tolist() == [0, 2, 5]
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    bad = boxes[1].clone()
    bad[2, 3] = 111                                        # wider than its 110-pixel frame
    with pytest.raises(IndexError):
        scorer.score_videos(full, boxes=[boxes[0], bad])


def test_score_videos_leaves_the_model_and_a_stream_alone(small):
    """(d)"""
    from istvt_amd import video
    model, videos = small['model'], small['videos']
    u8 = videos[3]
    fresh = video.VideoScorer(model, stride=3, frame_batch=4, window_batch=3, capacity=9)
    want = [fresh.push(u8[:6]), fresh.push(u8[6:]), fresh.flush()]
    model.train()
    model.vit.mlp_head.eval()                              # a mixed set of flags must come back as it was
    try:
        flags = [m.training for m in model.modules()]
        before = {k: v.clone() for k, v in model.state_dict().items()}
        assert any('num_batches_tracked' in k for k in before) and any('running_var' in k for k in before)
        scorer = video.VideoScorer(model, stride=3, frame_batch=4, window_batch=3, capacity=9)
        got = [scorer.push(u8[:6])]
        a = scorer.score_videos(videos)
        b = scorer.score_videos(videos)
        got += [scorer.push(u8[6:]), scorer.flush()]
        for x, y in zip(a[:6], b[:6]):
            assert torch.equal(x, y)
        after = model.state_dict()
        assert set(after) == set(before) and all(torch.equal(after[k], v) for k, v in before.items())
        assert [m.training for m in model.modules()] == flags
        assert not a.window_logits.requires_grad
        for (l0, s0), (l1, s1) in zip(want, got):
            assert torch.equal(l0, l1) and torch.equal(s0, s1)
    finally:
        model.vit.mlp_head.train()


@pytest.mark.parametrize('nc', [1, 3])
def test_windows_reduce(pkg, nc):
    """(e) videos of 1, 1, 68, 1 and 329 windows (more than one pass of the 256 lanes)"""
    from istvt_amd import ops, video
    off = [0, 1, 2, 70, 71, 400]
    g = torch.Generator().manual_seed(40 + nc)
    x = (torch.rand((400, nc), generator=g) * 60 - 30).float()
    x[5, 0], x[6, 0] = 30.0, -30.0
    lm64, pm64 = video.windows_reduce_ref(x, off)
    lm, pm = ops.windows_reduce(x.cuda(), off)
    assert lm.dtype == pm.dtype == torch.float32 and tuple(lm.shape) == tuple(pm.shape) == (5, nc)
    r32 = lm64.float()
    ulp = (torch.nextafter(r32.abs(), torch.full_like(r32, float('inf'))) - r32.abs()).double()
    dl = (lm.cpu().double() - lm64).abs()
    dp = (pm.cpu().double() - pm64).abs()
    print('windows_reduce nc=%d: logit_mean off by at most %.3f ulp, prob_mean by %.3e' % (nc, float((dl / ulp).max()), float(dp.max())))
    assert bool((dl <= ulp).all())
    assert float(dp.max()) <= 1e-6
    lm2, pm2 = ops.windows_reduce(x.cuda(), torch.tensor(off, dtype=torch.int32))
    assert torch.equal(lm, lm2) and torch.equal(pm, pm2)
    lm3, pm3 = ops.windows_reduce(x.cuda(), torch.tensor(off, dtype=torch.int32).cuda(), checked=True)
    assert torch.equal(lm, lm3) and torch.equal(pm, pm3)
    for bad in ([0, 1, 2, 70, 71, 399], [1, 2, 70, 71, 400], [0, 1, 1, 70, 71, 400], [0, 71, 70, 400], [400]):
        with pytest.raises(ValueError):
            ops.windows_reduce(x.cuda(), bad)
    with pytest.raises(TypeError):
        ops.windows_reduce(x.cuda().double(), off)
    with pytest.raises(RuntimeError):
        ops.windows_reduce(x, off)


def test_auc_pairs_and_set_metrics(pkg):
    """(f) V = 1, 2, 257 and 1000: the host's integer counts and its fp64 AUC, exactly"""
    from istvt_amd import ops, video
    from test_video_set_cpu import metric_cases, same_metrics
    for name, s, lab in metric_cases():
        for thr in (0.0, 3.0):
            ref = video.set_metrics_ref(s, lab, thr)
            m = video.set_metrics(s.cuda(), lab, thr)
            got = {k: getattr(m, k).item() for k in m._fields}
            same_metrics(got, ref)
        counts, auc = ops.auc_pairs(s.cuda(), lab.to(torch.int32).cuda(), 3.0)
        same_metrics(dict(zip(ops.AUC_COUNTS, counts.tolist()), auc=float(auc)), ref)
        counts2, auc2 = ops.auc_pairs(s.cuda(), lab.to(torch.int32).cuda(), 3.0)
        assert torch.equal(counts, counts2) and (torch.equal(auc, auc2) or (math.isnan(float(auc)) and math.isnan(float(auc2))))
    s = torch.zeros(4).cuda()
    with pytest.raises(ValueError):
        video.set_metrics(s, [0, 1, 2, 0])
    with pytest.raises(ValueError):
        video.set_metrics(s, [0, 1, 0])
    with pytest.raises(TypeError):
        ops.auc_pairs(s, torch.zeros(4, dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError):
        ops.auc_pairs(s, torch.zeros(3, dtype=torch.int32).cuda())


def test_production_224_bf16(pkg):
    """(g) three videos of 8, 9 and 20 frames, 224 x 224, T = 8, depth 2, bfloat16, against score() video by video at the
    bf16 bound of test_video_gpu.py's test_scorer_vs_clip_path"""
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    torch.manual_seed(11)
    model = XceptionVidTr(num_frames=8, grid=14, depth=2, compute_dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(11)
    for name, buf in model.named_buffers():                # running statistics away from (0, 1)
        if name.endswith('running_mean'):
            buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
        elif name.endswith('running_var'):
            buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
    model = model.cuda().eval()
    videos = [_video(n, 224, 50 + n) for n in (8, 9, 20)]
    scorer = video.VideoScorer(model, stride=2, frame_batch=16, window_batch=4)
    res = scorer.score_videos(videos, labels=[0, 1, 1])
    off = res.offsets.tolist()
    assert off == [0, 1, 3, 10] and torch.isfinite(res.window_logits).all()
    for v, u8 in enumerate(videos):
        ref = scorer.score(u8)
        assert res.starts[off[v]:off[v + 1]].tolist() == ref.starts.tolist()
        d = float((res.window_logits[off[v]:off[v + 1]] - ref.window_logits).abs().max())
        dm = float((res.logit_mean[v] - ref.logit_mean).abs().max())
        dp = float((res.prob_mean[v] - ref.prob_mean).abs().max())
        bound = 5e-2 * max(1.0, float(ref.window_logits.abs().max()))
        print('224 bf16 video %d: max abs diff vs score() %.3e (means %.3e, %.3e), bound %.3e' % (v, d, dm, dp, bound))
        assert d < bound and dm < bound and dp < bound
    assert int(res.metrics.positives) == 2 and int(res.metrics.negatives) == 1
