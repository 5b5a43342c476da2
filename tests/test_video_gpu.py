"""Video scoring (DESIGN.md "Video scoring") on a real MI355X: the byte conv1 and the token gather against the kernels
they restate (bit for bit), the scorer against the oracle and against model(clips), streaming against the whole video,
and the promise that a scoring call leaves the model as it found it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def relerr(a, b):
    a = torch.as_tensor(a.detach().cpu() if torch.is_tensor(a) else np.asarray(a), dtype=torch.float64)
    b = torch.as_tensor(b.detach().cpu() if torch.is_tensor(b) else np.asarray(b), dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _video(n, side, seed):
    """uint8 (n, side, side, 3) in which every channel takes every byte value (the first 256 pixels of frame 0, permuted per
    channel) and the rest is random"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 256, (n, side, side, 3), generator=g, dtype=torch.uint8)
    flat = v.view(-1, 3)
    for c in range(3):
        flat[:256, c] = torch.randperm(256, generator=g).to(torch.uint8)
    assert all(len(torch.unique(v[..., c])) == 256 for c in range(3))
    return v


def _normalise(u8, mean, std):
    """host, float32, as torchvision's ToTensor + Normalize: ((u / 255) - mean) / std -> (n, 3, S, S)"""
    x = ((u8.float() / 255) - torch.tensor(mean)) / torch.tensor(std)
    return x.permute(0, 3, 1, 2).contiguous()


def _windows(x, starts, T):
    return torch.stack([x[s:s + T] for s in starts])


# ---- kernels ---------------------------------------------------------------------------------------------------------
# Row-by-row staging above side 300, 2 frames each, bf16.  Side 1001: odd, so every staged row has another lead; a row pitch of
# 3024 bytes lets at most 7 output rows into the 48 KiB budget and the chooser takes R = 4 (Ho = 500: 4..7 fill the 256-thread
# passes equally).  Side 525: the budget itself decides, R = 14 (31 rows of pitch 1600 do not fit; the contiguous budget took
# 15), and the last group of a frame has 10 of its 14 rows.
CONV1_CASES = [pytest.param(side, norm, dtype, 3, id='%d-%s-%s' % (side, nid, did))
               for dtype, did in ((torch.float32, 'f32'), (torch.bfloat16, 'bf16'))
               for norm, nid in ((IMAGENET, 'imagenet'), (HALF, 'half')) for side in (96, 139, 224, 300)]
CONV1_CASES.append(pytest.param(1001, IMAGENET, torch.bfloat16, 2, id='1001-imagenet-bf16'))
CONV1_CASES.append(pytest.param(525, HALF, torch.bfloat16, 2, id='525-half-bf16'))


@pytest.mark.parametrize('side,norm,dtype,n', CONV1_CASES)
def test_conv1_from_bytes_bit_identical(pkg, side, norm, dtype, n):
    from istvt_amd import ops
    mean, std = norm
    u8 = _video(n, side, side)
    w = torch.randn((32, 3, 3, 3), generator=torch.Generator().manual_seed(side + 1)).cuda()
    x = _normalise(u8, mean, std).cuda()
    Ho = (side - 3) // 2 + 1
    ref = ops.conv1_fwd(x, w, dtype)
    m, s = torch.tensor(mean).cuda(), torch.tensor(std).cuda()
    dev = u8.cuda()
    out = ops.conv1_fwd_u8(dev, m, s, w, dtype)
    assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 0
    assert torch.equal(out, ref)
    # a view that starts in the middle of the allocation (frame 1 on: an odd byte offset at odd sides)
    out1 = ops.conv1_fwd_u8(dev[1:], m, s, w, dtype)
    assert torch.equal(out1, ref[Ho * Ho:])
    # the inference entry is the identity view of the training entry
    assert torch.equal(out, ops.conv1_fwd_u8_view(dev, None, side, m, s, w, dtype))
    with pytest.raises(RuntimeError):
        ops.conv1_fwd_u8(dev.permute(0, 3, 1, 2), m, s, w, dtype)
    with pytest.raises(TypeError):
        ops.conv1_fwd_u8(x, m, s, w, dtype)


def test_byte_entries_refuse_sides_past_4096(pkg):
    """side 4097: the shape error from all three byte entries that stage rows, before any launch (the buffers are whole, so a
    launch would be a wrong answer here, not a fault)"""
    from istvt_amd import _lib, ops
    L, S = _lib.lib(), 4097
    Ho = (S - 3) // 2 + 1
    x = torch.zeros((1, S, S, 3), dtype=torch.uint8, device='cuda')
    out = torch.empty((Ho * Ho, 32), dtype=torch.bfloat16, device='cuda')
    m, s = torch.tensor(HALF[0]).cuda(), torch.tensor(HALF[1]).cuda()
    w = torch.zeros((32, 3, 3, 3), device='cuda')
    st, bf16 = ops._stream(), ops._DT[torch.bfloat16]
    assert L.istvt_conv1_fwd_u8(x.data_ptr(), m.data_ptr(), s.data_ptr(), w.data_ptr(), out.data_ptr(), 1, S, bf16, st) == -3
    assert L.istvt_conv1_fwd_u8_view(x.data_ptr(), x.numel(), S, S, None, m.data_ptr(), s.data_ptr(), w.data_ptr(),
                                     out.data_ptr(), 1, S, bf16, st) == -3
    assert L.istvt_im2col_conv1_u8(x.data_ptr(), x.numel(), S, S, None, m.data_ptr(), s.data_ptr(), out.data_ptr(), 1, S, bf16,
                                   st) == -3
    with pytest.raises(RuntimeError, match='invalid shape'):
        ops.conv1_fwd_u8(x, m, s, w, torch.bfloat16)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('T', [4, 8, 16])
def test_tokens_gather_bit_identical(pkg, T, dtype):
    from istvt_amd import ops
    g = torch.Generator().manual_seed(T)
    cap, hw, D, W = 23, 36, 728, 7
    bank = torch.randn((cap, hw, D), generator=g).to(dtype).cuda()
    idx = torch.randint(0, cap, (W, T), generator=g, dtype=torch.int32)
    idx[1] = idx[0]                                        # a repeated window and a repeated frame within one
    idx[2, 1] = idx[2, 0]
    space, temporal = torch.randn((1, 1, D), generator=g).cuda(), torch.randn((1, 1, D), generator=g).cuda()
    pos = torch.randn((1, T, hw + 3, D), generator=g).cuda()      # declared with more tokens per frame than used
    for pad in (False, True):
        ref = ops.tokens_fwd(bank[idx.long().cuda()], space, temporal, pos, pad=pad)
        out = ops.tokens_gather_fwd(bank, idx, space, temporal, pos, pad=pad)
        assert out.shape == ref.shape == (W, (T + 1) * (hw + 1), D)
        assert torch.equal(out, ref)
        assert torch.equal(ops.tokens_gather_fwd(bank, idx.cuda(), space, temporal, pos, pad=pad), ref)
    bad = idx.clone()
    bad[3, 2] = cap
    with pytest.raises(IndexError):
        ops.tokens_gather_fwd(bank, bad, space, temporal, pos)
    bad[3, 2] = -1
    with pytest.raises(IndexError):
        ops.tokens_gather_fwd(bank, bad, space, temporal, pos)
    with pytest.raises(RuntimeError):
        ops.tokens_gather_fwd(bank, idx.long(), space, temporal, pos)


# ---- the scorer ------------------------------------------------------------------------------------------------------
def _oracle_case(T, side, depth, seed=0):
    from oracle import istvt_ref as R
    grid = R.stem_out_side(side)
    shapes = {'xcep.model.' + k: v for k, v in R.stem_param_shapes().items()}
    shapes.update({'vit.' + k: v for k, v in R.dsttr_param_shapes(T, grid, depth=depth).items()})
    p = R.random_params(shapes, seed=seed)
    x = torch.randn((2, T, 3, side, side), generator=torch.Generator().manual_seed(seed + 1))
    return R, p, x, grid


def _hip_model(p, T, grid, depth, dtype=torch.float32):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=T, grid=grid, depth=depth, compute_dtype=dtype)
    sd = model.state_dict()
    sd.update(p)
    model.load_state_dict(sd)
    return model.cuda().train()


@pytest.fixture(scope='module')
def small(pkg):
    """The case of test_eval_forward_vs_oracle (depth 2, T = 4, 96x96; running statistics moved by one training forward
    on both sides) and an 11-frame uint8 video.  The model is left in TRAIN mode: the scorer has to cope."""
    R, p, x, grid = _oracle_case(4, 96, 2)
    pr = {k: v.clone() for k, v in p.items()}
    with torch.no_grad():
        R.xception_vidtr_forward(pr, x, depth=2, training=True)
    model = _hip_model(p, 4, grid, 2)
    with torch.no_grad():
        model(x.cuda())
    u8 = _video(11, 96, 5)
    return dict(R=R, pr=pr, model=model, u8=u8, xn=_normalise(u8, *HALF), grid=grid)


@pytest.mark.parametrize('stride', [1, 3])
def test_scorer_vs_oracle(small, stride):
    from istvt_amd import video
    R, pr, model, u8, xn = small['R'], small['pr'], small['model'], small['u8'], small['xn']
    res = video.VideoScorer(model, stride=stride).score(u8)
    starts = video.window_starts(11, 4, stride, True)
    assert res.starts.tolist() == starts and (stride == 1 or starts[-1] == 7)
    assert res.window_logits.shape == (len(starts), 1) and res.window_logits.dtype == torch.float32
    with torch.no_grad():
        ref = R.xception_vidtr_forward({k: v.clone() for k, v in pr.items()}, _windows(xn, starts, 4), depth=2, training=False)
    for w in range(len(starts)):
        e = relerr(res.window_logits[w], ref[w])
        print('stride %d window %d (start %d): relerr vs oracle %.3e' % (stride, w, starts[w], e))
        assert e < 1e-3
    assert relerr(res.window_logits, ref) < 1e-3
    assert relerr(res.logit_mean, ref.mean(0)) < 1e-3
    assert relerr(res.prob_mean, torch.sigmoid(ref).mean(0)) < 1e-3


@pytest.mark.parametrize('stride', [1, 3])
def test_scorer_vs_clip_path(small, stride):
    """scorer.score(u8) against model(windows) in eval mode on the materialised, host-normalised windows; host frames
    and device frames; bfloat16 against float32"""
    from istvt_amd import video
    model, u8, xn = small['model'], small['u8'], small['xn']
    starts = video.window_starts(11, 4, stride, True)
    res = video.VideoScorer(model, stride=stride).score(u8)
    model.eval()
    try:
        with torch.no_grad():
            ref = model(_windows(xn, starts, 4).cuda())
    finally:
        model.train()
    e = relerr(res.window_logits, ref)
    print('stride %d: scorer vs clip path relerr %.3e' % (stride, e))
    assert e < 1e-5
    assert torch.equal(video.VideoScorer(model, stride=stride).score(u8.cuda()).window_logits, res.window_logits)
    assert torch.equal(model.score_video(u8, stride=stride).window_logits, res.window_logits)
    mb = _hip_model({}, 4, small['grid'], 2, dtype=torch.bfloat16)
    mb.load_state_dict(model.state_dict())
    outb = video.VideoScorer(mb, stride=stride).score(u8).window_logits
    d = float((outb - res.window_logits).abs().max())
    print('stride %d: bf16 scorer vs f32 scorer max abs diff %.3e' % (stride, d))
    assert d < 5e-2 * max(1.0, float(res.window_logits.abs().max()))


def test_bytes_equal_normalised_float(small):
    """conv1 from bytes is bit-identical to conv1 on the normalised tensor, and everything after conv1 is the same code"""
    from istvt_amd import video
    scorer = video.VideoScorer(small['model'], stride=1)
    a, b = scorer.score(small['u8']), scorer.score(small['xn'])
    assert torch.equal(a.window_logits, b.window_logits) and torch.equal(a.starts, b.starts)
    assert torch.equal(a.prob_mean, b.prob_mean) and torch.equal(a.logit_mean, b.logit_mean)


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('chunk', [1, 3, 5])
def test_push_matches_score(small, chunk, stride):
    from istvt_amd import video
    model, u8 = small['model'], small['u8']
    whole = video.VideoScorer(model, stride=stride).score(u8)
    scorer = video.VideoScorer(model, stride=stride, frame_batch=4, window_batch=3, capacity=9)   # the ring wraps
    logits, starts = [], []
    for i in range(0, 11, chunk):
        l, s = scorer.push(u8[i:i + chunk])
        assert l.shape[0] == s.shape[0] and all(int(v) + 4 <= i + chunk for v in s)
        logits.append(l)
        starts.append(s)
    l, s = scorer.flush()
    assert s.tolist() == ([7] if stride == 3 else [])
    logits, starts = torch.cat(logits + [l]), torch.cat(starts + [s])
    assert starts.tolist() == whole.starts.tolist()
    e = relerr(logits, whole.window_logits)
    print('chunk %d stride %d: push vs score relerr %.3e' % (chunk, stride, e))
    assert e < 1e-5
    with pytest.raises(RuntimeError):
        scorer.push(u8[:1])
    scorer.reset()
    l, s = scorer.push(u8)
    assert s.tolist() == video.window_starts(11, 4, stride, False)


def test_score_leaves_the_model_alone(small):
    from istvt_amd import video
    model, u8 = small['model'], small['u8']
    model.train()
    model.vit.mlp_head.eval()                              # a mixed set of flags must come back as it was
    try:
        flags = [m.training for m in model.modules()]
        before = {k: v.clone() for k, v in model.state_dict().items()}
        assert any('num_batches_tracked' in k for k in before) and any('running_var' in k for k in before)
        scorer = video.VideoScorer(model)
        a = scorer.score(u8)
        b = scorer.score(u8)
        assert torch.equal(a.window_logits, b.window_logits) and torch.equal(a.prob_mean, b.prob_mean)
        after = model.state_dict()
        assert set(after) == set(before) and all(torch.equal(after[k], v) for k, v in before.items())
        assert [m.training for m in model.modules()] == flags
        assert not a.window_logits.requires_grad
    finally:
        model.vit.mlp_head.train()


def test_stem_byte_entry_refused_in_training(small):
    model = small['model']
    xcep = model.xcep.model
    u8 = small['u8'][:2].cuda()
    with torch.no_grad(), pytest.raises(RuntimeError, match='eval mode'):
        xcep.low_level_features_nhwc(u8, torch.float32, HALF[0], HALF[1])          # the fixture leaves it in train mode
    xcep.eval()
    try:
        with pytest.raises(RuntimeError, match='no_grad'):
            xcep.low_level_features_nhwc(u8, torch.float32, HALF[0], HALF[1])
        with torch.no_grad():
            f = xcep.low_level_features_nhwc(u8, torch.float32, HALF[0], HALF[1])
        assert f.shape == (2, 6, 6, 728)
    finally:
        xcep.train()


# ---- production geometry ---------------------------------------------------------------------------------------------
def _random_model(T, grid, depth, dtype, seed):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    torch.manual_seed(seed)
    model = XceptionVidTr(num_frames=T, grid=grid, depth=depth, compute_dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    for name, buf in model.named_buffers():                # running statistics away from (0, 1)
        if name.endswith('running_mean'):
            buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
        elif name.endswith('running_var'):
            buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
    return model.cuda().eval()


def test_production_224_bf16(pkg):
    """24 frames, 224x224, T = 8, depth 2, bfloat16, stride 1: 17 windows against the clip path at the bf16 eval bound"""
    from istvt_amd import video
    model = _random_model(8, 14, 2, torch.bfloat16, 11)
    u8 = _video(24, 224, 12)
    res = video.VideoScorer(model, stride=1, frame_batch=16, window_batch=8).score(u8)
    starts = video.window_starts(24, 8, 1)
    assert res.starts.tolist() == starts and len(starts) == 17
    with torch.no_grad():
        ref = torch.cat([model(_windows(_normalise(u8, *HALF), starts[i:i + 8], 8).cuda()) for i in range(0, 17, 8)])
    d = float((res.window_logits - ref).abs().max())
    print('224 bf16: scorer vs clip path max abs diff %.3e, |ref|max %.3e' % (d, float(ref.abs().max())))
    assert torch.isfinite(res.window_logits).all()
    assert d < 5e-2 * max(1.0, float(ref.abs().max()))


def test_native_300_f32(pkg):
    """the reference's own geometry: 300x300 crops, T = 6, 19x19 grid, float32"""
    from istvt_amd import video
    model = _random_model(6, 19, 2, torch.float32, 13)
    u8 = _video(9, 300, 14)
    res = video.VideoScorer(model, stride=2, mean=IMAGENET[0], std=IMAGENET[1]).score(u8)
    starts = video.window_starts(9, 6, 2)
    assert res.starts.tolist() == starts == [0, 2, 3]
    with torch.no_grad():
        ref = model(_windows(_normalise(u8, *IMAGENET), starts, 6).cuda())
    e = relerr(res.window_logits, ref)
    print('300 f32: scorer vs clip path relerr %.3e' % e)
    assert e < 1e-5
