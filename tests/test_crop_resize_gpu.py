"""Frames and boxes (DESIGN.md "Frames and boxes") on a real MI355X: istvt_crop_resize_u8 against a float64 restatement
of its definition that this file carries itself, and the scorer's `boxes` keyword against the scorer on crops made
beforehand by the same kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = 1e-3            # a byte may differ by one only where the float64 value is this close to a half
BAND_SHARE = 0.02      # and at most this share of a box's bytes may lie there


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


# ---- the definition, restated in float64 ------------------------------------------------------------------------------
def _axis(n_in, n_out):
    """dense float64 (n_out, n_in) weights of one axis"""
    m = np.zeros((n_out, n_in), dtype=np.float64)
    scale = n_in / n_out
    sup = max(scale, 1.0)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - sup + 0.5), 0)
        hi = min(int(c + sup + 0.5), n_in)
        w = np.array([max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)], dtype=np.float64)
        m[i, lo:hi] = w / w.sum()
    return m


def _restate(frame, box, S):
    """frame uint8 numpy (Hs, Ws, 3), box (y0, x0, h, w) -> float64 (S, S, 3) before rounding; horizontal pass first"""
    y0, x0, h, w = box
    crop = frame[y0:y0 + h, x0:x0 + w].astype(np.float64)
    hor = np.einsum('xw,hwc->hxc', _axis(w, S), crop)
    return np.einsum('yh,hxc->yxc', _axis(h, S), hor)


def _assert_box(out, frame, box, S, what):
    v = _restate(frame, box, S)
    want = np.clip(np.floor(v + 0.5), 0, 255)
    got = out.astype(np.float64)
    band = np.abs(v - np.floor(v) - 0.5) <= BAND
    share = float(band.mean())
    nd = int((got != want).sum())
    print('%s box %s -> %d: %d of %d bytes differ, max |diff| %d, band share %.3f %%'
          % (what, tuple(box), S, nd, got.size, int(np.abs(got - want).max()), 100 * share))
    assert np.abs(got - want).max() <= 1
    assert np.array_equal(got[~band], want[~band])
    assert share <= BAND_SHARE


def _frames(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _boxes_for(Hs, Ws, S):
    """the boxes of the issue that fit a Hs x Ws frame at output side S"""
    bh, bw = min(Hs, 20), min(Ws, 25)
    boxes = [(3, 4, 11, 9),                                   # an upscale; 3 w = 27 is no multiple of 16
             (Hs - 1, Ws - 1, 1, 1), (Hs // 2, Ws // 3, 1, 1),               # 1 x 1
             (0, 0, bh, bw), (0, Ws - bw, bh, bw), (Hs - bh, 0, bh, bw), (Hs - bh, Ws - bw, bh, bw),     # the corners
             (0, 0, Hs, Ws),                                  # the whole frame, h != w
             (2, 5, Hs - 7, 13), (1, 0, 7, Ws - 3)]           # long and thin, both ways
    if S <= min(Hs, Ws):
        boxes += [(5, 7, S, S), (Hs - S, Ws - S, S, S)]       # identity
    if min(Hs, Ws) >= 128 and 128 <= 8 * S:
        boxes += [(3, Ws - 128, 128, 128)]                    # the 8 x downscale at S = 16
    return [b for b in boxes if b[2] <= 8 * S and b[3] <= 8 * S]


def _run(src, boxes, S):
    """src uint8 host (n, Hs, Ws, 3); box i is cut from frame i % n -> (frames used (host), output (host numpy))"""
    from istvt_amd import ops
    idx = [i % src.shape[0] for i in range(len(boxes))]
    frames = src[idx].contiguous()
    out = ops.crop_resize_u8(frames.cuda(), torch.tensor(boxes, dtype=torch.int32), S)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (len(boxes), S, S, 3) and out.is_cuda
    return frames, out.cpu().numpy()


@pytest.mark.parametrize('shape', [(3, 37, 53, 3), (2, 131, 200, 3)], ids=['37x53', '131x200'])
@pytest.mark.parametrize('S', [16, 48])
def test_kernel_against_restatement(pkg, shape, S):
    src = _frames(shape, shape[1] + S)
    boxes = _boxes_for(shape[1], shape[2], S)
    frames, out = _run(src, boxes, S)
    for i, box in enumerate(boxes):
        _assert_box(out[i], frames[i].numpy(), box, S, '%dx%d' % shape[1:3])


def test_kernel_at_the_models_side(pkg):
    """224 from 500 x 317: the row-group chooser at the model's own side (more than 64 KiB of LDS, several passes)"""
    src = _frames((2, 500, 317, 3), 224)
    boxes = [(0, 0, 500, 317), (100, 50, 300, 250), (276, 93, 224, 224), (10, 20, 150, 131)]
    frames, out = _run(src, boxes, 224)
    for i, box in enumerate(boxes):
        _assert_box(out[i], frames[i].numpy(), box, 224, '500x317')
    assert np.array_equal(out[2], frames[2, 276:500, 93:317].numpy())


@pytest.mark.parametrize('shape,S', [((3, 37, 53, 3), 16), ((2, 131, 200, 3), 48), ((2, 131, 200, 3), 16)])
def test_identity_box_is_the_slice(pkg, shape, S):
    from istvt_amd import ops
    src = _frames(shape, 5)
    n, Hs, Ws = shape[:3]
    boxes = [(0, 0, S, S), (Hs - S, Ws - S, S, S), (Hs - S - 1, 3, S, S)][:n]
    out = ops.crop_resize_u8(src.cuda(), torch.tensor(boxes, dtype=torch.int32), S).cpu()
    for i, (y0, x0, h, w) in enumerate(boxes):
        assert torch.equal(out[i], src[i, y0:y0 + h, x0:x0 + w])


def test_bytes_outside_the_box_do_not_matter(pkg):
    from istvt_amd import ops
    S = 16
    src = _frames((3, 37, 53, 3), 6)
    boxes = [(3, 4, 11, 9), (9, 20, 25, 31), (36, 52, 1, 1)]
    other = _frames((3, 37, 53, 3), 7)
    for i, (y0, x0, h, w) in enumerate(boxes):
        other[i, y0:y0 + h, x0:x0 + w] = src[i, y0:y0 + h, x0:x0 + w]
    assert not torch.equal(other, src)
    b = torch.tensor(boxes, dtype=torch.int32)
    assert torch.equal(ops.crop_resize_u8(src.cuda(), b, S), ops.crop_resize_u8(other.cuda(), b, S))


def test_slices_guard_band_and_determinism(pkg):
    from istvt_amd import ops
    S = 16
    n, Hs, Ws = 3, 37, 53
    src = _frames((n, Hs, Ws, 3), 8)
    boxes = torch.tensor([(0, 0, 20, 25), (3, 4, 11, 9), (Hs - 20, Ws - 25, 20, 25)], dtype=torch.int32)
    dev = src.cuda()
    base = ops.crop_resize_u8(dev, boxes, S)
    assert torch.equal(ops.crop_resize_u8(dev, boxes, S), base)                          # a second run: the same bits
    # a slice that starts mid-allocation at an odd byte offset (one frame is 5883 bytes)
    big = torch.empty((n + 1, Hs, Ws, 3), dtype=torch.uint8, device='cuda')
    big[0] = 77
    big[1:] = dev
    assert (big[1:].data_ptr() - big.data_ptr()) % 2 == 1
    assert torch.equal(ops.crop_resize_u8(big[1:], boxes, S), base)
    assert torch.equal(ops.crop_resize_u8(dev[1:], boxes[1:].contiguous(), S), base[1:])
    # a guard band on both sides, filled with a sentinel: its value must not show (the corner boxes touch the first and
    # the last byte of the tensor, so their 16-byte pieces reach into the band)
    G, N = 4099, n * Hs * Ws * 3
    for sentinel in (0, 255, 171):
        buf = torch.full((G + N + G,), sentinel, dtype=torch.uint8, device='cuda')
        buf[G:G + N] = dev.view(-1)
        assert torch.equal(ops.crop_resize_u8(buf[G:G + N].view(n, Hs, Ws, 3), boxes, S), base)
        assert bool((buf[:G] == sentinel).all()) and bool((buf[G + N:] == sentinel).all())
    # `out` given, at an odd offset inside a larger buffer: the same bits, and nothing around it written
    M = n * S * S * 3
    obuf = torch.full((M + 64,), 9, dtype=torch.uint8, device='cuda')
    got = ops.crop_resize_u8(dev, boxes, S, out=obuf[5:5 + M].view(n, S, S, 3))
    assert torch.equal(got, base) and bool((obuf[:5] == 9).all()) and bool((obuf[5 + M:] == 9).all())


def test_clips_share_a_box(pkg):
    from istvt_amd import ops
    src = _frames((2, 3, 37, 53, 3), 9)
    boxes = torch.tensor([(3, 4, 11, 9), (9, 20, 25, 31)], dtype=torch.int32)
    out = ops.crop_resize_u8(src.cuda(), boxes, 16)
    assert tuple(out.shape) == (2, 3, 16, 16, 3)
    flat = ops.crop_resize_u8(src.view(6, 37, 53, 3).cuda(), boxes.repeat_interleave(3, dim=0), 16)
    assert torch.equal(out.view(6, 16, 16, 3), flat)


def test_refusals_before_any_launch(pkg):
    from istvt_amd import ops
    dev = _frames((2, 37, 53, 3), 10).cuda()

    def b(row, dtype=torch.int32):
        return torch.tensor([[0, 0, 10, 10], row], dtype=dtype)

    for row in ([-1, 0, 10, 10], [0, -1, 10, 10], [30, 0, 8, 10], [0, 45, 10, 9]):
        with pytest.raises(IndexError):
            ops.crop_resize_u8(dev, b(row), 16)
    with pytest.raises(ValueError):
        ops.crop_resize_u8(dev, b([0, 0, 0, 10]), 16)
    with pytest.raises(ValueError):
        ops.crop_resize_u8(dev, b([0, 0, 10, 33]), 4)
    with pytest.raises(TypeError):
        ops.crop_resize_u8(dev, b([0, 0, 10, 10], torch.int64), 16)
    with pytest.raises(ValueError):
        ops.crop_resize_u8(dev, b([0, 0, 10, 10])[:1], 16)
    with pytest.raises(TypeError):
        ops.crop_resize_u8(dev.float(), b([0, 0, 10, 10]), 16)
    with pytest.raises(RuntimeError):
        ops.crop_resize_u8(dev.cpu(), b([0, 0, 10, 10]), 16)
    with pytest.raises(RuntimeError):
        ops.crop_resize_u8(dev, b([0, 0, 10, 10]), 16, out=torch.empty((2, 16, 16, 3), dtype=torch.uint8))
    torch.cuda.synchronize()


# ---- the scorer -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def boxed(pkg):
    """T = 4, side 96, depth 2, float32, a seeded random model in eval mode; 11 frames of 140 x 170 with boxes of side
    60..140; the crops made beforehand by the kernel"""
    from istvt_amd import ops
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    torch.manual_seed(21)
    model = XceptionVidTr(num_frames=4, grid=6, depth=2, compute_dtype=torch.float32)
    g = torch.Generator().manual_seed(21)
    for name, buf in model.named_buffers():                # running statistics away from (0, 1)
        if name.endswith('running_mean'):
            buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
        elif name.endswith('running_var'):
            buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
    model = model.cuda().eval()
    frames = _frames((11, 140, 170, 3), 22)
    h = torch.randint(60, 141, (11,), generator=g)
    w = torch.randint(60, 141, (11,), generator=g)
    y0 = (torch.rand(11, generator=g) * (140 - h + 1).float()).long().clamp(max=140 - 1)
    x0 = (torch.rand(11, generator=g) * (170 - w + 1).float()).long()
    y0, x0 = torch.minimum(y0, 140 - h), torch.minimum(x0, 170 - w)
    boxes = torch.stack([y0, x0, h, w], dim=1).to(torch.int32)
    crops = ops.crop_resize_u8(frames.cuda(), boxes, 96)
    return dict(model=model, frames=frames, boxes=boxes, crops=crops)


@pytest.mark.parametrize('stride', [1, 3])
def test_score_with_boxes_is_score_on_crops(boxed, stride):
    from istvt_amd import video
    scorer = video.VideoScorer(boxed['model'], stride=stride, frame_batch=4, side=96)
    ref = scorer.score(boxed['crops'])
    for frames in (boxed['frames'], boxed['frames'].cuda()):                 # host frames (uploaded per stem batch), device frames
        res = scorer.score(frames, boxes=boxed['boxes'])
        assert torch.isfinite(res.window_logits).all() and res.starts.tolist() == ref.starts.tolist()
        assert torch.equal(res.window_logits, ref.window_logits)
        assert torch.equal(res.logit_mean, ref.logit_mean) and torch.equal(res.prob_mean, ref.prob_mean)
    res = boxed['model'].score_video(boxed['frames'], boxes=boxed['boxes'], stride=stride, frame_batch=4, side=96)
    assert torch.equal(res.window_logits, ref.window_logits)


@pytest.mark.parametrize('stride', [1, 3])
def test_explain_with_boxes_is_explain_on_crops(boxed, stride):
    from istvt_amd import video
    scorer = video.VideoScorer(boxed['model'], stride=stride, frame_batch=4, side=96)
    ref = scorer.explain(boxed['crops'])
    ex = scorer.explain(boxed['frames'], boxes=boxed['boxes'])
    assert float(ref.frame_s.abs().max()) > 0
    for name in ('frame_s', 'frame_t', 'frame_weight', 'frame_logit', 'count'):
        assert torch.equal(getattr(ex, name), getattr(ref, name)), name
    assert torch.equal(ex.score.window_logits, ref.score.window_logits)
    ex2 = boxed['model'].explain_video(boxed['frames'], boxes=boxed['boxes'], stride=stride, frame_batch=4, side=96)
    assert torch.equal(ex2.frame_s, ref.frame_s)


def test_push_with_boxes_agrees_with_score(boxed):
    from istvt_amd import video
    frames, boxes = boxed['frames'], boxed['boxes']
    for stride in (1, 3):
        scorer = video.VideoScorer(boxed['model'], stride=stride, frame_batch=4, side=96)
        ref = scorer.score(frames, boxes=boxes)
        outs, starts = [], []
        for lo, hi in ((0, 3), (3, 8), (8, 11)):
            l, s = scorer.push(frames[lo:hi], boxes=boxes[lo:hi].contiguous())
            outs.append(l), starts.extend(s.tolist())
        l, s = scorer.flush()
        outs.append(l), starts.extend(s.tolist())
        got = torch.cat(outs)
        assert starts == ref.starts.tolist()
        d = float((got - ref.window_logits).abs().max())
        print('stride %d: push 3 + 5 + 3 with boxes vs score: max abs diff %.3e' % (stride, d))
        assert d <= 1e-5


def test_no_state_leaks_and_modes_do_not_mix(boxed):
    from istvt_amd import video
    model, frames, boxes, crops = boxed['model'], boxed['frames'], boxed['boxes'], boxed['crops']
    flags = [m.training for m in model.modules()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert any('num_batches_tracked' in k for k in before) and any('running_var' in k for k in before)
    scorer = video.VideoScorer(model, side=96)
    a = scorer.score(crops)
    scorer.score(frames, boxes=boxes)
    scorer.explain(frames, boxes=boxes)
    b = scorer.score(crops)
    assert torch.equal(a.window_logits, b.window_logits) and torch.equal(a.prob_mean, b.prob_mean)
    after = model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], v) for k, v in before.items())
    assert [m.training for m in model.modules()] == flags
    # a stream keeps one mode
    scorer.reset()
    scorer.push(frames[:3], boxes=boxes[:3].contiguous())
    with pytest.raises(ValueError):
        scorer.push(crops[3:6])
    scorer.reset()
    scorer.push(crops[:3])
    with pytest.raises(ValueError):
        scorer.push(frames[3:6], boxes=boxes[3:6].contiguous())
    scorer.reset()
    with pytest.raises(ValueError):                                            # no side anywhere
        video.VideoScorer(model).score(frames, boxes=boxes)
