"""Aligned crops (DESIGN.md "Aligned crops") on a real MI355X: istvt_warp_similarity_u8 against a float64 restatement of the
definition carried here (it does not import clips), the exact cases, the crop kernel on square boxes, what the output may
and may not depend on, NV12 against the warp of the converted frames, a table that was not validated, and the scorer's
transforms= against the plain scorer on warps made beforehand."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


# ---- the restatement ------------------------------------------------------------------------------------------------------
def similarity(s, deg, cx, cy, mirror, S):
    """M = s R(deg), the mirror folded into the first column, the output centre (S / 2, S / 2) taken to (cx, cy): float32 (2, 3)"""
    a = math.radians(deg)
    A = np.array([[s * math.cos(a), -s * math.sin(a)], [s * math.sin(a), s * math.cos(a)]])
    if mirror:
        A[:, 0] = -A[:, 0]
    t = np.array([cx, cy], dtype=np.float64) - A @ np.array([S / 2, S / 2])
    return torch.tensor(np.concatenate([A, t[:, None]], axis=1), dtype=torch.float32)


def warp_f64(img, M, S):
    """One frame uint8 (Hs, Ws, 3) (numpy) through M float32 (2, 3): -> (float64 values (S, S, 3) before the rounding to a
    byte, (x_lo, x_hi, y_lo, y_hi): the bounding rectangle of the taps with a weight, clamped into the frame).  All output
    pixels at once, one pass per tap offset around the pixel under the centre; K covers sqrt 2 sup with room to spare."""
    Hs, Ws = img.shape[:2]
    m = M.numpy().astype(np.float64)
    u, v = m[:, 0], m[:, 1]
    e1, e2 = u / math.sqrt(u[0] * u[0] + u[1] * u[1]), v / math.sqrt(v[0] * v[0] + v[1] * v[1])
    sup = max(math.sqrt(abs(m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])), 1.0)
    o = np.arange(S, dtype=np.float64) + 0.5
    cx = (m[0, 0] * o[None, :] + m[0, 1] * o[:, None]) + m[0, 2]                 # [oy, ox]
    cy = (m[1, 0] * o[None, :] + m[1, 1] * o[:, None]) + m[1, 2]
    bx, by = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    K = int(math.ceil(1.4143 * sup)) + 1
    src = img.astype(np.float64)
    num, den = np.zeros((S, S, 3)), np.zeros((S, S))
    xs, ys = [], []
    for ky in range(-K, K + 1):
        jy = by + ky
        dy = jy + 0.5 - cy
        yc = np.clip(jy, 0, Hs - 1)
        for kx in range(-K, K + 1):
            jx = bx + kx
            dx = jx + 0.5 - cx
            w = np.maximum(0.0, 1.0 - np.abs(dx * e1[0] + dy * e1[1]) / sup) * np.maximum(0.0, 1.0 - np.abs(dx * e2[0] + dy * e2[1]) / sup)
            if not w.any():
                continue
            xc = np.clip(jx, 0, Ws - 1)
            num += w[:, :, None] * src[yc, xc]
            den += w
            xs.append(xc[w > 0]), ys.append(yc[w > 0])
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    return num / den[:, :, None], (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))


def to_bytes(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def from_half(v):
    """distance of every value from the nearest n + 1/2"""
    return np.abs(v - np.floor(v) - 0.5)


def check_against_values(got, v, band, what):
    """the kernel's bytes `got` (numpy) against the float64 values: within 1 everywhere, equal outside the band around a half,
    and at most 0.1 % of the bytes inside that band (a condition on the inputs)"""
    want = to_bytes(v)
    inside = from_half(v) <= band
    print('%s: %d of %d bytes within %g of a half; max |kernel - restatement| = %d'
          % (what, int(inside.sum()), v.size, band, int(np.abs(got.astype(np.int64) - want).max())))
    assert inside.sum() <= 0.001 * v.size
    assert np.abs(got.astype(np.int64) - want).max() <= 1
    assert np.array_equal(got[~inside], want[~inside])


def frames_of(n, Hs, Ws, seed):
    return torch.randint(0, 256, (n, Hs, Ws, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


SMALL = [(0.6875, 17, 26, 18, False), (1.37, -23, 26, 18, False), (1.0, 5, 26, 18, True), (2.3, 45, 26, 18, False),
         (1.9, 31, 2, 3, False)]                       # the last: the footprint runs over the corner, replicate is exercised
LARGE = [(4.1, -12, 100, 66, False),                   # the tile-size switch
         (7.9, 38, 100, 66, False),                    # about 250 taps
         (0.126, 61, 100, 66, False)]                  # plain bilinear


@pytest.fixture(scope='module')
def small_frames():
    return frames_of(3, 37, 53, 3753)


@pytest.fixture(scope='module')
def large_frames():
    return frames_of(2, 131, 200, 131200)


# ---- the kernel against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [16, 48])
@pytest.mark.parametrize('which', ['small', 'large'])
def test_kernel_against_float64_restatement(pkg, small_frames, large_frames, which, S):
    from istvt_amd import ops
    frames, params = (small_frames, SMALL) if which == 'small' else (large_frames, LARGE)
    n = frames.shape[0]
    dev = frames.cuda()
    for k, p in enumerate(params):
        M = torch.stack([similarity(*p, S)] * n)
        got = ops.warp_similarity_u8(dev, M, S)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, S, S, 3) and got.is_cuda and got.is_contiguous()
        assert torch.equal(ops.warp_similarity_u8(dev, M, S), got)                       # a second run: the same bits
        got = got.cpu().numpy()
        for i in range(n):
            v, _ = warp_f64(frames[i].numpy(), M[i], S)
            check_against_values(got[i], v, 1e-6, '%s frame %d, S = %d, s = %g at %g deg' % (which, i, S, p[0], p[1]))


def test_exact_cases(pkg, small_frames, large_frames):
    """the quarter turn, the mirror and the identity: one tap of weight 1 per pixel"""
    from istvt_amd import ops
    for frames, S, y0, x0 in ((small_frames, 16, 5, 7), (small_frames, 16, 21, 37), (large_frames, 48, 0, 0),
                              (large_frames, 48, 83, 152), (large_frames, 48, 40, 61)):
        n = frames.shape[0]
        sl = frames[:, y0:y0 + S, x0:x0 + S]
        dev = frames.cuda()
        for M, want in (([[0, -1, x0 + S], [1, 0, y0]], torch.rot90(sl, 1, (1, 2))),
                        ([[-1, 0, x0 + S], [0, 1, y0]], sl.flip(2)),
                        ([[1, 0, x0], [0, 1, y0]], sl)):
            M = torch.tensor([M] * n, dtype=torch.float32)
            assert torch.equal(ops.warp_similarity_u8(dev, M, S).cpu(), want), (S, y0, x0, M[0].tolist())


def test_at_the_models_side(pkg):
    """S = 224 from 500 x 317 frames: two rotated maps against the restatement, one identity against the slice"""
    from istvt_amd import ops
    S = 224
    frames = frames_of(2, 500, 317, 500317)
    dev = frames.cuda()
    for p in ((1.6, 12, 158.5, 250, False), (2.2, -8, 158.5, 250, False)):
        M = torch.stack([similarity(*p, S)] * 2)
        got = ops.warp_similarity_u8(dev, M, S).cpu().numpy()
        for i in range(2):
            v, _ = warp_f64(frames[i].numpy(), M[i], S)
            check_against_values(got[i], v, 1e-6, 'frame %d, S = 224, s = %g at %g deg' % (i, p[0], p[1]))
    ident = torch.tensor([[[1, 0, 61], [0, 1, 203]]] * 2, dtype=torch.float32)
    assert torch.equal(ops.warp_similarity_u8(dev, ident, S).cpu(), frames[:, 203:203 + S, 61:61 + S])


def test_agrees_with_the_crop_kernel_inside_the_border(pkg, small_frames):
    """square boxes as similarities: rows and columns 1 .. S - 2 within 1 of ops.crop_resize_u8, equal wherever the float64
    value is more than 1e-3 from a half (the band of the crop kernel's float32 sums)"""
    from istvt_amd import clips, ops
    S = 16
    boxes = torch.tensor([(3, 4, 11, 11), (2, 3, 30, 30), (0, 0, 37, 37)], dtype=torch.int32)
    M = clips.similarity_of_boxes(boxes, S)
    dev = small_frames.cuda()
    warp = ops.warp_similarity_u8(dev, M, S).cpu().numpy()[:, 1:S - 1, 1:S - 1]
    crop = ops.crop_resize_u8(dev, boxes, S).cpu().numpy()[:, 1:S - 1, 1:S - 1]
    assert np.abs(warp.astype(np.int64) - crop.astype(np.int64)).max() <= 1
    for i in range(3):
        v, _ = warp_f64(small_frames[i].numpy(), M[i], S)
        clear = from_half(v[1:S - 1, 1:S - 1]) > 1e-3
        print('box %s: %d of %d bytes compared for equality' % (boxes[i].tolist(), int(clear.sum()), clear.size))
        assert np.array_equal(warp[i][clear], crop[i][clear])


def test_independence(pkg, small_frames, large_frames):
    """the bytes outside the clamped footprint rectangle do not show; nor does where the source starts in its allocation"""
    from istvt_amd import ops
    for frames, p, S in ((small_frames, SMALL[0], 16), (small_frames, SMALL[4], 16), (large_frames, LARGE[0], 16),
                         (large_frames, LARGE[1], 12)):                                 # 8 x 8 tiles, the last ones partial
        n = frames.shape[0]
        M = torch.stack([similarity(*p, S)] * n)
        ref = ops.warp_similarity_u8(frames.cuda(), M, S)
        _, (x_lo, x_hi, y_lo, y_hi) = warp_f64(frames[0].numpy(), M[0], S)
        assert (x_hi - x_lo + 1) * (y_hi - y_lo + 1) < frames.shape[1] * frames.shape[2]  # there is something outside
        other = 255 - frames
        other[:, y_lo:y_hi + 1, x_lo:x_hi + 1] = frames[:, y_lo:y_hi + 1, x_lo:x_hi + 1]
        assert not torch.equal(other, frames)
        assert torch.equal(ops.warp_similarity_u8(other.cuda(), M, S), ref), p
        assert torch.equal(ops.warp_similarity_u8(frames.cuda()[1:], M[1:], S), ref[1:])  # mid-allocation
        store = torch.empty((frames.numel() + 7,), dtype=torch.uint8, device='cuda')
        odd = store[7:].view(frames.shape)
        odd.copy_(frames)
        assert odd.data_ptr() % 2 == 1
        assert torch.equal(ops.warp_similarity_u8(odd, M, S), ref)
        out = torch.full((n, S, S, 3), 99, dtype=torch.uint8, device='cuda')
        assert ops.warp_similarity_u8(frames.cuda(), M, S, out=out) is out and torch.equal(out, ref)


def test_clips_take_one_map_each(pkg):
    from istvt_amd import clips, ops
    S = 16
    u8 = frames_of(6, 37, 53, 23).reshape(2, 3, 37, 53, 3).cuda()
    M = torch.stack([similarity(*SMALL[1], S), similarity(*SMALL[2], S)])
    got = ops.warp_similarity_u8(u8, M, S)
    assert tuple(got.shape) == (2, 3, S, S, 3)
    assert torch.equal(got.reshape(6, S, S, 3), ops.warp_similarity_u8(u8.reshape(6, 37, 53, 3), clips.per_frame_similarities(M, 3), S))


def test_argument_errors(pkg, small_frames):
    from istvt_amd import ops
    dev = small_frames.cuda()
    M = torch.stack([similarity(*SMALL[0], 16)] * 3)
    with pytest.raises(ValueError):
        ops.warp_similarity_u8(dev, M, 481)
    with pytest.raises(TypeError):
        ops.warp_similarity_u8(dev.float(), M, 16)
    with pytest.raises(ValueError):
        ops.warp_similarity_u8(dev, M[:2], 16)
    with pytest.raises(IndexError):
        ops.warp_similarity_u8(dev, torch.stack([similarity(1.0, 0, 60, 18, False, 16)] * 3), 16)
    with pytest.raises(RuntimeError):
        ops.warp_similarity_u8(dev, M, 16, checked=True)                                 # a checked table lives on the device
    with pytest.raises(RuntimeError):
        ops.warp_similarity_u8(dev, M, 16, out=torch.empty((3, 16, 16, 3), dtype=torch.uint8))


# ---- NV12 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('matrix', ['bt601', 'bt709', 'jfif'])
def test_nv12_is_the_warp_of_the_converted_frames(pkg, matrix):
    from istvt_amd import clips, ops
    for (Hs, Ws, seed), params, S in (((38, 54, 1), SMALL, 16), ((130, 200, 2), LARGE, 48), ((130, 200, 3), SMALL[:2], 16)):
        nv = clips.rgb_to_nv12_host(frames_of(2, Hs, Ws, seed), matrix)
        rows = Hs + Hs // 2
        pitch = Ws + 10                                                              # a padded pitch, through as_strided
        store = torch.full((5 + 2 * rows * pitch + 64,), 77, dtype=torch.uint8, device='cuda')
        surf = store.as_strided((2, rows, Ws), (rows * pitch, pitch, 1), 5)
        surf.copy_(nv)
        rgb = ops.nv12_to_rgb_u8(nv.cuda(), matrix)
        for p in params:
            M = torch.stack([similarity(*p, S)] * 2)
            want = ops.warp_similarity_u8(rgb, M, S)
            assert torch.equal(ops.warp_similarity_nv12(nv.cuda(), M, S, matrix), want), (Hs, Ws, p)
            assert torch.equal(ops.warp_similarity_nv12(surf, M, S, matrix), want), (Hs, Ws, p, 'pitched')
    four = nv.cuda().reshape(1, 2, rows, Ws)                                         # clips: one map for both frames
    assert torch.equal(ops.warp_similarity_nv12(four, M[:1], S, matrix).reshape(2, S, S, 3), want)


# ---- a table that was not validated ---------------------------------------------------------------------------------------
def test_unvalidated_table(pkg, small_frames):
    """checked=True with entries the kernel itself refuses: those frames are zeros, the others what the validated call gives"""
    from istvt_amd import clips, ops
    S = 16
    dev = small_frames.cuda()
    M = torch.stack([similarity(*SMALL[0], S), similarity(*SMALL[3], S), similarity(*SMALL[4], S)])
    ref = ops.warp_similarity_u8(dev, M, S)
    nv = clips.rgb_to_nv12_host(small_frames[:, :36, :52].contiguous(), 'bt709').cuda()
    ref_nv = ops.warp_similarity_nv12(nv, M, S)
    for bad in (lambda m: m[0].__setitem__(2, float('nan')), lambda m: m[1].__setitem__(0, float('inf')),
                lambda m: m.mul_(5.0),                                                   # s = 11.5
                lambda m: m[:, :2].mul_(0.001),                                          # s = 0.0023
                lambda m: m[0].__setitem__(2, 1.0e6)):                                   # the centre far outside
        t = M.clone()
        bad(t[1])
        got = ops.warp_similarity_u8(dev, t.cuda(), S, checked=True)
        assert int(got[1].max()) == 0 and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
        got = ops.warp_similarity_nv12(nv, t.cuda(), S, checked=True)
        assert int(got[1].max()) == 0 and torch.equal(got[0], ref_nv[0]) and torch.equal(got[2], ref_nv[2])


# ---- the scorer -------------------------------------------------------------------------------------------------------------
SIDE = 96


@pytest.fixture(scope='module')
def aligned(pkg):
    """the tiny configuration of the video tests: T = 4, side 96, depth 2, float32, a seeded random model in eval mode; 11
    frames of 140 x 170 with one similarity each (s 0.7 .. 1.4, within 25 degrees, some mirrored) and a second video of 7
    frames of 120 x 200; the same pictures as NV12 (other bytes: the encoder is lossy)"""
    from istvt_amd import clips, ops
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

    def video(n, Hs, Ws, seed):
        u8 = frames_of(n, Hs, Ws, seed)
        r = torch.rand((n, 5), generator=g).tolist()
        M = torch.stack([similarity(0.7 + 0.7 * a, 50 * b - 25, Ws * (0.4 + 0.2 * c), Hs * (0.4 + 0.2 * d), e < 0.3, SIDE)
                         for a, b, c, d, e in r])
        nv = clips.rgb_to_nv12_host(u8, 'bt709')
        return dict(u8=u8, M=M, crops=ops.warp_similarity_u8(u8.cuda(), M, SIDE), nv=nv,
                    nv_crops=ops.warp_similarity_nv12(nv.cuda(), M, SIDE, 'bt709'))

    return dict(model=model, a=video(11, 140, 170, 22), b=video(7, 120, 200, 23))


@pytest.mark.parametrize('fmt', ['rgb24', 'nv12'])
def test_score_explain_and_score_videos_are_those_on_the_warps(aligned, fmt):
    from istvt_amd import video
    model, a, b = aligned['model'], aligned['a'], aligned['b']
    frames, crops = ('u8', 'crops') if fmt == 'rgb24' else ('nv', 'nv_crops')
    plain = video.VideoScorer(model, frame_batch=4, window_batch=3, side=SIDE)
    scorer = video.VideoScorer(model, frame_batch=4, window_batch=3, side=SIDE, pixel_format=fmt)
    ref = plain.score(a[crops])
    for x in (a[frames], a[frames].cuda()):                                          # host frames and device frames
        res = scorer.score(x, transforms=a['M'])
        assert torch.isfinite(res.window_logits).all() and res.starts.tolist() == ref.starts.tolist()
        assert torch.equal(res.window_logits, ref.window_logits)
        assert torch.equal(res.logit_mean, ref.logit_mean) and torch.equal(res.prob_mean, ref.prob_mean)
    res = model.score_video(a[frames], transforms=a['M'], frame_batch=4, window_batch=3, side=SIDE, pixel_format=fmt)
    assert torch.equal(res.window_logits, ref.window_logits)
    # explain: the maps are in crop coordinates
    exr, ex = plain.explain(a[crops]), scorer.explain(a[frames], transforms=a['M'])
    assert float(exr.frame_s.abs().max()) > 0
    for name in ('frame_s', 'frame_t', 'frame_weight', 'frame_logit', 'count'):
        assert torch.equal(getattr(ex, name), getattr(exr, name)), name
    assert torch.equal(ex.score.window_logits, exr.score.window_logits)
    # a set: the same plan on the warps
    res = scorer.score_videos([a[frames], b[frames].cuda()], transforms=[a['M'], b['M']], labels=[1, 0])
    ref = plain.score_videos([a[crops], b[crops]], labels=[1, 0])
    for i in range(6):
        assert torch.equal(res[i], ref[i]), video.VideoSetScore._fields[i]
    assert res.metrics is not None
    res = model.score_videos([a[frames], b[frames]], transforms=[a['M'], b['M']], frame_batch=4, window_batch=3, side=SIDE,
                             pixel_format=fmt)
    assert torch.equal(res.window_logits, ref.window_logits)


def test_push_in_two_chunks_agrees_with_score(aligned):
    from istvt_amd import video
    a = aligned['a']
    scorer = video.VideoScorer(aligned['model'], frame_batch=4, side=SIDE)
    ref = scorer.score(a['u8'], transforms=a['M'])
    outs, starts = [], []
    for lo, hi in ((0, 4), (4, 11)):                                                 # two uneven chunks
        l, s = scorer.push(a['u8'][lo:hi], transforms=a['M'][lo:hi].contiguous())
        outs.append(l), starts.extend(s.tolist())
    l, s = scorer.flush()
    outs.append(l), starts.extend(s.tolist())
    assert starts == ref.starts.tolist()
    d = float((torch.cat(outs) - ref.window_logits).abs().max())
    print('push 4 + 7 of aligned frames vs score: max abs diff %.3e' % d)
    assert d <= 1e-5
    with pytest.raises(ValueError, match='stream'):                                  # a stream keeps one mode
        scorer.push(a['u8'][:4], boxes=torch.tensor([[0, 0, 96, 96]] * 4, dtype=torch.int32))
    scorer.reset()


def test_jpeg_quality_composes(aligned):
    from istvt_amd import ops, video
    a = aligned['a']
    plain = video.VideoScorer(aligned['model'], frame_batch=4, side=SIDE)
    ref = plain.score(ops.jpeg_roundtrip_u8(a['crops'], 40))
    res = video.VideoScorer(aligned['model'], frame_batch=4, side=SIDE, jpeg_quality=40).score(a['u8'], transforms=a['M'])
    assert torch.equal(res.window_logits, ref.window_logits)
    assert not torch.equal(res.window_logits, plain.score(a['crops']).window_logits)
    ref = plain.score(ops.jpeg_roundtrip_u8(a['nv_crops'], 40))
    res = video.VideoScorer(aligned['model'], frame_batch=4, side=SIDE, jpeg_quality=40, pixel_format='nv12').score(
        a['nv'], transforms=a['M'])
    assert torch.equal(res.window_logits, ref.window_logits)
