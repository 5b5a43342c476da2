"""Frames and boxes (DESIGN.md "Frames and boxes") without a device: the tap table against torch's antialiased
interpolate, the host definition, the box validation, the random boxes and the scorer's argument errors."""
import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _resize64(img, S):
    """float64 (h, w, 3) -> (S, S, 3) through clips.resize_weights, horizontal pass first"""
    from istvt_amd import clips
    h, w = img.shape[:2]
    xl, xn, xw = clips.resize_weights(w, S)
    yl, yn, yw = clips.resize_weights(h, S)
    assert xw.dtype == torch.float64 and int(xn.max()) == xw.shape[1] <= 17 and int(yn.max()) == yw.shape[1] <= 17
    xi = (xl[:, None] + torch.arange(xw.shape[1])[None]).clamp(max=w - 1)
    yi = (yl[:, None] + torch.arange(yw.shape[1])[None]).clamp(max=h - 1)
    hor = (img[:, xi, :] * xw[None, :, :, None]).sum(2)
    return (hor[yi] * yw[:, :, None, None]).sum(1)


@pytest.mark.parametrize('h,w,S', [(37, 53, 16), (16, 16, 16), (11, 9, 16), (97, 64, 32), (31, 200, 48)])
def test_resize_weights_against_interpolate(pkg, h, w, S):
    g = torch.Generator().manual_seed(h * 1000 + w)
    img = torch.rand((h, w, 3), generator=g, dtype=torch.float64) * 255
    ref = F.interpolate(img.permute(2, 0, 1)[None], size=(S, S), mode='bilinear', align_corners=False, antialias=True)
    ref = ref[0].permute(1, 2, 0)
    d = float((_resize64(img, S) - ref).abs().max())
    print('%d x %d -> %d: max |recipe - interpolate| = %.3e' % (h, w, S, d))
    assert d < 1e-9


def test_resize_weights_rows(pkg):
    from istvt_amd import clips
    for n_in, n_out in ((16, 16), (9, 16), (128, 16), (1, 16), (53, 48)):
        lo, cnt, w = clips.resize_weights(n_in, n_out)
        assert float((w.sum(1) - 1).abs().max()) < 1e-15 and bool((w >= 0).all())
        assert int(lo.min()) >= 0 and int((lo + cnt).max()) <= n_in and int(cnt.min()) >= 1
        assert all(float(w[i, int(cnt[i]):].abs().sum()) == 0.0 for i in range(n_out))
    lo, cnt, w = clips.resize_weights(16, 16)
    assert lo.tolist() == list(range(16)) and torch.equal(w[:, 0], torch.ones(16, dtype=torch.float64))
    assert float(w[:, 1:].abs().sum()) == 0.0
    assert max(int(clips.resize_weights(n_in, 16)[1].max()) for n_in in range(97, 129)) <= 17      # the limit h, w <= 8 S


def test_host_identity_box_is_the_slice(pkg):
    from istvt_amd import clips
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (3, 37, 53, 3), generator=g, dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 16, 16], [21, 37, 16, 16], [5, 11, 16, 16]], dtype=torch.int32)
    out = clips.crop_resize_host(u8, boxes, 16)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, 16, 16, 3)
    for i, (y0, x0, h, w) in enumerate(boxes.tolist()):
        assert torch.equal(out[i], u8[i, y0:y0 + h, x0:x0 + w])


def test_host_matches_interpolate_and_clips(pkg):
    """the float32 host definition stays within one byte of the float64 interpolate; a (B, 4) table spreads over T"""
    from istvt_amd import clips
    g = torch.Generator().manual_seed(4)
    u8 = torch.randint(0, 256, (2, 2, 40, 61, 3), generator=g, dtype=torch.uint8)
    boxes = torch.tensor([[3, 7, 30, 41], [0, 50, 9, 11]], dtype=torch.int32)
    out = clips.crop_resize_host(u8, boxes, 16)
    assert tuple(out.shape) == (2, 2, 16, 16, 3)
    for b in range(2):
        y0, x0, h, w = boxes[b].tolist()
        for t in range(2):
            img = u8[b, t, y0:y0 + h, x0:x0 + w].to(torch.float64).permute(2, 0, 1)[None]
            ref = F.interpolate(img, size=(16, 16), mode='bilinear', align_corners=False, antialias=True)[0].permute(1, 2, 0)
            ref = torch.floor(ref + 0.5).clamp(0, 255)
            assert int((out[b, t].to(torch.float64) - ref).abs().max()) <= 1
    flat = clips.crop_resize_host(u8.reshape(4, 40, 61, 3), clips.per_frame_boxes(boxes, 2), 16)
    assert torch.equal(flat, out.reshape(4, 16, 16, 3))


def test_check_boxes_refusals(pkg):
    from istvt_amd import clips
    ok = torch.tensor([[0, 0, 37, 53], [36, 52, 1, 1]], dtype=torch.int32)
    assert torch.equal(clips.check_boxes(ok, 2, 37, 53, 16), ok)

    def bad(row):
        return torch.tensor([[0, 0, 10, 10], row], dtype=torch.int32)

    for row in ([-1, 0, 10, 10], [0, -1, 10, 10], [30, 0, 8, 10], [0, 45, 10, 9]):      # top, left, bottom, right
        with pytest.raises(IndexError):
            clips.check_boxes(bad(row), 2, 37, 53, 16)
    with pytest.raises(ValueError):
        clips.check_boxes(bad([0, 0, 0, 10]), 2, 37, 53, 16)                            # h = 0
    with pytest.raises(ValueError):
        clips.check_boxes(bad([0, 0, 10, 33]), 2, 37, 53, 4)                            # w > 8 S
    assert clips.check_boxes(bad([0, 0, 10, 32]), 2, 37, 53, 4) is not None
    with pytest.raises(TypeError):
        clips.check_boxes(ok.to(torch.int64), 2, 37, 53, 16)
    with pytest.raises(TypeError):
        clips.check_boxes(ok.tolist(), 2, 37, 53, 16)
    with pytest.raises(ValueError):
        clips.check_boxes(ok, 3, 37, 53, 16)                                            # row count
    with pytest.raises(ValueError):
        clips.check_boxes(ok[:, :3], 2, 37, 53, 16)
    with pytest.raises(IndexError):
        clips.crop_resize_host(torch.zeros((2, 37, 53, 3), dtype=torch.uint8), bad([30, 0, 8, 10]), 16)


def test_random_boxes_bounds_and_seed(pkg):
    from istvt_amd import clips
    Hs, Ws = 270, 480
    scale, ratio = (0.5, 1.0), (3 / 4, 4 / 3)
    a = clips.random_boxes(500, Hs, Ws, scale, ratio, generator=torch.Generator().manual_seed(7))
    b = clips.random_boxes(500, Hs, Ws, scale, ratio, generator=torch.Generator().manual_seed(7))
    assert a.dtype == torch.int32 and tuple(a.shape) == (500, 4) and torch.equal(a, b)
    assert not torch.equal(a, clips.random_boxes(500, Hs, Ws, scale, ratio, generator=torch.Generator().manual_seed(8)))
    clips.check_boxes(a, 500, Hs, Ws, 224)                                  # inside the frame
    y0, x0, h, w = (a[:, i].to(torch.float64) for i in range(4))
    # sides are rounded to whole pixels (half a pixel each) and cut to the frame: an uncut box keeps its area and aspect
    # within that rounding, a cut one only loses area
    side = float(min(Hs, Ws))
    area = h * w
    slack = 0.5 * (h + w) + 1.0
    assert bool((area <= scale[1] * side * side + slack).all())
    uncut = (h < Hs) & (w < Ws)
    assert int(uncut.sum()) > 100
    assert bool((area[uncut] >= scale[0] * side * side - slack[uncut]).all())
    assert bool(((w[uncut] + 0.5) / (h[uncut] - 0.5) >= ratio[0]).all())
    assert bool(((w[uncut] - 0.5) / (h[uncut] + 0.5) <= ratio[1]).all())
    assert len(torch.unique(h)) > 20 and len(torch.unique(x0)) > 20
    with pytest.raises(ValueError):
        clips.random_boxes(4, Hs, Ws, scale=(0.0, 1.0))
    with pytest.raises(ValueError):
        clips.random_boxes(4, Hs, Ws, ratio=(2.0, 1.0))


def test_scorer_argument_errors_need_no_device(pkg):
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    assert model.crop_side is None
    frames = torch.zeros((5, 40, 50, 3), dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 30, 30]] * 5, dtype=torch.int32)
    scorer = video.VideoScorer(model)
    for call in (lambda: scorer.score(frames, boxes=boxes), lambda: scorer.push(frames, boxes=boxes),
                 lambda: scorer.explain(frames, boxes=boxes), lambda: model.score_video(frames, boxes=boxes),
                 lambda: model.explain_video(frames, boxes=boxes)):
        with pytest.raises(ValueError, match='side'):
            call()
    sided = video.VideoScorer(model, side=32)
    assert sided.side == 32
    with pytest.raises(ValueError, match='uint8'):
        sided.score(torch.zeros((5, 3, 40, 50)), boxes=boxes)                # float frames
    with pytest.raises(ValueError, match='uint8'):
        sided.push(torch.zeros((5, 3, 32, 32)), boxes=boxes)
    with pytest.raises(IndexError):
        sided.score(frames, boxes=torch.tensor([[20, 0, 30, 30]] * 5, dtype=torch.int32))
    with pytest.raises(ValueError):
        sided.score(frames, boxes=boxes[:4])
    with pytest.raises(ValueError):
        video.VideoScorer(model, side=2)
    model.set_crop_side(32)                                                  # the model's side is the default
    with pytest.raises(RuntimeError, match='ROCm'):                          # the arguments pass: the next stop is the device
        video.VideoScorer(model).score(frames, boxes=boxes)
