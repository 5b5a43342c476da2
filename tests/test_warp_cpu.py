"""Aligned crops (DESIGN.md "Aligned crops") without a device: the three properties of the definition
(clips.warp_similarity_host), the landmark fit, the validation of a table, the random tables and the scorer's argument
errors."""
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


S = 16
BOXES = [(3, 4, 11, 11), (5, 7, 16, 16), (2, 3, 30, 30), (0, 0, 37, 37)]        # (y0, x0, h, w) inside 37 x 53


@pytest.fixture(scope='module')
def frame():
    g = torch.Generator().manual_seed(1903)
    return torch.randint(0, 256, (1, 37, 53, 3), generator=g, dtype=torch.uint8)


def _axis_weights(n_in, n_out):
    """crop_resize's taps of one axis as a dense float64 matrix (n_out, n_in), restated from its definition"""
    W = np.zeros((n_out, n_in), dtype=np.float64)
    scale = n_in / n_out
    sup = max(scale, 1.0)
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
        w = np.array([max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)], dtype=np.float64)
        W[i, lo:hi] = w / w.sum()
    return W


def _crop_resize_f64(img, box, n_out):
    """float64 values (before rounding to a byte) of crop_resize on one frame"""
    y0, x0, h, w = box
    crop = img[y0:y0 + h, x0:x0 + w].astype(np.float64)
    return np.einsum('ys,xt,stc->yxc', _axis_weights(h, n_out), _axis_weights(w, n_out), crop)


def _warp_f64(img, M, n_out):
    """float64 values of the warp on one frame, restated from the definition with plain loops over a generous tap range"""
    Hs, Ws = img.shape[:2]
    m = np.asarray(M, dtype=np.float64)
    u, v = m[:, 0], m[:, 1]
    e1, e2 = u / np.linalg.norm(u), v / np.linalg.norm(v)
    sup = max(math.sqrt(abs(m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0])), 1.0)
    K = int(math.ceil(1.5 * sup)) + 2
    out = np.zeros((n_out, n_out, 3), dtype=np.float64)
    src = img.astype(np.float64)
    for oy in range(n_out):
        for ox in range(n_out):
            cx = m[0, 0] * (ox + .5) + m[0, 1] * (oy + .5) + m[0, 2]
            cy = m[1, 0] * (ox + .5) + m[1, 1] * (oy + .5) + m[1, 2]
            jx = np.arange(int(math.floor(cx)) - K, int(math.floor(cx)) + K + 1)
            jy = np.arange(int(math.floor(cy)) - K, int(math.floor(cy)) + K + 1)
            dx, dy = (jx + .5 - cx)[None, :], (jy + .5 - cy)[:, None]
            w = np.maximum(0.0, 1.0 - np.abs(dx * e1[0] + dy * e1[1]) / sup) * np.maximum(0.0, 1.0 - np.abs(dx * e2[0] + dy * e2[1]) / sup)
            px = src[np.clip(jy, 0, Hs - 1)[:, None], np.clip(jx, 0, Ws - 1)[None, :]]
            out[oy, ox] = (w[:, :, None] * px).sum((0, 1)) / w.sum()
    return out


@pytest.mark.parametrize('box', BOXES)
def test_agrees_with_crop_resize_inside_the_border(pkg, frame, box):
    """M = [[s, 0, x0], [0, s, y0]]: rows and columns 1 .. S - 2 carry crop_resize's float64 values (to 1e-9), and the bytes
    of the definition are those values rounded"""
    from istvt_amd import clips
    img = frame[0].numpy()
    M = clips.similarity_of_boxes(torch.tensor([box], dtype=torch.int32), S)
    y0, x0, h, w = box
    assert M.dtype == torch.float32 and M[0].tolist() == [[h / S, 0.0, float(x0)], [0.0, h / S, float(y0)]]
    want = _crop_resize_f64(img, box, S)
    got = _warp_f64(img, M[0].numpy(), S)
    err = float(np.abs(got - want)[1:S - 1, 1:S - 1].max())
    print('box %s: max |warp - crop_resize| inside the border = %.3g' % (box, err))
    assert err <= 1e-9
    out = clips.warp_similarity_host(frame, M, S)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, S, S, 3)
    near_half = np.abs(got - np.floor(got) - 0.5) < 1e-9
    ref = np.clip(np.floor(got + 0.5), 0, 255).astype(np.uint8)
    assert np.array_equal(out[0].numpy()[~near_half], ref[~near_half])


@pytest.mark.parametrize('y0,x0', [(5, 7), (0, 0), (21, 37)])
def test_quarter_turn_mirror_and_identity_are_exact(pkg, frame, y0, x0):
    from istvt_amd import clips
    img = frame[0].numpy()
    sl = img[y0:y0 + S, x0:x0 + S]
    turn = torch.tensor([[[0, -1, x0 + S], [1, 0, y0]]], dtype=torch.float32)
    assert np.array_equal(clips.warp_similarity_host(frame, turn, S)[0].numpy(), np.rot90(sl, 1))
    mirror = torch.tensor([[[-1, 0, x0 + S], [0, 1, y0]]], dtype=torch.float32)
    assert np.array_equal(clips.warp_similarity_host(frame, mirror, S)[0].numpy(), sl[:, ::-1])
    ident = torch.tensor([[[1, 0, x0], [0, 1, y0]]], dtype=torch.float32)
    assert np.array_equal(clips.warp_similarity_host(frame, ident, S)[0].numpy(), sl)


def test_rotated_definition_against_loops_and_clips(pkg):
    """a rotated, downscaling map near the corner (the border is replicated) against the plain-loop restatement; a (B, T)
    batch equals the flat call on per_frame_similarities"""
    from istvt_amd import clips
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (2, 3, 37, 53, 3), generator=g, dtype=torch.uint8)
    M = torch.stack([_similarity(1.9, 31, 2, 3, False, 8), _similarity(0.6875, -17, 26, 18, True, 8)])
    out = clips.warp_similarity_host(u8, M, 8)
    assert tuple(out.shape) == (2, 3, 8, 8, 3)
    flat = clips.warp_similarity_host(u8.reshape(6, 37, 53, 3), clips.per_frame_similarities(M, 3), 8)
    assert torch.equal(out.reshape(6, 8, 8, 3), flat)
    for b in range(2):
        v = _warp_f64(u8[b, 1].numpy(), M[b].numpy(), 8)
        keep = np.abs(v - np.floor(v) - 0.5) > 1e-9
        assert np.array_equal(out[b, 1].numpy()[keep], np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)[keep])


def _similarity(s, deg, cx, cy, mirror, n_out):
    """M = s R(deg), the mirror folded into the first column, the output centre taken to (cx, cy); float32 (2, 3)"""
    a = math.radians(deg)
    A = np.array([[s * math.cos(a), -s * math.sin(a)], [s * math.sin(a), s * math.cos(a)]])
    if mirror:
        A[:, 0] = -A[:, 0]
    t = np.array([cx, cy]) - A @ np.array([n_out / 2, n_out / 2])
    return torch.tensor(np.concatenate([A, t[:, None]], axis=1), dtype=torch.float32)


def test_landmarks_recover_a_known_similarity(pkg):
    from istvt_amd import clips
    template = torch.tensor([[38.3, 51.7], [73.5, 51.5], [56.0, 71.7], [41.5, 92.4], [70.7, 92.2]], dtype=torch.float64)
    s, ang, t = 2.35, math.radians(-14.0), np.array([301.25, 177.5])
    A = np.array([[s * math.cos(ang), -s * math.sin(ang)], [s * math.sin(ang), s * math.cos(ang)]])
    marks = torch.tensor(template.numpy() @ A.T + t)[None]
    M = clips.similarity_from_landmarks(marks, template, 112)
    assert M.dtype == torch.float32 and tuple(M.shape) == (1, 2, 3)
    m = M[0].double().numpy()
    assert abs(math.hypot(m[0, 0], m[1, 0]) - s) <= 1e-5 and abs(math.atan2(m[1, 0], m[0, 0]) - ang) <= 1e-5
    assert np.abs(m[:, :2] - A).max() <= 1e-5 and np.abs(m[:, 2] - t).max() <= 1e-4      # float32 carries 301.25 to 3e-5
    shift = torch.tensor([12.5, -7.25], dtype=torch.float64)
    M2 = clips.similarity_from_landmarks(marks + shift, template)[0].double().numpy()
    assert np.array_equal(M2[:, :2], m[:, :2])
    assert np.abs(M2[:, 2] - m[:, 2] - shift.numpy()).max() <= 1e-4
    # a least-squares fit of noisy points keeps the centroids on each other
    g = torch.Generator().manual_seed(3)
    noisy = marks + 0.8 * torch.randn((1, 5, 2), generator=g, dtype=torch.float64)
    mn = clips.similarity_from_landmarks(noisy, template)[0].double().numpy()
    assert abs(mn[0, 0] - mn[1, 1]) <= 1e-6 and abs(mn[0, 1] + mn[1, 0]) <= 1e-6         # no shear, no reflection
    assert np.abs(mn[:, :2] @ template.mean(0).numpy() + mn[:, 2] - noisy[0].mean(0).numpy()).max() <= 1e-3
    with pytest.raises(ValueError):
        clips.similarity_from_landmarks(marks[:, :1], template[:1])                      # K = 1
    with pytest.raises(ValueError):
        clips.similarity_from_landmarks(marks, template[:1].repeat(5, 1))                # the template's points coincide
    with pytest.raises(ValueError):
        clips.similarity_from_landmarks(marks, template, 64)                             # outside a 64 x 64 crop


def test_check_similarities_raises_each_error(pkg):
    from istvt_amd import clips
    ok = torch.stack([_similarity(1.5, 20, 26, 18, False, S), _similarity(0.5, -100, 3, 30, True, S)])
    assert torch.equal(clips.check_similarities(ok, 2, 37, 53, S), ok)
    with pytest.raises(TypeError):
        clips.check_similarities(ok.double(), 2, 37, 53, S)
    with pytest.raises(TypeError):
        clips.check_similarities(ok.tolist(), 2, 37, 53, S)
    for bad in (ok[:1], ok.reshape(2, 3, 2), ok.reshape(2, 6)):
        with pytest.raises(ValueError):
            clips.check_similarities(bad, 2, 37, 53, S)

    def one(edit):
        m = ok.clone()
        edit(m)
        return m

    with pytest.raises(ValueError, match='finite'):
        clips.check_similarities(one(lambda m: m[1, 0].__setitem__(2, float('nan'))), 2, 37, 53, S)
    with pytest.raises(ValueError, match='finite'):
        clips.check_similarities(one(lambda m: m[0, 1].__setitem__(1, float('inf'))), 2, 37, 53, S)
    with pytest.raises(ValueError, match='affine'):
        clips.check_similarities(one(lambda m: m[0, 0].__setitem__(1, m[0, 0, 1] + 0.3)), 2, 37, 53, S)      # shear
    with pytest.raises(ValueError, match='affine'):
        clips.check_similarities(one(lambda m: m[0, :, 0].mul_(1.01)), 2, 37, 53, S)                         # two scales
    with pytest.raises(ValueError, match='scale'):
        clips.check_similarities(torch.stack([ok[0], _similarity(8.5, 0, 26, 18, False, S)]), 2, 37, 53, S)
    with pytest.raises(ValueError, match='scale'):
        clips.check_similarities(torch.stack([ok[0], _similarity(0.01, 0, 26, 18, False, S)]), 2, 37, 53, S)
    with pytest.raises(IndexError):
        clips.check_similarities(torch.stack([ok[0], _similarity(1.0, 0, 54, 18, False, S)]), 2, 37, 53, S)
    with pytest.raises(IndexError):
        clips.check_similarities(torch.stack([ok[0], _similarity(1.0, 0, 26, -0.5, False, S)]), 2, 37, 53, S)
    clips.check_similarities(torch.stack([ok[0], _similarity(8.0, 0, 53, 37, False, S)]), 2, 37, 53, S)      # the limits pass


def test_similarity_of_boxes_refuses_rectangles(pkg):
    from istvt_amd import clips
    with pytest.raises(ValueError):
        clips.similarity_of_boxes(torch.tensor([[0, 0, 11, 11], [1, 2, 11, 12]], dtype=torch.int32), S)
    with pytest.raises(TypeError):
        clips.similarity_of_boxes(torch.tensor([[0, 0, 11, 11]]), S)


def test_random_similarities(pkg):
    from istvt_amd import clips
    a = clips.random_similarities(64, 270, 480, 224, generator=torch.Generator().manual_seed(5))
    b = clips.random_similarities(64, 270, 480, 224, generator=torch.Generator().manual_seed(5))
    assert a.dtype == torch.float32 and tuple(a.shape) == (64, 2, 3) and a.is_contiguous() and torch.equal(a, b)
    assert not torch.equal(a, clips.random_similarities(64, 270, 480, 224, generator=torch.Generator().manual_seed(6)))
    clips.check_similarities(a, 64, 270, 480, 224)
    m = a.double()
    det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
    assert bool((det < 0).any()) and bool((det > 0).any())                                # mirrors, folded into M
    side = det.abs().sqrt() * 224
    assert float(side.min()) >= math.sqrt(0.5) * 270 - 1 and float(side.max()) <= 270 + 1e-3
    ang = torch.atan2(-m[:, 0, 1], m[:, 1, 1])                                            # v = s (-sin, cos)
    assert float(ang.abs().max()) <= math.radians(10.0) + 1e-6
    # where it fits (a side of at most sqrt(0.6) * 270 = 209, turned by 10 degrees, spans 241 < 270) the rotated source square
    # stays inside the frame: the images of the crop's four corners
    fit = clips.random_similarities(64, 270, 480, 224, scale=(0.3, 0.6), generator=torch.Generator().manual_seed(8)).double()
    cor = torch.tensor([[0.0, 0.0, 1.0], [224.0, 0.0, 1.0], [0.0, 224.0, 1.0], [224.0, 224.0, 1.0]], dtype=torch.float64)
    pts = torch.einsum('nij,kj->nki', fit, cor)
    assert float(pts.min()) >= -1e-3 and float(pts[..., 0].max()) <= 480 + 1e-3 and float(pts[..., 1].max()) <= 270 + 1e-3
    flat = clips.random_similarities(16, 100, 80, 32, degrees=0.0, flip_p=0.0, generator=torch.Generator().manual_seed(1))
    assert bool((flat[:, 0, 1] == 0).all()) and bool((flat[:, 1, 0] == 0).all())          # axis-aligned
    assert bool((flat[:, 0, 0] > 0).all()) and torch.equal(flat[:, 0, 0], flat[:, 1, 1])
    clips.check_similarities(flat, 16, 100, 80, 32)
    small = clips.random_similarities(8, 40, 40, 32, scale=(1.0, 1.0), degrees=45.0, generator=torch.Generator().manual_seed(2))
    clips.check_similarities(small, 8, 40, 40, 32)                                        # no room: the frame's centre
    c = small.double() @ torch.tensor([16.0, 16.0, 1.0], dtype=torch.float64)
    assert float((c - 20.0).abs().max()) <= 1e-4
    # where the side is cut to a limit of the scale (8 S from large frames, S / 64 from tiny ones) the float32 table still
    # passes: the side is kept 1e-6 inside, more than the rounding of s cos and s sin (6e-8) can move sqrt |det|
    for args, kw, limit in (((256, 1080, 1920, 96), {}, 8.0), ((256, 1080, 1920, 112), {}, 8.0),
                            ((256, 64, 64, 480), dict(scale=(0.005, 0.01)), 2.0 ** -6),
                            ((64, 2160, 3840, 224), dict(degrees=180.0), 8.0)):
        for seed in (1, 2):
            t = clips.random_similarities(*args, generator=torch.Generator().manual_seed(seed), **kw)
            clips.check_similarities(t, args[0], args[1], args[2], args[3])
            d = t.double()
            sc = (d[:, 0, 0] * d[:, 1, 1] - d[:, 0, 1] * d[:, 1, 0]).abs().sqrt()
            cut = ((sc - limit).abs() <= 2e-6 * limit)
            print('%s %s: %d of %d entries cut to s = %g' % (args, kw, int(cut.sum()), args[0], limit))
            assert int(cut.sum()) >= args[0] // 4                                        # the cut is active in these cases
    edge = clips.similarities_of_squares(torch.tensor([8.0 * 96, 96 / 64.0, 1.0e9, 0.0]), torch.tensor([0.3, -2.0, 1.0, 0.1]),
                                         torch.full((4,), 500.0), torch.full((4,), 400.0), torch.tensor([0, 1, 1, 0]), 96)
    clips.check_similarities(edge, 4, 1080, 1920, 96)
    with pytest.raises(ValueError):
        clips.random_similarities(0, 40, 40, 32)
    with pytest.raises(ValueError):
        clips.random_similarities(4, 40, 40, 32, scale=(0.0, 1.0))


def test_scorer_argument_errors_need_no_device(pkg):
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    rgb = torch.zeros((5, 40, 50, 3), dtype=torch.uint8)
    nv = torch.zeros((5, 60, 50), dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 30, 30]] * 5, dtype=torch.int32)
    M = torch.stack([_similarity(0.9, 10, 25, 20, False, 32)] * 5)
    scorer = video.VideoScorer(model, side=32)
    for call in (lambda: scorer.score(rgb, boxes=boxes, transforms=M), lambda: scorer.push(rgb, boxes=boxes, transforms=M),
                 lambda: scorer.explain(rgb, boxes=boxes, transforms=M),
                 lambda: scorer.score_videos([rgb], boxes=[boxes], transforms=[M]),
                 lambda: model.score_video(rgb, boxes=boxes, transforms=M, side=32),
                 lambda: model.explain_video(rgb, boxes=boxes, transforms=M, side=32),
                 lambda: model.score_videos([rgb], boxes=[boxes], transforms=[M], side=32)):
        with pytest.raises(ValueError, match='transforms'):
            call()
    nvs = video.VideoScorer(model, side=32, pixel_format='nv12')
    for call in (lambda: nvs.score(nv), lambda: nvs.push(nv), lambda: nvs.explain(nv), lambda: nvs.score_videos([nv])):
        with pytest.raises(ValueError, match='transforms'):
            call()
    with pytest.raises(TypeError):
        scorer.score(rgb, transforms=M.double())
    with pytest.raises(ValueError):
        scorer.score(rgb, transforms=M[:4])
    with pytest.raises(IndexError):
        scorer.score(rgb, transforms=torch.stack([_similarity(0.9, 10, 25, 41, False, 32)] * 5))
    with pytest.raises(IndexError):                                                        # the NV12 picture has 40 rows, not 60
        nvs.score(nv, transforms=torch.stack([_similarity(0.9, 10, 25, 50, False, 32)] * 5))
    with pytest.raises(ValueError):
        scorer.score_videos([rgb, rgb], transforms=[M])
    with pytest.raises(ValueError, match='side'):
        video.VideoScorer(model).score(rgb, transforms=M)
    for call in (lambda: scorer.score(rgb, transforms=M), lambda: nvs.score(nv, transforms=M),      # the arguments pass
                 lambda: model.score_video(nv, transforms=M, side=32, pixel_format='nv12')):
        with pytest.raises(RuntimeError, match='ROCm'):
            call()
