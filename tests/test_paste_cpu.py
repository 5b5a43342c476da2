"""Pasting maps onto frames (DESIGN.md "Pasting maps onto frames") without a device: the symbols, the argument errors, the
geometry (clips.paste_geometry), the field against torch's bilinear upsampling, and the properties of the definition
(clips.paste_maps_host) in packed RGB and NV12."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


HS, WS, S, G = 40, 56, 16, 4


def _frames(n, Hs, Ws, seed):
    return torch.randint(0, 256, (n, Hs, Ws, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _maps(n, g, seed):
    return torch.randn((n, g, g), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _similarity(s, rad, cx, cy, mirror, n_out):
    A = np.array([[s * math.cos(rad), -s * math.sin(rad)], [s * math.sin(rad), s * math.cos(rad)]])
    if mirror:
        A[:, 0] = -A[:, 0]
    t = np.array([cx, cy]) - A @ np.array([n_out / 2, n_out / 2])
    return torch.tensor(np.concatenate([A, t[:, None]], axis=1), dtype=torch.float32)


def _region(clips, A, Hs, Ws, side):
    """bool (Hs, Ws): the pixels whose centre lands in the crop, from the definition's own field over the whole frame"""
    _, inside = clips.paste_field_host(torch.arange(4, dtype=torch.float32).reshape(2, 2), A, (0, 0, Hs, Ws), side)
    return inside


def test_argument_errors_need_no_device(pkg):
    from istvt_amd import clips, explain, ops, video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    boxes = torch.tensor([[3, 5, 20, 20]] * 4, dtype=torch.int32)
    M = torch.stack([_similarity(1.2, 0.2, 28, 20, False, S)] * 4)
    with pytest.raises(ValueError):
        clips.paste_geometry(4, HS, WS, S, boxes=boxes, transforms=M)
    with pytest.raises(ValueError):
        clips.paste_geometry(4, HS, WS, S)
    with pytest.raises(ValueError):
        clips.paste_geometry(4, 41, WS, S, boxes=boxes, even=True)
    rgb, nv = _frames(4, HS, WS, 1), torch.zeros((4, HS * 3 // 2, WS), dtype=torch.uint8)
    maps = _maps(4, G, 2)
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    scorer = video.VideoScorer(model, side=S)
    nvs = video.VideoScorer(model, side=S, pixel_format='nv12')
    ex = video.VideoExplanation(None, None, maps.reshape(4, -1), maps.reshape(4, -1), torch.ones(4), torch.zeros(4),
                                torch.ones(4, dtype=torch.int32))

    def calls(**kw):
        return (lambda: explain.overlay_frames(rgb, maps, side=S, **kw),
                lambda: explain.overlay_frames(nv, maps, side=S, pixel_format='nv12', **kw),
                lambda: scorer.render_explanation(rgb, ex, **kw), lambda: nvs.render_explanation(nv, ex, **kw),
                lambda: model.render_explanation(rgb, ex, side=S, **kw))

    for call in calls(boxes=boxes, transforms=M):
        with pytest.raises(ValueError, match='transforms'):
            call()
    for call in (lambda: explain.overlay_frames(rgb, maps, side=S), lambda: nvs.render_explanation(nv, ex)):
        with pytest.raises(ValueError, match='transforms'):
            call()
    # the two validators' own errors pass through, before anything is launched (the model and the frames are on the host)
    for call in calls(boxes=boxes.long()) + calls(transforms=M.double()):
        with pytest.raises(TypeError):
            call()
    for call in calls(boxes=boxes[:3]) + calls(transforms=M[:3]) + calls(transforms=M * 100.0):
        with pytest.raises(ValueError):
            call()
    far = torch.stack([_similarity(1.2, 0.2, 28, 45, False, S)] * 4)
    for call in calls(boxes=torch.tensor([[30, 5, 20, 20]] * 4, dtype=torch.int32)) + calls(transforms=far):
        with pytest.raises(IndexError):
            call()
    with pytest.raises(ValueError, match='side'):
        explain.overlay_frames(rgb, maps, boxes=boxes)
    with pytest.raises(ValueError, match='which'):
        scorer.render_explanation(rgb, ex, boxes=boxes, which='x')
    with pytest.raises(ValueError, match='frames'):
        scorer.render_explanation(rgb[:3], ex, boxes=boxes[:3])
    # valid arguments: the host tensors are refused where the device is needed, in ops and in the scorer
    A, rect = clips.paste_geometry(4, HS, WS, S, boxes=boxes)
    lut = explain.jet_lut()
    with pytest.raises(RuntimeError, match='ROCm'):
        ops.relevance_paste_u8(rgb, maps, A, rect, lut, 0.5, S)
    with pytest.raises(RuntimeError, match='ROCm'):
        ops.relevance_paste_nv12(nv, maps, A, rect, clips.lut_to_ycc(lut), 0.5, S)
    for call in calls(boxes=boxes) + calls(transforms=M):
        with pytest.raises(RuntimeError, match='ROCm'):
            call()


def test_geometry_of_boxes_and_similarities(pkg):
    from istvt_amd import clips
    sq = torch.tensor([[3, 5, 20, 20], [0, 0, 40, 40], [17, 33, 1, 1], [8, 2, 31, 31]], dtype=torch.int32)
    A_box, _ = clips.paste_geometry(4, HS, WS, S, boxes=sq)
    A_sim, _ = clips.paste_geometry(4, HS, WS, S, transforms=clips.similarity_of_boxes(sq, S))
    assert A_box.dtype == torch.float64 and tuple(A_box.shape) == (4, 2, 3)
    err = float((A_box - A_sim).abs().max())
    print('square boxes against their similarities: max |A - A| = %.3g' % err)
    assert err <= 1e-9
    boxes = torch.tensor([[3, 5, 20, 13], [0, 0, 40, 56], [17, 33, 1, 1], [9, 2, 7, 50]], dtype=torch.int32)
    for even in (False, True):
        A, rect = clips.paste_geometry(4, HS, WS, S, boxes=boxes, even=even)
        assert rect.dtype == torch.int32 and tuple(rect.shape) == (4, 4)
        for i, (y0, x0, h, w) in enumerate(boxes.tolist()):
            assert A[i].tolist() == [[S / w, 0.0, -x0 * S / w], [0.0, S / h, -y0 * S / h]]
            want = torch.zeros((HS, WS), dtype=torch.bool)
            want[y0:y0 + h, x0:x0 + w] = True
            assert torch.equal(_region(clips, A[i], HS, WS, S), want), boxes[i].tolist()   # exactly the box's pixels
    tables = [_similarity(0.126, 1.1, 30, 20, False, S), _similarity(1.7, 0.3, 28, 20, False, S),
              _similarity(7.9, -0.7, 28, 20, False, S), _similarity(1.0, 0.0, 28, 20, True, S),
              _similarity(1.5, 0.4, 2, 3, False, S), _similarity(1.5, 0.4, 55, 39, False, S),
              _similarity(2.0, 2.5, 1, 20, True, S), _similarity(0.9, -1.3, 28, 39.5, False, S)]
    M = torch.stack(tables)
    n = len(tables)
    for even in (False, True):
        A, rect = clips.paste_geometry(n, HS, WS, S, transforms=M, even=even)
        for i in range(n):
            y0, x0, h, w = rect[i].tolist()
            assert 0 <= y0 and 0 <= x0 and h >= 0 and w >= 0 and y0 + h <= HS and x0 + w <= WS
            if even:
                assert y0 % 2 == 0 and x0 % 2 == 0 and h % 2 == 0 and w % 2 == 0
            reg = _region(clips, A[i], HS, WS, S)
            assert bool(reg.any())
            outside = reg.clone()
            outside[y0:y0 + h, x0:x0 + w] = False
            assert not bool(outside.any()), (i, rect[i].tolist())                        # rect contains the region
        # A inverts M: the crop's centre comes back
        c = M.double() @ torch.tensor([S / 2, S / 2, 1.0], dtype=torch.float64)
        back = torch.einsum('nij,nj->ni', A, torch.cat([c, torch.ones(n, 1, dtype=torch.float64)], 1))
        assert float((back - S / 2).abs().max()) <= 1e-9


@pytest.mark.parametrize('g,side', [(6, 96), (14, 224)])
def test_field_is_bilinear_upsampling_of_the_normalised_grid(pkg, g, side):
    from istvt_amd import clips
    grid = _maps(1, g, 100 + g)[0]
    A, rect = clips.paste_geometry(1, side, side, side, boxes=torch.tensor([[0, 0, side, side]], dtype=torch.int32))
    assert rect[0].tolist() == [0, 0, side, side]
    m, inside = clips.paste_field_host(grid, A[0], rect[0].tolist(), side)
    assert bool(inside.all())
    d = grid.double()
    mhat = (d - d.min()) / (d.max() - d.min())
    want = F.interpolate(mhat[None, None], scale_factor=side / g, mode='bilinear', align_corners=False)[0, 0]
    err = float((m - want).abs().max())
    print('g = %d, S = %d: max |field - F.interpolate| = %.3g' % (g, side, err))
    assert err <= 1e-12
    assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0


def _both_formats(clips, rgb, matrix='bt709'):
    return (('rgb24', rgb), ('nv12', clips.rgb_to_nv12_host(rgb, matrix)))


def test_identities_of_the_definition(pkg):
    """alpha = 0, a constant map and a map with a NaN give the input bytes; bytes outside the region are equal"""
    from istvt_amd import clips, explain
    lut = explain.jet_lut()
    M = torch.stack([_similarity(1.3, 0.3, 28, 20, False, S), _similarity(1.0, -0.6, 4, 5, True, S),
                     _similarity(2.2, 1.0, 50, 30, False, S), _similarity(0.7, 0.1, 20, 20, False, S)])
    maps = _maps(4, G, 5)
    for fmt, frames in _both_formats(clips, _frames(4, HS, WS, 4)):
        even = fmt == 'nv12'
        A, rect = clips.paste_geometry(4, HS, WS, S, transforms=M, even=even)
        kw = dict(pixel_format=fmt)
        assert torch.equal(clips.paste_maps_host(frames, maps, A, rect, lut, 0.0, S, **kw), frames)
        assert torch.equal(clips.paste_maps_host(frames, torch.full_like(maps, 3.5), A, rect, lut, 1.0, S, **kw), frames)
        bad = maps.clone()
        bad[1, 2, 1] = float('nan')
        bad[3, 0, 0] = float('inf')
        out = clips.paste_maps_host(frames, bad, A, rect, lut, 0.8, S, **kw)
        ref = clips.paste_maps_host(frames, maps, A, rect, lut, 0.8, S, **kw)
        assert out.dtype == torch.uint8 and out.shape == frames.shape and out.data_ptr() != frames.data_ptr()
        assert torch.equal(out[1], frames[1]) and torch.equal(out[3], frames[3])
        assert torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2])
        badA = A.clone()
        badA[2, 0, 1] = float('nan')
        out = clips.paste_maps_host(frames, maps, badA, rect, lut, torch.tensor([0.8, float('nan'), 0.8, 0.8]), S, **kw)
        assert torch.equal(out[1], frames[1]) and torch.equal(out[2], frames[2]) and torch.equal(out[0], ref[0])
        for i in range(4):
            reg = _region(clips, A[i], HS, WS, S)
            assert not torch.equal(ref[i], frames[i])
            if fmt == 'rgb24':
                assert torch.equal(ref[i][~reg], frames[i][~reg])
                continue
            assert torch.equal(ref[i, :HS][~reg], frames[i, :HS][~reg])
            blocks = reg.reshape(HS // 2, 2, WS // 2, 2).any(3).any(1)                   # a block any of whose pixels is inside
            keep = ~blocks.repeat_interleave(2, dim=1)
            assert torch.equal(ref[i, HS:][keep], frames[i, HS:][keep])
        big = torch.tensor([[-5, -7, 900, 900]] * 4, dtype=torch.int32)                   # a rectangle that is too large
        assert torch.equal(clips.paste_maps_host(frames, maps, A, big, lut, 0.8, S, **kw), ref)


def test_quarter_turn_pastes_the_turned_map(pkg):
    """maps whose normalised cells are multiples of 1 / 8 at scale 1: every product of the bilinear is exact, in any order"""
    from istvt_amd import clips, explain
    lut = explain.jet_lut()
    cells = torch.randint(0, 9, (2, G, G), generator=torch.Generator().manual_seed(9)).float()
    cells[:, 0, 0], cells[:, 3, 2] = 0.0, 8.0
    for fmt, frames in _both_formats(clips, _frames(2, HS, WS, 8)):
        even = fmt == 'nv12'
        for y0, x0 in ((6, 10), (24, 40)):
            turn = torch.tensor([[[0, -1, x0 + S], [1, 0, y0]]] * 2, dtype=torch.float32)
            box = torch.tensor([[y0, x0, S, S]] * 2, dtype=torch.int32)
            At, rt = clips.paste_geometry(2, HS, WS, S, transforms=turn, even=even)
            Ab, rb = clips.paste_geometry(2, HS, WS, S, boxes=box, even=even)
            got = clips.paste_maps_host(frames, cells, At, rt, lut, 0.75, S, pixel_format=fmt)
            # the crop is rot90(slice, 1), so the slice shows rot90(crop field, -1)
            want = clips.paste_maps_host(frames, torch.rot90(cells, -1, (1, 2)).contiguous(), Ab, rb, lut, 0.75, S,
                                         pixel_format=fmt)
            assert torch.equal(got, want) and not torch.equal(got, frames)


def test_two_faces_compose_in_either_order(pkg):
    from istvt_amd import clips, explain
    lut_a = explain.jet_lut()
    lut_b = lut_a.flip(1).contiguous()
    b1 = torch.tensor([[4, 6, 14, 17]] * 2, dtype=torch.int32)
    b2 = torch.tensor([[22, 30, 16, 22]] * 2, dtype=torch.int32)
    m1, m2 = _maps(2, G, 11), _maps(2, G, 12)
    for fmt, frames in _both_formats(clips, _frames(2, HS, WS, 10)):
        even = fmt == 'nv12'
        A1, r1 = clips.paste_geometry(2, HS, WS, S, boxes=b1, even=even)
        A2, r2 = clips.paste_geometry(2, HS, WS, S, boxes=b2, even=even)
        one = clips.paste_maps_host(frames, m1, A1, r1, lut_a, 0.6, S, pixel_format=fmt)
        two = clips.paste_maps_host(frames, m2, A2, r2, lut_b, 0.9, S, pixel_format=fmt)
        ab = clips.paste_maps_host(one, m2, A2, r2, lut_b, 0.9, S, pixel_format=fmt)
        ba = clips.paste_maps_host(two, m1, A1, r1, lut_a, 0.6, S, pixel_format=fmt)
        assert torch.equal(ab, ba) and not torch.equal(ab, one) and not torch.equal(ab, two)


@pytest.mark.parametrize('matrix', ['bt601', 'bt709', 'jfif'])
def test_lut_to_ycc_is_the_encoder_on_flat_blocks(pkg, matrix):
    from istvt_amd import clips
    colours = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)]
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    for i, c in enumerate(colours):
        lut[i] = torch.tensor(c, dtype=torch.uint8)
    ycc = clips.lut_to_ycc(lut, matrix)
    assert ycc.dtype == torch.uint8 and tuple(ycc.shape) == (256, 3)
    for i, c in enumerate(colours):
        flat = torch.tensor(c, dtype=torch.uint8).expand(2, 2, 3).contiguous()
        nv = clips.rgb_to_nv12_host(flat, matrix)                                         # (3, 2): two Y rows, one (Cb, Cr) pair
        assert nv[:2].flatten().tolist() == [int(ycc[i, 0])] * 4 and nv[2].tolist() == ycc[i, 1:].tolist(), (matrix, c)
    with pytest.raises(ValueError):
        clips.lut_to_ycc(lut, 'bt2020')
    with pytest.raises(ValueError):
        clips.lut_to_ycc(lut[:, :2], matrix)
