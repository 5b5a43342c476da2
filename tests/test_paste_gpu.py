"""Pasting maps onto frames (DESIGN.md "Pasting maps onto frames") on a real MI355X: istvt_relevance_paste_u8 / _nv12 against
the definition on the host (clips.paste_maps_host) on the same tables, in place and out of place, what a paste may and may
not touch, tables that were not validated, and VideoScorer.render_explanation against the plain op.

The comparison rule: every byte within 1 of the definition, and equal wherever 255 m and 256 alpha m are more than 1e-6 from
a half-integer (m: the definition's float64 field).  The pixels inside that band are counted from the host field and may be at
most 0.1 % of the region: a cap on what is exempt, not a tolerance."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def similarity(s, rad, cx, cy, mirror, S):
    """M = s R(rad), the mirror folded into the first column, the crop's centre (S / 2, S / 2) taken to (cx, cy)"""
    A = np.array([[s * math.cos(rad), -s * math.sin(rad)], [s * math.sin(rad), s * math.cos(rad)]])
    if mirror:
        A[:, 0] = -A[:, 0]
    t = np.array([cx, cy], dtype=np.float64) - A @ np.array([S / 2, S / 2])
    return torch.tensor(np.concatenate([A, t[:, None]], axis=1), dtype=torch.float32)


def frames_of(n, Hs, Ws, seed):
    return torch.randint(0, 256, (n, Hs, Ws, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def maps_of(n, g, seed):
    return torch.randn((n, g, g), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


ALPHAS = (0.0, 0.37, 0.5, 1.0)
HS, WS, S, G = 40, 56, 16, 4
# name -> (kind, table) for 4 frames of 40 x 56 at S = 16, g = 4.  Scale 7.9 cuts a 126-pixel square: every edge is clipped.
SMALL = {
    'boxes': ('boxes', [(3, 5, 20, 13),                # odd x0, odd width: ragged 16-byte edges
                        (0, 0, 40, 56),                # the whole frame
                        (17, 33, 1, 1),                # one pixel
                        (8, 2, 30, 50)]),
    'scales': ('transforms', [(0.126, 1.1, 30, 20, False), (1.7, 0.3, 28, 20, False), (7.9, -0.7, 28, 20, False),
                              (1.0, 0.0, 27.5, 19.25, True)]),
    'corner_and_edges': ('transforms', [(1.5, 0.4, 2, 3, False),                          # over the corner
                                        (1.4, -0.2, 1, 20, False), (1.4, 0.5, 55.5, 20, True),  # left, right
                                        (1.2, 0.3, 28, 0.5, False)]),                     # top
    'bottom_and_more': ('transforms', [(1.3, -0.3, 28, 39.5, False),                      # bottom
                                       (2.6, 2.0, 54, 38, True), (0.5, 0.3, 9.3, 31.7, False), (1.0, math.pi / 2, 20, 20, False)]),
}


def small_table(name):
    kind, rows = SMALL[name]
    if kind == 'boxes':
        return {'boxes': torch.tensor(rows, dtype=torch.int32)}
    return {'transforms': torch.stack([similarity(*r, S) for r in rows])}


def small_alphas(name):
    k = list(SMALL).index(name)
    return torch.tensor(ALPHAS[k:] + ALPHAS[:k], dtype=torch.float32)


def band_of(clips, maps, A, rect, alpha, side, Hs, Ws, even):
    """-> (band, region) bool (n, Hs, Ws): the pixels where 255 m or 256 alpha m lies within 1e-6 of a half-integer, and the
    pixels inside the region, from the definition's own field"""
    n = maps.shape[0]
    band = torch.zeros((n, Hs, Ws), dtype=torch.bool)
    region = torch.zeros((n, Hs, Ws), dtype=torch.bool)
    for i in range(n):
        y0, x0, h, w = rect[i].tolist()
        m, inside = clips.paste_field_host(maps[i], A[i], (y0, x0, h, w), side)

        def near(v):
            return ((v - torch.floor(v) - 0.5).abs() <= 1e-6) & inside

        band[i, y0:y0 + h, x0:x0 + w] = near(255.0 * m) | near(256.0 * float(alpha[i]) * m)
        region[i, y0:y0 + h, x0:x0 + w] = inside
    return band, region


def check_bytes(got, want, band, region, fmt, what):
    """the comparison rule of the module's docstring; got, want: host tensors of frames"""
    n, Hs, Ws = band.shape
    cap = 0.001 * int(region.sum())
    print('%s: %d of %d region pixels in the band; max |kernel - definition| = %d'
          % (what, int(band.sum()), int(region.sum()), int((got.int() - want.int()).abs().max())))
    assert int(band.sum()) <= cap
    assert int((got.int() - want.int()).abs().max()) <= 1
    if fmt == 'rgb24':
        assert torch.equal(got[~band], want[~band])
        return
    assert torch.equal(got[:, :Hs][~band], want[:, :Hs][~band])
    blocks = band.reshape(n, Hs // 2, 2, Ws // 2, 2).any(4).any(2).repeat_interleave(2, dim=2)    # a block with a pixel in the band
    assert torch.equal(got[:, Hs:][~blocks], want[:, Hs:][~blocks])


def outside_rect_untouched(got, before, rect, fmt, Hs):
    for i in range(got.shape[0]):
        y0, x0, h, w = rect[i].tolist()
        keep = torch.ones(got.shape[1:3] if fmt == 'rgb24' else got.shape[1:], dtype=torch.bool)
        keep[y0:y0 + h, x0:x0 + w] = False
        if fmt == 'nv12':
            keep[Hs + y0 // 2:Hs + (y0 + h) // 2, x0:x0 + w] = False
        assert torch.equal(got[i][keep], before[i][keep]), i


@pytest.fixture(scope='module')
def small(pkg):
    """the 40 x 56 frames in both formats, their maps, the colour table, and per table the geometry and the definition's
    result, computed once"""
    from istvt_amd import clips, explain
    rgb = frames_of(4, HS, WS, 4056)
    maps = maps_of(4, G, 44)
    lut = explain.jet_lut()
    nv = {mx: clips.rgb_to_nv12_host(rgb, mx) for mx in clips.YUV_MATRICES}
    ref = {}

    def case(name, fmt, matrix='bt709'):
        key = (name, fmt, matrix)
        if key not in ref:
            even = fmt == 'nv12'
            A, rect = clips.paste_geometry(4, HS, WS, S, even=even, **small_table(name))
            al = small_alphas(name)
            frames = nv[matrix] if even else rgb
            want = clips.paste_maps_host(frames, maps, A, rect, lut, al, S, pixel_format=fmt, yuv_matrix=matrix)
            ref[key] = dict(A=A, rect=rect, alpha=al, frames=frames, want=want,
                            table=clips.lut_to_ycc(lut, matrix) if even else lut)
        return ref[key]

    return dict(rgb=rgb, maps=maps, lut=lut, case=case)


# ---- the kernels against the definition --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(SMALL))
def test_rgb_against_the_definition(pkg, small, name):
    from istvt_amd import clips, ops
    c = small['case'](name, 'rgb24')
    dev, maps = c['frames'].cuda(), small['maps'].cuda()
    before = dev.clone()
    got = ops.relevance_paste_u8(dev, maps, c['A'], c['rect'], c['table'].cuda(), c['alpha'], S)
    assert got.dtype == torch.uint8 and got.shape == dev.shape and got.is_cuda and got.data_ptr() != dev.data_ptr()
    assert torch.equal(dev, before)                                                       # out of place: the input stays
    band, region = band_of(clips, small['maps'], c['A'], c['rect'], c['alpha'], S, HS, WS, False)
    check_bytes(got.cpu(), c['want'], band, region, 'rgb24', name)
    assert torch.equal(c['want'][0], c['frames'][0]) == (float(c['alpha'][0]) == 0.0)    # the definition pasted something
    # in place equals out of place; a second run gives the same bits; nothing outside rect is written
    assert ops.relevance_paste_u8(dev, maps, c['A'], c['rect'], c['table'].cuda(), c['alpha'], S, inplace=True) is dev
    assert torch.equal(dev, got)
    outside_rect_untouched(dev.cpu(), before.cpu(), c['rect'], 'rgb24', HS)
    assert torch.equal(ops.relevance_paste_u8(before, maps, c['A'], c['rect'], c['table'].cuda(), c['alpha'], S), got)
    # where the frames start in their allocation does not show, nor does a caller's out, nor the flat form of the maps
    store = torch.empty((before.numel() + 5,), dtype=torch.uint8, device='cuda')
    odd = store[5:].view(before.shape)
    odd.copy_(before)
    out = torch.full_like(before, 9)
    assert ops.relevance_paste_u8(odd, maps.reshape(4, G * G), c['A'], c['rect'], c['table'].cuda(), c['alpha'], S, out=out) is out
    assert torch.equal(out, got)
    ops.relevance_paste_u8(odd, maps, c['A'], c['rect'], c['table'].cuda(), c['alpha'], S, inplace=True)
    assert torch.equal(odd, got)


@pytest.mark.parametrize('matrix', ['bt601', 'bt709', 'jfif'])
@pytest.mark.parametrize('name', list(SMALL))
def test_nv12_against_the_definition(pkg, small, name, matrix):
    """a contiguous batch (pitch 56: byte by byte) and surfaces with a padded pitch of 66 (byte by byte) and 64 (16-byte
    accesses, ragged at the rectangle's edges), in place where they lie"""
    from istvt_amd import clips, ops
    c = small['case'](name, 'nv12', matrix)
    maps, table = small['maps'].cuda(), c['table'].cuda()
    band, region = band_of(clips, small['maps'], c['A'], c['rect'], c['alpha'], S, HS, WS, True)
    dev = c['frames'].cuda()
    got = ops.relevance_paste_nv12(dev, maps, c['A'], c['rect'], table, c['alpha'], S)
    assert got.shape == dev.shape and got.is_contiguous() and torch.equal(dev, c['frames'].cuda())
    check_bytes(got.cpu(), c['want'], band, region, 'nv12', '%s %s' % (name, matrix))
    outside_rect_untouched(got.cpu(), c['frames'], c['rect'], 'nv12', HS)
    assert torch.equal(ops.relevance_paste_nv12(dev, maps, c['A'], c['rect'], table, c['alpha'], S), got)    # the same bits again
    rows = HS + HS // 2
    for pitch, lead in ((66, 5), (64, 0), (64, 6)):
        store = torch.full((lead + 4 * rows * pitch + 64,), 77, dtype=torch.uint8, device='cuda')
        surf = store.as_strided((4, rows, WS), (rows * pitch, pitch, 1), lead)
        surf.copy_(c['frames'])
        assert torch.equal(ops.relevance_paste_nv12(surf, maps, c['A'], c['rect'], table, c['alpha'], S), got), (pitch, lead)
        assert ops.relevance_paste_nv12(surf, maps, c['A'], c['rect'], table, c['alpha'], S, inplace=True) is surf
        assert torch.equal(surf, got), (pitch, lead)
        pad = store.clone()
        pad.as_strided((4, rows, WS), (rows * pitch, pitch, 1), lead).fill_(77)
        assert int((pad != 77).sum()) == 0                                                # the padding between the rows is untouched


@pytest.mark.parametrize('Hs,Ws,side,g,tab', [(120, 160, 96, 6, (0.9, 0.25, 83.3, 57.1, False)),
                                              (96, 128, 224, 14, (0.3, -0.4, 60.2, 50.9, True))])
def test_at_the_models_geometries(pkg, Hs, Ws, side, g, tab):
    from istvt_amd import clips, explain, ops
    rgb = frames_of(1, Hs, Ws, Hs * Ws)
    maps = maps_of(1, g, g)
    M = similarity(*tab, side)[None]
    lut = explain.jet_lut()
    al = torch.tensor([0.37], dtype=torch.float32)
    for fmt, frames in (('rgb24', rgb), ('nv12', clips.rgb_to_nv12_host(rgb, 'bt709'))):
        even = fmt == 'nv12'
        A, rect = clips.paste_geometry(1, Hs, Ws, side, transforms=M, even=even)
        want = clips.paste_maps_host(frames, maps, A, rect, lut, al, side, pixel_format=fmt)
        band, region = band_of(clips, maps, A, rect, al, side, Hs, Ws, even)
        if even:
            got = ops.relevance_paste_nv12(frames.cuda(), maps.cuda(), A, rect, clips.lut_to_ycc(lut).cuda(), al, side)
        else:
            got = ops.relevance_paste_u8(frames.cuda(), maps.cuda(), A, rect, lut.cuda(), al, side)
        check_bytes(got.cpu(), want, band, region, fmt, '%d x %d, S = %d, g = %d, %s' % (Hs, Ws, side, g, fmt))
        assert torch.equal(explain.overlay_frames(frames.cuda(), maps.cuda(), transforms=M, side=side, alpha=0.37, lut=lut,
                                                  pixel_format=fmt), got)


# ---- tables that were not validated --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['rgb24', 'nv12'])
def test_unvalidated_tables(pkg, small, fmt):
    """checked=True: a frame with a non-finite A, alpha or map entry keeps its bytes and the others are pasted; a rectangle
    larger than needed, or one that sticks out of the frame, gives the same bytes"""
    from istvt_amd import ops
    c = small['case']('scales', fmt)
    paste = ops.relevance_paste_nv12 if fmt == 'nv12' else ops.relevance_paste_u8
    dev, maps, table = c['frames'].cuda(), small['maps'].cuda(), c['table'].cuda()
    al = torch.tensor([0.9, 0.37, 0.5, 1.0], dtype=torch.float32)
    A, rect = c['A'].cuda(), c['rect'].cuda()
    ref = paste(dev, maps, A, rect, table, al.cuda(), S, checked=True)
    assert torch.equal(ref, paste(dev, maps, c['A'], c['rect'], table, al, S))
    for f in range(4):
        assert not torch.equal(ref[f], dev[f])
    for what, value in (('A', float('nan')), ('A', float('inf')), ('alpha', float('nan')), ('alpha', float('-inf')),
                        ('map', float('nan')), ('map', float('inf'))):
        a2, al2, m2 = A.clone(), al.clone(), maps.clone()
        if what == 'A':
            a2[1, 1, 2] = value
        elif what == 'alpha':
            al2[1] = value
        else:
            m2[1, 3, 2] = value
        got = paste(dev, m2, a2, rect, table, al2.cuda(), S, checked=True)
        assert torch.equal(got[1], dev[1]), (what, value)
        for f in (0, 2, 3):
            assert torch.equal(got[f], ref[f]), (what, value, f)
    big = torch.tensor([[-7, -9, 1000, 1000], [0, 0, HS, WS], [-(2 ** 31), -(2 ** 31), 2 ** 31 - 1, 2 ** 31 - 1], [1, 1, 39, 55]],
                       dtype=torch.int32)
    big[3] = c['rect'][3] + torch.tensor([-1, -1, 2, 2], dtype=torch.int32) if fmt == 'rgb24' else c['rect'][3]
    got = paste(dev, maps, A, big.cuda(), table, al.cuda(), S, checked=True)
    for f in (0, 1, 3):
        assert torch.equal(got[f], ref[f]), f
    assert torch.equal(got[2], dev[2])                                                    # an empty rectangle after the clamp
    with pytest.raises(RuntimeError):
        paste(dev, maps, c['A'], c['rect'], table, al, S, checked=True)                   # checked tables live on the device
    with pytest.raises(ValueError):
        paste(dev, maps, c['A'] * float('nan'), c['rect'], table, al, S)
    with pytest.raises(RuntimeError):
        paste(dev, maps[:3], c['A'], c['rect'], table, al, S)
    with pytest.raises(RuntimeError):
        paste(dev, maps, c['A'], c['rect'], table, al, S, out=torch.empty_like(dev), inplace=True)


def test_two_faces_in_place(pkg, small):
    from istvt_amd import clips, explain
    b1 = torch.tensor([[4, 6, 14, 17]] * 4, dtype=torch.int32)
    b2 = torch.tensor([[22, 30, 16, 22]] * 4, dtype=torch.int32)
    lut2 = small['lut'].flip(1).contiguous()
    m2 = maps_of(4, G, 45)
    A1, r1 = clips.paste_geometry(4, HS, WS, S, boxes=b1)
    A2, r2 = clips.paste_geometry(4, HS, WS, S, boxes=b2)
    want = clips.paste_maps_host(clips.paste_maps_host(small['rgb'], small['maps'], A1, r1, small['lut'], 0.6, S), m2, A2, r2, lut2,
                                 0.9, S)
    dev = small['rgb'].cuda()
    explain.overlay_frames(dev, small['maps'].cuda(), boxes=b1, side=S, alpha=0.6, inplace=True)
    explain.overlay_frames(dev, m2.cuda(), boxes=b2, side=S, alpha=0.9, lut=lut2, inplace=True)
    assert int((dev.cpu().int() - want.int()).abs().max()) <= 1
    other = small['rgb'].cuda()
    explain.overlay_frames(other, m2.cuda(), boxes=b2, side=S, alpha=0.9, lut=lut2, inplace=True)
    explain.overlay_frames(other, small['maps'].cuda(), boxes=b1, side=S, alpha=0.6, inplace=True)
    assert torch.equal(other, dev)


# ---- the scorer ------------------------------------------------------------------------------------------------------------
SIDE = 96


@pytest.fixture(scope='module')
def video_case(pkg):
    """the test model's geometry: XceptionVidTr(num_frames=4, grid=6, depth=1) at side 96 with the oracle's seeded random
    parameters, its running statistics moved by one training forward (default initialisation with statistics (0, 1) gives
    maps of zeros: nothing would be pasted); 12 frames of 120 x 160 with one box and one similarity each"""
    from istvt_amd import clips
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    from oracle import istvt_ref as R
    shapes = {'xcep.model.' + k: v for k, v in R.stem_param_shapes().items()}
    shapes.update({'vit.' + k: v for k, v in R.dsttr_param_shapes(4, 6, depth=1).items()})
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    sd = model.state_dict()
    sd.update(R.random_params(shapes, seed=0))
    model.load_state_dict(sd)
    model = model.cuda().train()
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        model(torch.randn((2, 4, 3, SIDE, SIDE), generator=g).cuda())
    u8 = frames_of(12, 120, 160, 120160)
    r = torch.rand((12, 5), generator=g).tolist()
    M = torch.stack([similarity(0.7 + 0.6 * a, 0.8 * b - 0.4, 160 * (0.4 + 0.2 * c), 120 * (0.4 + 0.2 * d), e < 0.3, SIDE)
                     for a, b, c, d, e in r])
    boxes = torch.tensor([[int(10 + 20 * a), int(15 + 40 * b), int(60 + 30 * c), int(70 + 30 * d)] for a, b, c, d, _ in r],
                         dtype=torch.int32)
    return dict(model=model, u8=u8, nv=clips.rgb_to_nv12_host(u8, 'bt709'), M=M, boxes=boxes)


@pytest.mark.parametrize('fmt', ['rgb24', 'nv12'])
@pytest.mark.parametrize('kind', ['boxes', 'transforms'])
def test_render_explanation_is_the_op_on_the_explanation(video_case, kind, fmt):
    from istvt_amd import clips, explain, ops, video
    model = video_case['model']
    frames = video_case['u8' if fmt == 'rgb24' else 'nv']
    table = {kind: video_case['boxes' if kind == 'boxes' else 'M']}
    flags = [m.training for m in model.modules()]                                        # the model is in train mode
    params = [p.detach().clone() for p in model.parameters()]
    scorer = video.VideoScorer(model, frame_batch=64, window_batch=3, side=SIDE, pixel_format=fmt)
    ex = scorer.explain(frames, **table)
    got = scorer.render_explanation(frames, ex, **table)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == frames.shape
    even = fmt == 'nv12'
    A, rect = clips.paste_geometry(12, 120, 160, SIDE, even=even, **table)
    lut = explain.jet_lut()
    al = 0.5 * (ex.frame_weight / ex.frame_weight.max()).clamp(0, 1)
    # (at depth 1 the verdict reads the spatial attention of the temporal token's frame alone, so frame_s of the real frames
    # is all zeros and nothing is pasted here: the same call on maps and weights that are not zero follows below)
    if even:
        want = ops.relevance_paste_nv12(frames.cuda(), ex.frame_s, A, rect, clips.lut_to_ycc(lut, 'bt709').cuda(), al, SIDE)
    else:
        want = ops.relevance_paste_u8(frames.cuda(), ex.frame_s, A, rect, lut.cuda(), al, SIDE)
    assert torch.equal(got, want)
    five = video.VideoScorer(model, frame_batch=5, window_batch=3, side=SIDE, pixel_format=fmt)
    gen = torch.Generator().manual_seed(5)
    busy = ex._replace(frame_s=torch.randn((12, 36), generator=gen).cuda(), frame_weight=torch.rand((12,), generator=gen).cuda())
    for e, ref in ((ex, got), (busy, None)):
        if ref is None:                                                                   # maps that paste something
            al = 0.5 * (e.frame_weight / e.frame_weight.max()).clamp(0, 1)
            assert float(al.max()) == 0.5 and float(al.min()) >= 0
            if even:
                ref = ops.relevance_paste_nv12(frames.cuda(), e.frame_s, A, rect, clips.lut_to_ycc(lut, 'bt709').cuda(), al, SIDE)
            else:
                ref = ops.relevance_paste_u8(frames.cuda(), e.frame_s, A, rect, lut.cuda(), al, SIDE)
            assert not torch.equal(ref, frames.cuda())
            assert torch.equal(scorer.render_explanation(frames, e, **table), ref)
        assert torch.equal(scorer.render_explanation(frames.cuda(), e, **table), ref)    # device frames: the bits of host frames
        assert torch.equal(five.render_explanation(frames, e, **table), ref)
        assert torch.equal(model.render_explanation(frames, e, side=SIDE, pixel_format=fmt, **table), ref)
    # the temporal maps with one weight for every frame, and a caller's table
    flat = scorer.render_explanation(frames, ex, which='t', alpha=0.8, weight_frames=False, lut=lut.flip(1).contiguous(), **table)
    tab = lut.flip(1).contiguous()
    if even:
        want = ops.relevance_paste_nv12(frames.cuda(), ex.frame_t, A, rect, clips.lut_to_ycc(tab, 'bt709').cuda(), 0.8, SIDE)
    else:
        want = ops.relevance_paste_u8(frames.cuda(), ex.frame_t, A, rect, tab.cuda(), 0.8, SIDE)
    assert torch.equal(flat, want)
    assert [m.training for m in model.modules()] == flags
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))
