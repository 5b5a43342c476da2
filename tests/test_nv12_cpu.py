"""NV12 frames (DESIGN.md "NV12 frames") without a device: the coefficients against their derivation, the integer
expression against the float64 matrix, the layout, the argument errors and the float encoder's round trip."""
from fractions import Fraction

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


KR_KB = {'bt601': (Fraction(299, 1000), Fraction(114, 1000)), 'bt709': (Fraction(2126, 10000), Fraction(722, 10000))}


def _exact(matrix):
    """the five exact rationals of a limited-range matrix: ky, krv, kgu, kgv, kbu"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    c = Fraction(255, 224)
    return (Fraction(255, 219), c * 2 * (1 - kr), c * 2 * kb * (1 - kb) / kg, c * 2 * kr * (1 - kr) / kg, c * 2 * (1 - kb))


def _triples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (3, n), generator=g, dtype=torch.uint8)


def _as_nv12(Y, Cb, Cr):
    """n triples as one NV12 frame of 2 x 2n pixels whose every pixel column pair holds one triple: (3, 2n) bytes"""
    n = Y.numel()
    f = torch.empty((1, 3, 2 * n), dtype=torch.uint8)
    f[0, 0] = Y.repeat_interleave(2)
    f[0, 1] = Y.repeat_interleave(2)
    f[0, 2, 0::2] = Cb
    f[0, 2, 1::2] = Cr
    return f


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_coefficients_follow_from_kr_kb(pkg, matrix):
    from istvt_amd import clips
    ky, krv, kgu, kgv, kbu = (int((v * 65536 + Fraction(1, 2)).__floor__()) for v in _exact(matrix))
    assert clips.nv12_coefficients(matrix) == (ky, 16, krv, kgu, kgv, kbu)
    assert all(abs(Fraction(k, 65536) - v) <= Fraction(1, 2 * 65536) for k, v in zip((ky, krv, kgu, kgv, kbu), _exact(matrix)))
    with pytest.raises(ValueError):
        clips.nv12_coefficients('bt2020')


def test_jfif_is_the_jpeg_decoders_colour_out(pkg):
    from istvt_amd import clips
    assert clips.nv12_coefficients('jfif') == (65536, 0, 91881, 22554, 46802, 116130)
    Y, Cb, Cr = _triples(200000, 1)
    got = clips.nv12_to_rgb_host(_as_nv12(Y, Cb, Cr), 'jfif')[0, 0, 0::2]
    y, cb, cr = Y.to(torch.int32), Cb.to(torch.int32) - 128, Cr.to(torch.int32) - 128
    want = torch.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                        y + ((116130 * cb + 32768) >> 16)], dim=1).clamp(0, 255).to(torch.uint8)
    assert torch.equal(got, want)


@pytest.mark.parametrize('matrix', ['bt601', 'bt709'])
def test_integer_expression_against_float64(pkg, matrix):
    """Every byte within 1 of clamp(floor(v + 0.5)) of the float64 matrix product, equal where v is more than 0.004 from a
    half: three coefficients each off by at most 0.5 / 65536 times magnitudes of at most 239 + 128 + 128 give 0.0038.  At
    most 2 % of the values may lie in that band."""
    from istvt_amd import clips
    Y, Cb, Cr = _triples(2000000, 7 if matrix == 'bt601' else 8)
    got = clips.nv12_to_rgb_host(_as_nv12(Y, Cb, Cr), matrix)[0, 0, 0::2].numpy().astype(np.int64)
    ky, krv, kgu, kgv, kbu = (float(v) for v in _exact(matrix))
    y, cb, cr = Y.numpy().astype(np.float64) - 16, Cb.numpy().astype(np.float64) - 128, Cr.numpy().astype(np.float64) - 128
    v = np.stack([ky * y + krv * cr, ky * y - kgu * cb - kgv * cr, ky * y + kbu * cb], axis=1)
    want = np.clip(np.floor(v + 0.5), 0, 255).astype(np.int64)
    band = np.abs(v - np.floor(v) - 0.5) <= 0.004
    share = float(band.mean())
    diff = np.abs(got - want)
    print('%s: %d of %d bytes differ, max %d, band share %.3f %%' % (matrix, int((diff != 0).sum()), diff.size, int(diff.max()),
                                                                    100 * share))
    assert diff.max() <= 1
    assert np.array_equal(got[~band], want[~band])
    assert share <= 0.02


def test_layout_nearest_chroma_pitch_and_clips(pkg):
    from istvt_amd import clips
    g = torch.Generator().manual_seed(3)
    Hs, Ws = 6, 10
    nv = torch.randint(0, 256, (4, 9, Ws), generator=g, dtype=torch.uint8)
    rgb = clips.nv12_to_rgb_host(nv, 'bt709')
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (4, Hs, Ws, 3)
    coef = clips.nv12_coefficients('bt709')
    for f, y, x in ((0, 0, 0), (1, 3, 5), (2, 5, 9), (3, 1, 8), (0, 4, 3)):          # odd origins pick (y >> 1, x >> 1)
        Y = nv[f, y, x].to(torch.int32).reshape(1)
        cb = nv[f, Hs + (y >> 1), 2 * (x >> 1)].to(torch.int32).reshape(1) - 128
        cr = nv[f, Hs + (y >> 1), 2 * (x >> 1) + 1].to(torch.int32).reshape(1) - 128
        assert torch.equal(clips._ycc_to_rgb(Y, cb, cr, coef)[0], rgb[f, y, x])
    # a pitched surface wrapped with as_strided equals its contiguous copy
    pitch, fstride = 16, 9 * 16 + 5
    store = torch.randint(0, 256, (4 * fstride + 64,), generator=g, dtype=torch.uint8)
    surf = store.as_strided((4, 9, Ws), (fstride, pitch, 1), 3)
    assert not surf.is_contiguous() and clips.check_nv12(surf) == (Hs, Ws)
    assert torch.equal(clips.nv12_to_rgb_host(surf, 'bt601'), clips.nv12_to_rgb_host(surf.contiguous(), 'bt601'))
    # clips are the flattened call, through the crop too
    boxes = torch.tensor([[1, 3, 5, 7], [0, 0, 6, 10]], dtype=torch.int32)
    four = nv.reshape(2, 2, 9, Ws)
    assert torch.equal(clips.nv12_to_rgb_host(four, 'jfif').reshape(4, Hs, Ws, 3), clips.nv12_to_rgb_host(nv, 'jfif'))
    a = clips.crop_resize_nv12_host(four, boxes, 4, 'bt709')
    b = clips.crop_resize_nv12_host(nv, clips.per_frame_boxes(boxes, 2), 4, 'bt709')
    assert tuple(a.shape) == (2, 2, 4, 4, 3) and torch.equal(a.reshape(4, 4, 4, 3), b)
    assert torch.equal(b, clips.crop_resize_host(rgb, clips.per_frame_boxes(boxes, 2), 4))


def test_check_nv12_and_argument_errors(pkg):
    from istvt_amd import clips, ops
    ok = torch.zeros((2, 9, 10), dtype=torch.uint8)
    assert clips.check_nv12(ok) == (6, 10) and clips.check_nv12(ok.reshape(1, 2, 9, 10)) == (6, 10)
    for bad in (ok.float(), ok.to(torch.int8), ok.tolist()):
        with pytest.raises(TypeError):
            clips.check_nv12(bad)
    for bad in (torch.zeros((2, 8, 10), dtype=torch.uint8),                      # rows not divisible by 3
                torch.zeros((2, 9, 9), dtype=torch.uint8),                       # odd width
                torch.zeros((2, 9, 20), dtype=torch.uint8)[:, :, ::2],           # a last dimension with a stride
                torch.zeros((9, 10), dtype=torch.uint8)):                        # rank
        with pytest.raises(ValueError):
            clips.check_nv12(bad)
    assert clips.check_nv12(torch.zeros((2, 12, 16), dtype=torch.uint8)[:, :9, :10]) == (6, 10)     # a pitched slice is fine
    with pytest.raises(ValueError):
        clips.nv12_to_rgb_host(ok, 'rec2020')
    with pytest.raises(ValueError):
        clips.rgb_to_nv12_host(torch.zeros((1, 5, 4, 3), dtype=torch.uint8))
    # the ops refuse by type before they look for a device
    boxes = torch.tensor([[0, 0, 4, 4]] * 2, dtype=torch.int32)
    for call in (lambda f: ops.nv12_to_rgb_u8(f), lambda f: ops.crop_resize_nv12(f, boxes, 4)):
        with pytest.raises(TypeError):
            call(ok.float())
        with pytest.raises(ValueError):
            call(torch.zeros((2, 8, 10), dtype=torch.uint8))
        with pytest.raises(ValueError):
            call(torch.zeros((2, 9, 9), dtype=torch.uint8))
        with pytest.raises(RuntimeError):
            call(torch.zeros((9, 10), dtype=torch.uint8))
        with pytest.raises(RuntimeError, match='ROCm'):                          # the arguments pass: the next stop is the device
            call(ok)
    with pytest.raises(ValueError):
        ops.nv12_to_rgb_u8(ok, matrix='bt2020')


def test_scorer_nv12_argument_errors_need_no_device(pkg):
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    nv = torch.zeros((5, 60, 50), dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 30, 30]] * 5, dtype=torch.int32)
    scorer = video.VideoScorer(model, side=32, pixel_format='nv12')
    assert scorer.pixel_format == 'nv12' and scorer.yuv_matrix == 'bt709'
    assert video.VideoScorer(model).pixel_format == 'rgb24'
    for call in (lambda: scorer.score(nv), lambda: scorer.push(nv), lambda: scorer.explain(nv),
                 lambda: scorer.score_videos([nv, nv]), lambda: model.score_video(nv, side=32, pixel_format='nv12'),
                 lambda: model.explain_video(nv, side=32, pixel_format='nv12'),
                 lambda: model.score_videos([nv], side=32, pixel_format='nv12')):
        with pytest.raises(ValueError, match='boxes'):
            call()
    with pytest.raises(ValueError):
        scorer.score(torch.zeros((5, 40, 50, 3), dtype=torch.uint8), boxes=boxes)      # packed RGB into an NV12 scorer
    with pytest.raises(ValueError):
        scorer.score(torch.zeros((5, 61, 50), dtype=torch.uint8), boxes=boxes)         # rows not divisible by 3
    with pytest.raises(IndexError):
        scorer.score(nv, boxes=torch.tensor([[20, 0, 30, 30]] * 5, dtype=torch.int32))  # the picture has 40 rows, not 60
    with pytest.raises(ValueError):
        video.VideoScorer(model, pixel_format='yuv420p')
    with pytest.raises(ValueError):
        video.VideoScorer(model, pixel_format='nv12', yuv_matrix='bt2020')
    with pytest.raises(RuntimeError, match='ROCm'):                                    # the arguments pass
        scorer.score(nv, boxes=boxes)
    with pytest.raises(RuntimeError, match='ROCm'):
        model.score_video(nv, boxes=boxes, side=32, pixel_format='nv12', yuv_matrix='bt601')


@pytest.mark.parametrize('matrix', ['bt601', 'bt709', 'jfif'])
def test_encoder_round_trip_on_flat_blocks(pkg, matrix):
    """rgb_to_nv12_host then nv12_to_rgb_host on an image whose 2 x 2 blocks are flat: within 2 levels (the encoder rounds Y
    and the chroma, the decoder rounds once more: a sanity bound, not a promise)"""
    from istvt_amd import clips
    g = torch.Generator().manual_seed(11)
    rgb = torch.randint(0, 256, (2, 20, 30, 3), generator=g, dtype=torch.uint8).repeat_interleave(2, 1).repeat_interleave(2, 2)
    nv = clips.rgb_to_nv12_host(rgb, matrix)
    assert nv.dtype == torch.uint8 and tuple(nv.shape) == (2, 60, 60) and nv.is_contiguous()
    back = clips.nv12_to_rgb_host(nv, matrix)
    d = int((back.to(torch.int32) - rgb.to(torch.int32)).abs().max())
    print('%s: max |round trip - image| = %d' % (matrix, d))
    assert d <= 2
