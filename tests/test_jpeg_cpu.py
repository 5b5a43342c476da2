"""JPEG round trip (DESIGN.md "JPEG round trip") without a device: the integer definition against PIL's recorded output,
the quantisation tables, fixed points, passthrough, per-clip tables, the random qualities and the validation."""
import os

import numpy as np
import pytest
import torch

SIZES = ((16, 16), (24, 40), (17, 33), (48, 48))
CASES = [(2, q) for q in (30, 50, 75, 90)] + [(0, 75)]         # (PIL's subsampling number, quality)
NAMES = {2: '420', 0: '444'}


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'J1_jpeg_pil.npz'))


def _mad(a, b):
    return float(np.abs(a.astype(np.int64) - b.astype(np.int64)).mean())


@pytest.mark.parametrize('h,w', SIZES)
def test_definition_against_pil(clips, fixture, h, w):
    """d = mean |definition - PIL(q)| <= half of PIL's own distance to the nearer of PIL(q - 10), PIL(q + 10): the definition
    is closer to the codec at its own quality than the codec is to itself one quality step away."""
    src = fixture['src_%dx%d' % (h, w)]
    for sub, q in CASES:
        pil = {d: fixture['pil_%dx%d_s%d_q%d' % (h, w, sub, q + d)] for d in (-10, 0, 10)}
        out = clips.jpeg_roundtrip_host(torch.from_numpy(src)[None], q, NAMES[sub])[0].numpy()
        d = _mad(out, pil[0])
        step = min(_mad(pil[0], pil[-10]), _mad(pil[0], pil[10]))
        print('%d x %d %s q=%d: d = %.4f, neighbour distance %.3f, ratio %.4f, bytes that differ %d of %d'
              % (h, w, NAMES[sub], q, d, step, d / step, int((out != pil[0]).sum()), out.size))
        assert d <= 0.5 * step, (h, w, sub, q, d, step)


def test_quant_tables(clips):
    t50 = clips.jpeg_quant_tables(50)
    assert t50.dtype == torch.int32 and tuple(t50.shape) == (2, 8, 8)
    assert t50[0].flatten().tolist() == list(clips.JPEG_LUMA) and t50[1].flatten().tolist() == list(clips.JPEG_CHROMA)
    assert t50[0, 0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and t50[0, 7, 7] == 99 and t50[0, 7, 0] == 72   # Annex K.1
    assert t50[1, 0].tolist() == [17, 18, 24, 47, 99, 99, 99, 99] and int(t50[1, 4:].min()) == 99                 # Annex K.2
    assert bool((clips.jpeg_quant_tables(100) == 1).all())
    t1 = clips.jpeg_quant_tables(1)
    assert int(t1.max()) == 255 and bool((t1 == 255).all())            # 16 * 5000 / 100 = 800 already: every entry clamps
    assert clips.jpeg_quant_tables(75)[0, 0, :4].tolist() == [8, 6, 5, 8]                 # (base * 50 + 50) // 100
    assert clips.jpeg_quant_tables(25)[0, 0, :2].tolist() == [32, 22]                     # s = 200
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            clips.jpeg_quant_tables(bad)


@pytest.mark.parametrize('sub', ['420', '444'])
def test_grey_is_a_fixed_point(clips, sub):
    grey = torch.full((1, 17, 23, 3), 128, dtype=torch.uint8)
    for q in range(1, 101):
        assert torch.equal(clips.jpeg_roundtrip_host(grey, q, sub), grey), q


def _frames(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_passthrough_and_determinism(clips):
    u8 = _frames(4, 19, 21, 3)
    q = torch.tensor([0, 60, -5, 20], dtype=torch.int32)
    out = clips.jpeg_roundtrip_host(u8, q)
    assert out.dtype == torch.uint8 and out.shape == u8.shape
    assert torch.equal(out[0], u8[0]) and torch.equal(out[2], u8[2])
    assert not torch.equal(out[1], u8[1]) and not torch.equal(out[3], u8[3])
    assert torch.equal(clips.jpeg_roundtrip_host(u8, q), out)                               # a second call: equal bytes
    assert torch.equal(out[1:2], clips.jpeg_roundtrip_host(u8[1:2], 60))                   # a frame does not see its batch
    # a lower quality loses more
    err = [float((clips.jpeg_roundtrip_host(u8, v).float() - u8.float()).abs().mean()) for v in (10, 50, 90, 100)]
    assert err[0] > err[1] > err[2] > err[3]


def test_per_clip_table(clips):
    u8 = _frames(6, 24, 40, 5).view(2, 3, 24, 40, 3)
    q = torch.tensor([35, 0], dtype=torch.int32)
    out = clips.jpeg_roundtrip_host(u8, q, '420')
    flat = clips.jpeg_roundtrip_host(u8.view(6, 24, 40, 3), q.repeat_interleave(3), '420')
    assert out.shape == u8.shape and torch.equal(out.view(6, 24, 40, 3), flat)
    assert torch.equal(out[1], u8[1])


def test_smallest_frames(clips):
    for h, w in ((1, 1), (1, 9), (2, 3), (8, 8)):
        for sub in ('420', '444'):
            u8 = _frames(1, h, w, h * 10 + w)
            assert clips.jpeg_roundtrip_host(u8, 100, sub).shape == u8.shape
    one = _frames(1, 1, 1, 9)
    # a single pixel is a flat block: only its DC survives, and quality 100 keeps it to the rounding of the colour transforms
    assert int((clips.jpeg_roundtrip_host(one, 100, '444').int() - one.int()).abs().max()) <= 2


def test_random_qualities(clips):
    a = clips.random_qualities(500, generator=torch.Generator().manual_seed(7))
    b = clips.random_qualities(500, generator=torch.Generator().manual_seed(7))
    assert torch.equal(a, b) and a.dtype == torch.int32 and a.is_contiguous() and tuple(a.shape) == (500,)
    on = a[a != 0]
    assert 150 < on.numel() < 350 and int(on.min()) >= 30 and int(on.max()) <= 95
    assert bool((clips.random_qualities(64, p=0.0) == 0).all())
    full = clips.random_qualities(400, p=1.0, lo=40, hi=43, generator=torch.Generator().manual_seed(1))
    assert sorted(set(full.tolist())) == [40, 41, 42, 43]
    assert clips.random_qualities(3, p=1.0, lo=77, hi=77).tolist() == [77, 77, 77]
    for kw in (dict(n=0), dict(n=4, p=1.5), dict(n=4, p=-0.1), dict(n=4, lo=0), dict(n=4, hi=101), dict(n=4, lo=60, hi=50)):
        with pytest.raises(ValueError):
            clips.random_qualities(**kw)
    clips.check_qualities(a, 500)


def test_check_qualities(clips):
    ok = torch.tensor([0, -1, 1, 100], dtype=torch.int32)
    assert torch.equal(clips.check_qualities(ok, 4), ok)
    assert clips.check_qualities(40, 3).tolist() == [40, 40, 40]
    with pytest.raises(TypeError):
        clips.check_qualities(ok.long(), 4)
    with pytest.raises(TypeError):
        clips.check_qualities([1, 2, 3, 4], 4)
    with pytest.raises(TypeError):
        clips.check_qualities(40.0, 4)
    with pytest.raises(ValueError):
        clips.check_qualities(ok, 5)
    with pytest.raises(ValueError):
        clips.check_qualities(ok.view(2, 2), 4)
    with pytest.raises(ValueError):
        clips.check_qualities(torch.tensor([50, 101], dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        clips.check_qualities(101, 2)
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        clips.jpeg_roundtrip_host(u8, 50, '422')
    with pytest.raises(ValueError):
        clips.jpeg_roundtrip_host(u8.float(), 50)
    with pytest.raises(ValueError):
        clips.jpeg_roundtrip_host(u8[..., :2], 50)


def test_entry_point_declared_and_exported(clips):
    from istvt_amd import ops, video
    assert callable(ops.jpeg_roundtrip_u8)                  # (header, table and library: test_abi_cpu.py)
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 50)            # a CPU tensor: no fallback
    import inspect
    assert inspect.signature(video.VideoScorer.__init__).parameters['jpeg_quality'].default is None


def test_scorer_checks_its_quality():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    for bad in (0, 101, 50.0, True):
        with pytest.raises(ValueError):
            video.VideoScorer(model, jpeg_quality=bad)
    s = video.VideoScorer(model, jpeg_quality=40)
    assert s.jpeg_quality == 40 and video.VideoScorer(model).jpeg_quality is None
    floats = torch.zeros((4, 3, 96, 96))
    for call in (lambda: s.score(floats), lambda: s.push(floats), lambda: s.score_videos([floats]), lambda: s.explain(floats)):
        with pytest.raises(TypeError):
            call()
