"""JPEG round trip (DESIGN.md "JPEG round trip") on a real MI355X: ops.jpeg_roundtrip_u8 against the integer definition
clips.jpeg_roundtrip_host, bit for bit; its arguments, its output bounds, graph capture, and VideoScorer(jpeg_quality=)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE_W = 64                    # JP_TILE_W of csrc/jpeg.hip: a workgroup's tile is one MCU row x TILE_W pixels
# (n, H, W): less than one MCU | exactly one (4:2:0) | half-MCU remainders | one-pixel remainders, odd chroma size | several
# tiles | one MCU (16 at 4:2:0, 8 at 4:4:4) wider than a tile | the real side
SHAPES = [(1, 5, 7), (1, 16, 16), (2, 24, 40), (3, 17, 33), (2, 48, 80), (2, 20, TILE_W + 16), (2, 9, TILE_W + 8),
          (1, 224, 224)]
MIX = (0, 1, 30, 75, 100)


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _random(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _smooth(n, h, w, seed):
    """the recipe of tests/golden/make_jpeg_golden.py: a sinusoid per channel around 128 plus N(0, 12) noise"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = np.stack([128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)], -1)
    img = np.clip(np.round(planes[None] + g.normal(0.0, 12.0, (n, h, w, 3))), 0, 255).astype(np.uint8)
    return torch.from_numpy(img)


def _table(n, first):
    """n qualities cycling through MIX from position `first`; the last frame always compresses"""
    q = [MIX[(first + i) % len(MIX)] for i in range(n)]
    if q[-1] == 0:
        q[-1] = 50
    return torch.tensor(q, dtype=torch.int32)


@pytest.mark.parametrize('sub', ['420', '444'])
@pytest.mark.parametrize('n,h,w', SHAPES)
def test_bit_identity(pkg, n, h, w, sub):
    from istvt_amd import clips, ops
    for k, src in enumerate((_random(n, h, w, h * 1000 + w), _smooth(n, h, w, h * 1000 + w))):
        for first in (1, 3):
            q = _table(n, first + k)
            got = ops.jpeg_roundtrip_u8(src.cuda(), q, sub).cpu()
            ref = clips.jpeg_roundtrip_host(src, q, sub)
            bad = int((got != ref).sum())
            print('%s (%d, %d, %d) q=%s: %d of %d bytes differ' % (sub, n, h, w, q.tolist(), bad, ref.numel()))
            assert torch.equal(got, ref)


@pytest.mark.parametrize('sub', ['420', '444'])
def test_mixed_table_in_one_batch(pkg, sub):
    """0, 1, 30, 75 and 100 in one batch of frames with partial MCUs (17 x 33), the last frame compressed; a frame's bytes do
    not depend on its batch, and a second run gives the same bits"""
    from istvt_amd import clips, ops
    src = torch.cat([_random(3, 17, 33, 1), _smooth(3, 17, 33, 2)])
    q = torch.tensor([0, 1, 30, 75, 100, 30], dtype=torch.int32)
    dev = src.cuda()
    got = ops.jpeg_roundtrip_u8(dev, q, sub)
    assert torch.equal(got.cpu(), clips.jpeg_roundtrip_host(src, q, sub))
    assert torch.equal(got[0], dev[0]) and not torch.equal(got[1], dev[1])
    assert torch.equal(ops.jpeg_roundtrip_u8(dev, q, sub), got)
    assert torch.equal(ops.jpeg_roundtrip_u8(dev[5:], q[5:].contiguous(), sub), got[5:])
    assert torch.equal(ops.jpeg_roundtrip_u8(dev, 75, sub)[3], got[3])                      # an int: that quality everywhere


def test_clips_with_a_per_clip_table(pkg):
    from istvt_amd import clips, ops
    src = _random(6, 24, 40, 11).view(2, 3, 24, 40, 3)
    q = torch.tensor([35, 0], dtype=torch.int32)
    got = ops.jpeg_roundtrip_u8(src.cuda(), q)
    assert got.shape == src.shape and torch.equal(got.cpu(), clips.jpeg_roundtrip_host(src, q))
    flat = ops.jpeg_roundtrip_u8(src.view(6, 24, 40, 3).cuda(), q.repeat_interleave(3))
    assert torch.equal(got.view(6, 24, 40, 3), flat) and torch.equal(got[1].cpu(), src[1])


def test_arguments(pkg):
    from istvt_amd import clips, ops
    src = _random(3, 17, 33, 4)
    dev = src.cuda()
    q = torch.tensor([20, 0, 90], dtype=torch.int32)
    ref = clips.jpeg_roundtrip_host(src, q)
    out = torch.empty_like(dev)
    assert ops.jpeg_roundtrip_u8(dev, q, out=out) is out and torch.equal(out.cpu(), ref)
    assert torch.equal(ops.jpeg_roundtrip_u8(dev, q.cuda(), checked=True).cpu(), ref)      # a checked device table
    # any slice of a larger buffer is a valid source, unaligned base included
    N = dev.numel()
    big = torch.zeros((N + 64,), dtype=torch.uint8, device='cuda')
    for lead in (1, 3, 16):
        big[lead:lead + N].copy_(dev.flatten())
        assert torch.equal(ops.jpeg_roundtrip_u8(big[lead:lead + N].view(3, 17, 33, 3), q).cpu(), ref)
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev, q, out=dev)                                            # in place
    both = torch.zeros((2 * N,), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(both[:N].view(3, 17, 33, 3), q, out=both[N - 8:2 * N - 8].view(3, 17, 33, 3))   # overlapping
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev[:, :, :16], q)                                          # not contiguous
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev.permute(0, 2, 1, 3), q)
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(src, q)                                                     # a CPU tensor
    with pytest.raises(TypeError):
        ops.jpeg_roundtrip_u8(dev.float(), q)
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev[..., :2].contiguous(), q)
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip_u8(dev, torch.tensor([20, 0, 101], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip_u8(dev, q[:2])
    with pytest.raises(TypeError):
        ops.jpeg_roundtrip_u8(dev, q.long())
    with pytest.raises(ValueError):
        ops.jpeg_roundtrip_u8(dev, q, '422')
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev, q, checked=True)                                       # checked wants a device table
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev, q.cuda())                                              # and a device table wants checked
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev, q, out=torch.empty((3, 17, 33, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(dev, q, out=torch.empty((3, 17, 32, 3), dtype=torch.uint8, device='cuda'))


@pytest.mark.parametrize('sub', ['420', '444'])
def test_output_bounds(pkg, sub):
    """4096 guard bytes in front of and behind the output keep their pattern: at a 4-byte aligned output (dword stores) and at
    an odd one (byte stores); the last frame ends in partial MCUs and the batch in a partial group of 4 pixels"""
    from istvt_amd import clips, ops
    src = _random(3, 17, 33, 8)
    q = torch.tensor([0, 40, 85], dtype=torch.int32)
    ref = clips.jpeg_roundtrip_host(src, q, sub)
    N, G = src.numel(), 4096
    for lead in (0, 1):
        buf = torch.full((G + lead + N + G,), 0xA5, dtype=torch.uint8, device='cuda')
        out = buf[G + lead:G + lead + N].view(3, 17, 33, 3)
        ops.jpeg_roundtrip_u8(src.cuda(), q, sub, out=out)
        host = buf.cpu()
        assert torch.equal(host[G + lead:G + lead + N].view(3, 17, 33, 3), ref)
        assert bool((host[:G + lead] == 0xA5).all()) and bool((host[G + lead + N:] == 0xA5).all())


def test_graph_capture(pkg):
    from istvt_amd import ops
    src = _smooth(4, 24, 40, 6).cuda()
    q = torch.tensor([30, 0, 75, 100], dtype=torch.int32).cuda()
    eager = ops.jpeg_roundtrip_u8(src, q, checked=True).clone()
    out = torch.zeros_like(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        ops.jpeg_roundtrip_u8(src, q, out=out, checked=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        ops.jpeg_roundtrip_u8(src, q, out=out, checked=True)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------- the scorer
@pytest.fixture(scope='module')
def small(pkg):
    """The `small` case of tests/test_video_gpu.py, rebuilt here: depth 2, T = 4, 96 x 96, float32, running statistics moved
    by one training forward; three uint8 videos of 4, 6 and 9 frames."""
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
    videos = [_smooth(n, side, side, 30 + n) for n in (4, 6, 9)]
    return dict(model=model, videos=videos, side=side)


def _same(a, b):
    return torch.equal(a.window_logits, b.window_logits) and torch.equal(a.logit_mean, b.logit_mean) and \
        torch.equal(a.prob_mean, b.prob_mean) and torch.equal(a.starts, b.starts)


def test_scorer_quality(small):
    from istvt_amd import ops, video
    model, frames = small['model'], small['videos'][2]
    plain = video.VideoScorer(model)
    base = plain.score(frames)
    res = video.VideoScorer(model, jpeg_quality=40).score(frames)
    assert _same(res, plain.score(ops.jpeg_roundtrip_u8(frames.cuda(), 40)))
    assert not torch.equal(res.window_logits, base.window_logits)                   # the recompression reaches the logits
    assert _same(video.VideoScorer(model, jpeg_quality=None).score(frames), base)
    assert _same(model.score_video(frames, jpeg_quality=40), res)
    # streaming: the windows of score()
    s = video.VideoScorer(model, jpeg_quality=40, frame_batch=4)
    parts = [s.push(frames[:5])[0], s.push(frames[5:])[0], s.flush()[0]]
    assert torch.equal(torch.cat(parts), res.window_logits)
    ex = video.VideoScorer(model, jpeg_quality=40).explain(frames)
    ref = plain.explain(ops.jpeg_roundtrip_u8(frames.cuda(), 40))
    assert torch.equal(ex.frame_s, ref.frame_s) and torch.equal(ex.score.window_logits, ref.score.window_logits)
    with pytest.raises(TypeError):
        video.VideoScorer(model, jpeg_quality=40).score(torch.zeros((4, 3, 96, 96)))


def test_scorer_quality_with_boxes(small):
    from istvt_amd import ops, video
    model, side = small['model'], small['side']
    full = _smooth(6, 120, 150, 77)
    boxes = torch.tensor([[3 + i, 5 + 2 * i, 100, 110 + i] for i in range(6)], dtype=torch.int32)
    crops = ops.jpeg_roundtrip_u8(ops.crop_resize_u8(full.cuda(), boxes, side), 40)
    res = video.VideoScorer(model, side=side, jpeg_quality=40).score(full, boxes=boxes)
    assert _same(res, video.VideoScorer(model).score(crops))


def test_scorer_quality_score_videos(small):
    from istvt_amd import ops, video
    model, videos = small['model'], small['videos']
    res = video.VideoScorer(model, jpeg_quality=40, frame_batch=8).score_videos(videos)
    ref = video.VideoScorer(model, frame_batch=8).score_videos([ops.jpeg_roundtrip_u8(v.cuda(), 40) for v in videos])
    assert torch.equal(res.window_logits, ref.window_logits) and torch.equal(res.logit_mean, ref.logit_mean)
    assert torch.equal(res.prob_mean, ref.prob_mean) and torch.equal(res.offsets, ref.offsets)
    assert torch.equal(model.score_videos(videos, jpeg_quality=40, frame_batch=8).window_logits, res.window_logits)
    base = video.VideoScorer(model, frame_batch=8).score_videos(videos)
    none = video.VideoScorer(model, frame_batch=8, jpeg_quality=None).score_videos(videos)
    assert torch.equal(none.window_logits, base.window_logits) and not torch.equal(res.window_logits, base.window_logits)
