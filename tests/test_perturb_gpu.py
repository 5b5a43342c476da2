"""Perturbations (DESIGN.md "Perturbations") on a real MI355X: ops.perturb_u8 against the integer definition
clips.perturb_host, bit for bit; its arguments, its output bounds, graph capture, and VideoScorer(perturb=)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE_W = 64                    # PT_TILE_W of csrc/perturb.hip: a workgroup's tile is 16 rows x TILE_W pixels
# (n, H, W): smaller than every halo and block | odd sizes | multiples of 8 | a quarter tile past one tile | tiles and halos
# cross in both directions, partial last tile | the real side
SHAPES = [(1, 5, 7), (3, 17, 33), (2, 24, 40), (2, 20, TILE_W + 16), (2, 37, 2 * TILE_W + 22), (1, 224, 224)]
SIGMAS = (0.5, 3.5)
# (kind, param) of every case: gains 0, 102, 256, 1024; noise 1, 160, 1023; both rows of the bank; blocks 2, 3, 8, 32
CASES = [(0, 0)] + [(k, p) for k in (1, 2, 3) for p in (0, 102, 256, 1024)] + [(4, p) for p in (1, 160, 1023)] + \
        [(5, 0), (5, 1)] + [(6, k) for k in (2, 3, 8, 32)]


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module', autouse=True)
def _one_host_thread():
    """the definition is many small int32 tensor operations: one thread runs it many times faster than a pool does"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _random(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _smooth(n, h, w, seed):
    """the recipe of tests/test_jpeg_gpu.py: a sinusoid per channel around 128 plus N(0, 12) noise"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = np.stack([128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)], -1)
    img = np.clip(np.round(planes[None] + g.normal(0.0, 12.0, (n, h, w, 3))), 0, 255).astype(np.uint8)
    return torch.from_numpy(img)


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize('n,h,w', SHAPES)
def test_bit_identity(pkg, n, h, w):
    """every kind at every param, on random and on smooth bytes.  The cases of a shape go through the device as one batch
    (frame i of the batch = source frame i % n through case i // n, with its own frame id) and through the definition one
    case at a time, so the reference is computed once per case."""
    from istvt_amd import clips, ops
    taps = clips.gaussian_taps(list(SIGMAS))
    seed = 0x1234567890abcdef
    for k, src in enumerate((_random(n, h, w, h * 1000 + w), _smooth(n, h, w, h * 1000 + w))):
        rows = [[kind, p, 3 * i + f, k + 1] for i, (kind, p) in enumerate(CASES) for f in range(n)]
        got = ops.perturb_u8(src.repeat(len(CASES), 1, 1, 1).cuda(), _table(rows), taps, seed).cpu()
        for i, (kind, p) in enumerate(CASES):
            ref = clips.perturb_host(src, _table(rows[i * n:(i + 1) * n]), taps, seed)
            bad = int((got[i * n:(i + 1) * n] != ref).sum())
            print('(%d, %d, %d) %s kind %d param %d: %d of %d bytes differ' % (n, h, w, ('random', 'smooth')[k], kind, p, bad,
                                                                             ref.numel()))
            assert bad == 0


def _mixed():
    """8 frames of 17 x 33 through all seven kinds; the last frame is blurred"""
    src = torch.cat([_random(4, 17, 33, 1), _smooth(4, 17, 33, 2)])
    rows = [[0, 0, 0, 0], [1, 300, 1, 0], [2, 102, 2, 0], [3, 51, 3, 1], [4, 160, 4, 1], [5, 1, 5, 1], [6, 3, 6, 2], [5, 0, 7, 2]]
    return src, _table(rows)


def test_mixed_batch_and_independence(pkg):
    from istvt_amd import clips, ops
    src, tab = _mixed()
    taps = clips.gaussian_taps(list(SIGMAS))
    dev = src.cuda()
    got = ops.perturb_u8(dev, tab, taps, 11)
    assert torch.equal(got.cpu(), clips.perturb_host(src, tab, taps, 11))
    assert torch.equal(got[0], dev[0]) and all(not torch.equal(got[i], dev[i]) for i in range(1, 8))
    assert torch.equal(ops.perturb_u8(dev, tab, taps, 11), got)                     # a second run: the same bits
    for lo, hi in ((5, 8), (2, 5), (4, 5)):                                         # a frame does not depend on its batch
        assert torch.equal(ops.perturb_u8(dev[lo:hi], tab[lo:hi].contiguous(), taps, 11), got[lo:hi])
    assert not torch.equal(ops.perturb_u8(dev, tab, taps, 12)[4], got[4])           # the seed reaches the noise ...
    assert torch.equal(ops.perturb_u8(dev, tab, taps, 12)[:4], got[:4])             # ... and nothing else


def test_clips_with_a_per_clip_table(pkg):
    from istvt_amd import clips, ops
    src = _random(6, 24, 40, 11).view(2, 3, 24, 40, 3)
    taps = clips.gaussian_taps(list(SIGMAS))
    for rows in ([[4, 200, 7, 1], [5, 1, 0, 0]], [[2, 400, 0, 0], [6, 3, 1, 1]], [[0, 0, 0, 0], [3, 0, 0, 0]]):
        tab = _table(rows)
        got = ops.perturb_u8(src.cuda(), tab, taps, 5)
        assert got.shape == src.shape and torch.equal(got.cpu(), clips.perturb_host(src, tab, taps, 5))
        flat = _table([r[:2] + [r[2] + t, r[3]] for r in rows for t in range(3)])
        assert torch.equal(got.view(6, 24, 40, 3), ops.perturb_u8(src.view(6, 24, 40, 3).cuda(), flat, taps, 5))


def test_arguments(pkg):
    from istvt_amd import clips, ops
    src = _random(3, 17, 33, 4)
    dev = src.cuda()
    taps = clips.gaussian_taps(list(SIGMAS))
    tab = _table([[4, 160, 0, 0], [5, 1, 1, 0], [6, 3, 2, 0]])
    ref = clips.perturb_host(src, tab, taps, 9)
    out = torch.empty_like(dev)
    assert ops.perturb_u8(dev, tab, taps, 9, out=out) is out and torch.equal(out.cpu(), ref)
    assert torch.equal(ops.perturb_u8(dev, tab.cuda(), taps.cuda(), 9, checked=True).cpu(), ref)   # a checked device table
    # any slice of a larger buffer is a valid source, unaligned base included
    N = dev.numel()
    big = torch.zeros((N + 64,), dtype=torch.uint8, device='cuda')
    for lead in (1, 3, 16):
        big[lead:lead + N].copy_(dev.flatten())
        assert torch.equal(ops.perturb_u8(big[lead:lead + N].view(3, 17, 33, 3), tab, taps, 9).cpu(), ref)
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev, tab, taps, out=dev)                                           # in place
    both = torch.zeros((2 * N,), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError):
        ops.perturb_u8(both[:N].view(3, 17, 33, 3), tab, taps, out=both[N - 8:2 * N - 8].view(3, 17, 33, 3))   # overlapping
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev[:, :, :16], tab, taps)                                         # not contiguous
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev.permute(0, 2, 1, 3), tab, taps)
    with pytest.raises(RuntimeError):
        ops.perturb_u8(src, tab, taps)                                                    # a CPU tensor
    with pytest.raises(TypeError):
        ops.perturb_u8(dev.float(), tab, taps)
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev[..., :2].contiguous(), tab, taps)
    with pytest.raises(ValueError):
        ops.perturb_u8(dev, _table([[4, 1024, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]))
    with pytest.raises(ValueError):
        ops.perturb_u8(dev, tab)                                                          # a blurred frame and no taps
    with pytest.raises(ValueError):
        ops.perturb_u8(dev, tab[:2], taps)
    with pytest.raises(TypeError):
        ops.perturb_u8(dev, tab.long(), taps)
    with pytest.raises(ValueError):
        ops.perturb_u8(dev, tab, taps, seed=-1)
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev, tab, taps, checked=True)                                      # checked wants a device table
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev, tab.cuda(), taps)                                             # and a device table wants checked
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev, tab, taps.cuda())
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev, tab, taps, out=torch.empty((3, 17, 33, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ops.perturb_u8(dev, tab, taps, out=torch.empty((3, 17, 32, 3), dtype=torch.uint8, device='cuda'))


def test_output_bounds(pkg):
    """4096 guard bytes in front of and behind the output keep their pattern: at a 4-byte aligned output (dword stores) and at
    an odd one (byte stores), for a batch that mixes a point kind, blur and pixelate; the frames end in partial tiles and
    blocks and the batch in a partial group of 4 pixels"""
    from istvt_amd import clips, ops
    src = _random(3, 17, 33, 8)
    taps = clips.gaussian_taps(list(SIGMAS))
    for rows in ([[3, 102, 0, 0], [5, 1, 1, 0], [6, 8, 2, 0]], [[6, 3, 0, 0], [4, 160, 1, 0], [5, 0, 2, 0]]):
        tab = _table(rows)
        ref = clips.perturb_host(src, tab, taps, 2)
        N, G = src.numel(), 4096
        for lead in (0, 1):
            buf = torch.full((G + lead + N + G,), 0xA5, dtype=torch.uint8, device='cuda')
            out = buf[G + lead:G + lead + N].view(3, 17, 33, 3)
            ops.perturb_u8(src.cuda(), tab, taps, 2, out=out)
            host = buf.cpu()
            assert torch.equal(host[G + lead:G + lead + N].view(3, 17, 33, 3), ref)
            assert bool((host[:G + lead] == 0xA5).all()) and bool((host[G + lead + N:] == 0xA5).all())


def test_graph_capture(pkg):
    from istvt_amd import clips, ops
    src, tab = _mixed()
    src, tab = src.cuda(), tab.cuda()
    taps = clips.gaussian_taps(list(SIGMAS)).cuda()
    eager = ops.perturb_u8(src, tab, taps, 3, checked=True).clone()
    out = torch.zeros_like(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        ops.perturb_u8(src, tab, taps, 3, out=out, checked=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        ops.perturb_u8(src, tab, taps, 3, out=out, checked=True)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------- the scorer
@pytest.fixture(scope='module')
def small(pkg):
    """The `small` case of tests/test_jpeg_gpu.py, rebuilt here: depth 2, T = 4, 96 x 96, float32, running statistics moved
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


PERTURBS = [('blur', 2.0), ('noise', 10.0)]
SEED = 77


def _perturbed(frames, P, stream=0):
    from istvt_amd import clips, ops
    tab, taps = clips.perturbation_table(int(frames.shape[0]), *P, stream=stream)
    return ops.perturb_u8(frames.cuda(), tab, taps, SEED)


@pytest.mark.parametrize('P', PERTURBS, ids=lambda P: P[0])
def test_scorer_perturb(small, P):
    from istvt_amd import video
    model, frames = small['model'], small['videos'][2]
    plain = video.VideoScorer(model)
    base = plain.score(frames)
    res = video.VideoScorer(model, perturb=P, perturb_seed=SEED).score(frames)
    assert _same(res, plain.score(_perturbed(frames, P)))
    assert not torch.equal(res.window_logits, base.window_logits)                   # the perturbation reaches the logits
    assert _same(video.VideoScorer(model, perturb=None).score(frames), base)
    assert _same(model.score_video(frames, perturb=P, perturb_seed=SEED), res)
    # streaming: the windows of score(), the frame ids counted across the pushes
    s = video.VideoScorer(model, perturb=P, perturb_seed=SEED, frame_batch=4)
    parts = [s.push(frames[:5])[0], s.push(frames[5:])[0], s.flush()[0]]
    assert torch.equal(torch.cat(parts), res.window_logits)
    ex = video.VideoScorer(model, perturb=P, perturb_seed=SEED).explain(frames)
    ref = plain.explain(_perturbed(frames, P))
    assert torch.equal(ex.frame_s, ref.frame_s) and torch.equal(ex.score.window_logits, ref.score.window_logits)
    with pytest.raises(TypeError):
        video.VideoScorer(model, perturb=P).score(torch.zeros((4, 3, 96, 96)))


@pytest.mark.parametrize('P', PERTURBS, ids=lambda P: P[0])
def test_scorer_perturb_with_boxes_and_jpeg(small, P):
    from istvt_amd import ops, video
    model, side = small['model'], small['side']
    full = _smooth(6, 120, 150, 77)
    boxes = torch.tensor([[3 + i, 5 + 2 * i, 100, 110 + i] for i in range(6)], dtype=torch.int32)
    crops = _perturbed(ops.crop_resize_u8(full.cuda(), boxes, side), P)
    res = video.VideoScorer(model, side=side, perturb=P, perturb_seed=SEED).score(full, boxes=boxes)
    assert _same(res, video.VideoScorer(model).score(crops))
    # with jpeg_quality too: the perturbed crops are compressed, not the reverse
    both = video.VideoScorer(model, side=side, perturb=P, perturb_seed=SEED, jpeg_quality=40).score(full, boxes=boxes)
    assert _same(both, video.VideoScorer(model).score(ops.jpeg_roundtrip_u8(crops, 40)))
    assert not torch.equal(both.window_logits, res.window_logits)


@pytest.mark.parametrize('P', PERTURBS, ids=lambda P: P[0])
def test_scorer_perturb_score_videos(small, P):
    from istvt_amd import video
    model, videos = small['model'], small['videos']
    res = video.VideoScorer(model, perturb=P, perturb_seed=SEED, frame_batch=8).score_videos(videos)
    ref = video.VideoScorer(model, frame_batch=8).score_videos([_perturbed(v, P, stream=i) for i, v in enumerate(videos)])
    assert torch.equal(res.window_logits, ref.window_logits) and torch.equal(res.logit_mean, ref.logit_mean)
    assert torch.equal(res.prob_mean, ref.prob_mean) and torch.equal(res.offsets, ref.offsets)
    assert torch.equal(model.score_videos(videos, perturb=P, perturb_seed=SEED, frame_batch=8).window_logits, res.window_logits)
    base = video.VideoScorer(model, frame_batch=8).score_videos(videos)
    none = video.VideoScorer(model, frame_batch=8, perturb=None).score_videos(videos)
    assert torch.equal(none.window_logits, base.window_logits) and not torch.equal(res.window_logits, base.window_logits)
