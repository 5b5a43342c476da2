"""NV12 frames (DESIGN.md "NV12 frames") on a real MI355X: istvt_nv12_to_rgb_u8 against the integer host definition, bit
for bit; istvt_crop_resize_nv12 against istvt_crop_resize_u8 on the converted frames, bit for bit (the same filter code
sees the same bytes); and the scorer's pixel_format='nv12' against the RGB scorer on crops made beforehand."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MATRICES = ('bt601', 'bt709', 'jfif')


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _nv12(n, Hs, Ws, seed):
    """random bytes in every plane: values outside the nominal range are legal and clamp"""
    return torch.randint(0, 256, (n, Hs + Hs // 2, Ws), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _pitched(nv, pitch, fstride=None, offset=0, fill=0):
    """the frames of `nv` (host) on the device inside one allocation with a row pitch, a frame stride and a byte offset:
    -> (the as_strided view, the whole allocation)"""
    n, rows, Ws = nv.shape
    fstride = rows * pitch if fstride is None else fstride
    store = torch.full((offset + n * fstride + 64,), fill, dtype=torch.uint8, device='cuda')
    view = store.as_strided((n, rows, Ws), (fstride, pitch, 1), offset)
    view.copy_(nv)
    return view, store


# ---- whole frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('Hs,Ws', [(2, 2), (6, 10), (34, 50)])
def test_to_rgb_equals_the_host_definition(pkg, Hs, Ws, matrix):
    from istvt_amd import clips, ops
    nv = _nv12(3, Hs, Ws, Hs * 100 + Ws)
    want = clips.nv12_to_rgb_host(nv, matrix)
    got = ops.nv12_to_rgb_u8(nv.cuda(), matrix)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, Hs, Ws, 3) and got.is_cuda and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.nv12_to_rgb_u8(nv.cuda(), matrix), got)                       # a second run: the same bits


@pytest.mark.parametrize('matrix', MATRICES)
def test_to_rgb_every_luma_against_extreme_chroma(pkg, matrix):
    """every Y value against chroma 0, 16, 128, 240, 255 in both components: the clamps on both sides"""
    from istvt_amd import clips, ops
    cs = (0, 16, 128, 240, 255)
    nv = torch.empty((len(cs) * len(cs), 3, 512), dtype=torch.uint8)
    for i, cb in enumerate(cs):
        for j, cr in enumerate(cs):
            f = nv[i * len(cs) + j]
            f[0] = torch.arange(256).repeat_interleave(2).to(torch.uint8)
            f[1] = torch.arange(255, -1, -1).repeat_interleave(2).to(torch.uint8)
            f[2, 0::2], f[2, 1::2] = cb, cr
    want = clips.nv12_to_rgb_host(nv, matrix)
    assert int(want.min()) == 0 and int(want.max()) == 255
    assert torch.equal(ops.nv12_to_rgb_u8(nv.cuda(), matrix).cpu(), want)


def test_to_rgb_pitch_slices_offsets_and_guards(pkg):
    from istvt_amd import clips, ops
    Hs, Ws = 34, 50
    nv = _nv12(3, Hs, Ws, 5)
    want = clips.nv12_to_rgb_host(nv, 'bt709')
    view, _ = _pitched(nv, 64)                                                           # pitch 64 for width 50
    assert torch.equal(ops.nv12_to_rgb_u8(view, 'bt709').cpu(), want)
    assert torch.equal(ops.nv12_to_rgb_u8(nv.cuda()[1:], 'bt709').cpu(), want[1:])       # frames[1:] of a batch
    odd, _ = _pitched(nv, Ws, offset=7)                                                  # an odd byte offset in its allocation
    assert odd.data_ptr() % 2 == 1 and torch.equal(ops.nv12_to_rgb_u8(odd, 'bt709').cpu(), want)
    far, _ = _pitched(nv, 80, fstride=51 * 80 + 13, offset=3)                            # frames further apart than their rows
    assert torch.equal(ops.nv12_to_rgb_u8(far, 'bt709').cpu(), want)
    four = nv.cuda()[:2].reshape(1, 2, Hs + Hs // 2, Ws)                                 # clips
    assert torch.equal(ops.nv12_to_rgb_u8(four, 'bt709').cpu(), want[:2].reshape(1, 2, Hs, Ws, 3))
    # guard bytes in front of and behind input and output, unchanged afterwards; their value must not show
    G, N, M = 4099, nv.numel(), want.numel()
    for sentinel in (0, 255, 171):
        buf = torch.full((G + N + G,), sentinel, dtype=torch.uint8, device='cuda')
        buf[G:G + N] = nv.cuda().view(-1)
        obuf = torch.full((5 + M + 64,), sentinel, dtype=torch.uint8, device='cuda')
        got = ops.nv12_to_rgb_u8(buf[G:G + N].view(3, Hs + Hs // 2, Ws), 'bt709', out=obuf[5:5 + M].view(3, Hs, Ws, 3))
        assert torch.equal(got.cpu(), want)
        assert bool((buf[:G] == sentinel).all()) and bool((buf[G + N:] == sentinel).all())
        assert bool((obuf[:5] == sentinel).all()) and bool((obuf[5 + M:] == sentinel).all())


# ---- the fused crop ---------------------------------------------------------------------------------------------------
def _crop_boxes(Hs, Ws, S):
    boxes = [(3, 5, 11, 9),                                  # odd origin, odd sides
             (1, 1, 1, 1), (Hs - 1, Ws - 1, 1, 1), (4, 7, 1, 1),   # 1 x 1
             (7, 9, S, S),                                   # identity at an odd origin
             (0, 0, Hs, Ws), (2, 3, Hs - 2, Ws - 3),         # flush with the right and bottom edges
             (Hs - 20, Ws - 25, 20, 25), (5, 0, 21, Ws), (0, 6, Hs, 13),
             (1, 1, min(8 * S, Hs - 1), min(8 * S, Ws - 1))]       # the 8 S box: a 17-tap axis where it fits
    return [b for b in boxes if b[2] <= 8 * S and b[3] <= 8 * S]


@pytest.mark.parametrize('matrix', MATRICES)
@pytest.mark.parametrize('S', [8, 24])
def test_fused_crop_equals_convert_then_crop(pkg, S, matrix):
    from istvt_amd import ops
    Hs, Ws = 66, 70
    boxes = _crop_boxes(Hs, Ws, S)
    assert (1, 1, 64, 64) in boxes or S != 8                                             # 8 S at S = 8: 17 taps, one row per pass
    nv = _nv12(len(boxes), Hs, Ws, S)
    b = torch.tensor(boxes, dtype=torch.int32)
    dev = nv.cuda()
    rgb = ops.nv12_to_rgb_u8(dev, matrix)
    want = ops.crop_resize_u8(rgb, b, S)
    got = ops.crop_resize_nv12(dev, b, S, matrix)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(boxes), S, S, 3)
    assert torch.equal(got, want)
    assert torch.equal(ops.crop_resize_nv12(dev, b, S, matrix), got)                     # a second run: the same bits
    i = boxes.index((7, 9, S, S))
    assert torch.equal(got[i], rgb[i, 7:7 + S, 9:9 + S])                                 # identity reproduces the converted slice
    # pitched, sliced and offset sources, and `out` at an odd offset with guards
    view, _ = _pitched(nv, 96, fstride=100 * 96 + 5, offset=9, fill=255)
    assert torch.equal(ops.crop_resize_nv12(view, b, S, matrix), want)
    assert torch.equal(ops.crop_resize_nv12(dev[2:], b[2:].contiguous(), S, matrix), want[2:])
    M = want.numel()
    obuf = torch.full((3 + M + 64,), 9, dtype=torch.uint8, device='cuda')
    got = ops.crop_resize_nv12(dev, b, S, matrix, out=obuf[3:3 + M].view(want.shape))
    assert torch.equal(got, want) and bool((obuf[:3] == 9).all()) and bool((obuf[3 + M:] == 9).all())


def test_fused_crop_clips_and_strided_clips(pkg):
    from istvt_amd import ops
    Hs, Ws, S = 66, 70, 24
    nv = _nv12(6, Hs, Ws, 31).cuda()
    boxes = torch.tensor([(3, 5, 41, 39), (10, 1, 56, 69)], dtype=torch.int32)
    flat = ops.crop_resize_nv12(nv, boxes.repeat_interleave(3, dim=0), S)
    four = nv.view(2, 3, Hs + Hs // 2, Ws)
    assert torch.equal(ops.crop_resize_nv12(four, boxes, S).view(6, S, S, 3), flat)
    big = torch.zeros((2, 5, Hs + Hs // 2, Ws), dtype=torch.uint8, device='cuda')        # clip stride != T frame strides
    big[:, 1:4] = four
    assert torch.equal(ops.crop_resize_nv12(big[:, 1:4], boxes, S).view(6, S, S, 3), flat)
    assert torch.equal(ops.nv12_to_rgb_u8(big[:, 1:4]).view(6, Hs, Ws, 3), ops.nv12_to_rgb_u8(nv))


def test_fused_crop_at_the_models_side(pkg):
    """S = 224 from two 1080 x 1920 frames: more than 64 KiB of LDS"""
    from istvt_amd import ops
    nv = _nv12(2, 1080, 1920, 224).cuda()
    boxes = torch.tensor([(101, 203, 601, 599), (1080 - 1079, 1920 - 1793, 1079, 1792)], dtype=torch.int32)
    want = ops.crop_resize_u8(ops.nv12_to_rgb_u8(nv), boxes, 224)
    assert torch.equal(ops.crop_resize_nv12(nv, boxes, 224), want)


def test_bytes_no_box_pixel_maps_to_do_not_matter(pkg):
    from istvt_amd import ops
    Hs, Ws, S = 34, 50, 8
    boxes = [(3, 5, 11, 9), (10, 20, 20, 24), (33, 49, 1, 1)]
    a = _nv12(3, Hs, Ws, 41)
    b = _nv12(3, Hs, Ws, 42)
    for i, (y0, x0, h, w) in enumerate(boxes):
        b[i, y0:y0 + h, x0:x0 + w] = a[i, y0:y0 + h, x0:x0 + w]
        # an odd origin shares its first pair with the outside neighbour: the pairs (y >> 1, x >> 1) of all box pixels
        cy0, cy1, cx0, cx1 = y0 >> 1, (y0 + h - 1) >> 1, x0 >> 1, (x0 + w - 1) >> 1
        b[i, Hs + cy0:Hs + cy1 + 1, 2 * cx0:2 * cx1 + 2] = a[i, Hs + cy0:Hs + cy1 + 1, 2 * cx0:2 * cx1 + 2]
    assert not torch.equal(a[:, :Hs], b[:, :Hs]) and not torch.equal(a[:, Hs:], b[:, Hs:])
    t = torch.tensor(boxes, dtype=torch.int32)
    assert torch.equal(ops.crop_resize_nv12(a.cuda(), t, S), ops.crop_resize_nv12(b.cuda(), t, S))


def test_unvalidated_table_stays_inside(pkg):
    """checked=True hands over a table nobody validated: boxes outside the frame are forced into it, and nothing around the
    frames or the output is touched"""
    from istvt_amd import ops
    Hs, Ws, S = 34, 50, 8
    nv = _nv12(3, Hs, Ws, 51)
    G, N, M = 4099, nv.numel(), 3 * S * S * 3
    buf = torch.full((G + N + G,), 171, dtype=torch.uint8, device='cuda')
    buf[G:G + N] = nv.cuda().view(-1)
    obuf = torch.full((5 + M + 64,), 171, dtype=torch.uint8, device='cuda')
    wild = torch.tensor([(-5, -7, 20, 20), (30, 45, 900, 900), (1 << 30, 1 << 30, -3, 0)], dtype=torch.int32, device='cuda')
    got = ops.crop_resize_nv12(buf[G:G + N].view(3, Hs + Hs // 2, Ws), wild, S, out=obuf[5:5 + M].view(3, S, S, 3), checked=True)
    forced = torch.tensor([(0, 0, 20, 20), (0, 0, Hs, Ws), (Hs - 1, Ws - 1, 1, 1)], dtype=torch.int32)
    assert torch.equal(got, ops.crop_resize_nv12(nv.cuda(), forced, S))
    assert bool((buf[:G] == 171).all()) and bool((buf[G + N:] == 171).all())
    assert bool((obuf[:5] == 171).all()) and bool((obuf[5 + M:] == 171).all())


def test_refusals_before_any_launch(pkg):
    from istvt_amd import ops
    dev = _nv12(2, 34, 50, 61).cuda()
    ok = torch.tensor([[0, 0, 10, 10]] * 2, dtype=torch.int32)
    with pytest.raises(IndexError):
        ops.crop_resize_nv12(dev, torch.tensor([[0, 0, 10, 10], [30, 0, 8, 10]], dtype=torch.int32), 8)    # 34 rows of picture
    with pytest.raises(ValueError):
        ops.crop_resize_nv12(dev, ok, 481)
    with pytest.raises(ValueError):
        ops.crop_resize_nv12(dev, ok, 8, matrix='bt2020')
    with pytest.raises(TypeError):
        ops.crop_resize_nv12(dev, ok.to(torch.int64), 8)
    with pytest.raises(RuntimeError):
        ops.crop_resize_nv12(dev, ok, 8, out=torch.empty((2, 8, 8, 3), dtype=torch.uint8))
    buf = torch.zeros((20000,), dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError):                                                                    # out over the frames
        ops.nv12_to_rgb_u8(buf[:5100].view(2, 51, 50), out=buf[100:100 + 10200].view(2, 34, 50, 3))
    torch.cuda.synchronize()


# ---- the scorer -------------------------------------------------------------------------------------------------------
SIDE = 96


@pytest.fixture(scope='module')
def boxed(pkg):
    """the tiny configuration of the video tests: T = 4, side 96, depth 2, float32, a seeded random model in eval mode; 11
    NV12 frames of 140 x 170 with boxes of side 60..140, and a second video of 7 frames of 120 x 200"""
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

    def video(n, Hs, Ws, seed):
        nv = _nv12(n, Hs, Ws, seed)
        h = torch.randint(60, min(Hs, 140) + 1, (n,), generator=g)
        w = torch.randint(60, 141, (n,), generator=g)
        y0 = torch.minimum((torch.rand(n, generator=g) * (Hs - h + 1).float()).long(), Hs - h)
        x0 = torch.minimum((torch.rand(n, generator=g) * (Ws - w + 1).float()).long(), Ws - w)
        boxes = torch.stack([y0, x0, h, w], dim=1).to(torch.int32)
        return nv, boxes, ops.crop_resize_nv12(nv.cuda(), boxes, SIDE)

    nv, boxes, crops = video(11, 140, 170, 22)
    nv2, boxes2, crops2 = video(7, 120, 200, 23)
    return dict(model=model, nv=nv, boxes=boxes, crops=crops, nv2=nv2, boxes2=boxes2, crops2=crops2)


def test_score_nv12_is_score_on_crops(boxed):
    from istvt_amd import video
    rgb = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE)
    scorer = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE, pixel_format='nv12')
    ref = rgb.score(boxed['crops'])
    for frames in (boxed['nv'], boxed['nv'].cuda()):                             # host frames and device frames
        res = scorer.score(frames, boxes=boxed['boxes'])
        assert torch.isfinite(res.window_logits).all() and res.starts.tolist() == ref.starts.tolist()
        assert torch.equal(res.window_logits, ref.window_logits)
        assert torch.equal(res.logit_mean, ref.logit_mean) and torch.equal(res.prob_mean, ref.prob_mean)
    res = boxed['model'].score_video(boxed['nv'], boxes=boxed['boxes'], frame_batch=4, side=SIDE, pixel_format='nv12')
    assert torch.equal(res.window_logits, ref.window_logits)
    # another matrix is another picture
    other = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE, pixel_format='nv12', yuv_matrix='bt601')
    assert not torch.equal(other.score(boxed['nv'], boxes=boxed['boxes']).window_logits, ref.window_logits)
    with pytest.raises(ValueError, match='boxes'):
        scorer.score(boxed['nv'].cuda())


def test_push_nv12_agrees_with_score(boxed):
    from istvt_amd import video
    nv, boxes = boxed['nv'], boxed['boxes']
    scorer = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE, pixel_format='nv12')
    ref = scorer.score(nv, boxes=boxes)
    outs, starts = [], []
    for lo, hi in ((0, 4), (4, 11)):                                             # two uneven chunks
        l, s = scorer.push(nv[lo:hi], boxes=boxes[lo:hi].contiguous())
        outs.append(l), starts.extend(s.tolist())
    l, s = scorer.flush()
    outs.append(l), starts.extend(s.tolist())
    assert starts == ref.starts.tolist()
    d = float((torch.cat(outs) - ref.window_logits).abs().max())
    print('push 4 + 7 of NV12 frames vs score: max abs diff %.3e' % d)
    assert d <= 1e-5
    scorer.reset()
    with pytest.raises(ValueError, match='boxes'):
        scorer.push(nv[:4])


def test_score_videos_nv12_is_the_per_video_score(boxed):
    from istvt_amd import video
    scorer = video.VideoScorer(boxed['model'], frame_batch=4, window_batch=3, side=SIDE, pixel_format='nv12')
    res = scorer.score_videos([boxed['nv'], boxed['nv2'].cuda()], boxes=[boxed['boxes'], boxed['boxes2']], labels=[1, 0])
    off = res.offsets.tolist()
    for v, (nv, b) in enumerate(((boxed['nv'], boxed['boxes']), (boxed['nv2'], boxed['boxes2']))):
        one = scorer.score(nv, boxes=b)
        mine = res.window_logits[off[v]:off[v + 1]].double()
        d = float((mine - one.window_logits.double()).norm() / one.window_logits.double().norm())
        print('video %d: score_videos vs score: relative error %.3e' % (v, d))
        assert res.starts[off[v]:off[v + 1]].tolist() == one.starts.tolist()
        assert d < 1e-5                               # other batch shapes: what "Scoring a set of videos" promises of a set
    assert res.metrics is not None
    rgb = video.VideoScorer(boxed['model'], frame_batch=4, window_batch=3, side=SIDE)
    ref = rgb.score_videos([boxed['crops'], boxed['crops2']])
    assert torch.equal(res.window_logits, ref.window_logits)                     # the same plan on the crops: the same bits


def test_explain_nv12_is_explain_on_crops(boxed):
    from istvt_amd import video
    ref = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE).explain(boxed['crops'])
    ex = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE, pixel_format='nv12').explain(boxed['nv'], boxes=boxed['boxes'])
    assert float(ref.frame_s.abs().max()) > 0
    for name in ('frame_s', 'frame_t', 'frame_weight', 'frame_logit', 'count'):
        assert torch.equal(getattr(ex, name), getattr(ref, name)), name
    assert torch.equal(ex.score.window_logits, ref.score.window_logits)


def test_score_nv12_with_jpeg_quality(boxed):
    from istvt_amd import ops, video
    ref = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE).score(ops.jpeg_roundtrip_u8(boxed['crops'], 40))
    res = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE, pixel_format='nv12', jpeg_quality=40).score(
        boxed['nv'], boxes=boxed['boxes'])
    assert torch.equal(res.window_logits, ref.window_logits)
    plain = video.VideoScorer(boxed['model'], frame_batch=4, side=SIDE).score(boxed['crops'])
    assert not torch.equal(res.window_logits, plain.window_logits)


# ---- every option through every entry -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_model(pkg):
    """the `small` model of tests/test_video_set_gpu.py: depth 2, T = 4, 96 x 96 (grid 6), float32, running statistics moved by
    one training forward, left in TRAIN mode"""
    from oracle import istvt_ref as R
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    T, depth = 4, 2
    grid = R.stem_out_side(SIDE)
    shapes = {'xcep.model.' + k: v for k, v in R.stem_param_shapes().items()}
    shapes.update({'vit.' + k: v for k, v in R.dsttr_param_shapes(T, grid, depth=depth).items()})
    model = XceptionVidTr(num_frames=T, grid=grid, depth=depth)
    sd = model.state_dict()
    sd.update(R.random_params(shapes, seed=0))
    model.load_state_dict(sd)
    model = model.cuda().train()
    with torch.no_grad():
        model(torch.randn((2, T, 3, SIDE, SIDE), generator=torch.Generator().manual_seed(1)).cuda())
    return model


def test_nv12_jpeg_boxes_through_every_entry(small_model):
    """NV12 frames, boxes and JPEG recompression at once, through score_videos, score, push / flush and explain, on a bank of 8
    slots: the bits of the plain scorer on ops.jpeg_roundtrip_u8(ops.crop_resize_nv12(...)) made beforehand.  The set's plan
    has a frame batch made of two videos' pieces and one whose slots are scattered; the 9-frame video wraps the ring."""
    from istvt_amd import ops, video
    counts, sizes = [5, 9, 6], [(120, 160), (130, 110), (120, 160)]
    plan = video.SetPlan(counts, 4, 3, True, 4, 2, 8)
    fsteps = [st for st in plan.steps if st.kind == 'frames']
    assert any(len(plan.pieces(st.first, st.count)) > 1 for st in fsteps)
    assert any(st.slots != tuple(range(st.slots[0], st.slots[0] + st.count)) for st in fsteps)
    g = torch.Generator().manual_seed(31)
    nvs, boxes, crops = [], [], []
    for i, (n, (Hs, Ws)) in enumerate(zip(counts, sizes)):
        nv = _nv12(n, Hs, Ws, 40 + i)
        h = torch.randint(40, Hs + 1, (n,), generator=g)
        w = torch.randint(40, Ws + 1, (n,), generator=g)
        y0 = torch.minimum((torch.rand(n, generator=g) * (Hs - h + 1).float()).long(), Hs - h)
        x0 = torch.minimum((torch.rand(n, generator=g) * (Ws - w + 1).float()).long(), Ws - w)
        b = torch.stack([y0, x0, h, w], dim=1).to(torch.int32)
        crops.append(ops.jpeg_roundtrip_u8(ops.crop_resize_nv12(nv.cuda(), b, SIDE, 'bt709'), 40))
        nvs.append(nv if i == 1 else nv.cuda())                                  # the 9-frame video stays on the host
        boxes.append(b)
    kw = dict(stride=3, frame_batch=4, window_batch=2, capacity=8)
    scorer = video.VideoScorer(small_model, side=SIDE, jpeg_quality=40, pixel_format='nv12', **kw)
    plain = video.VideoScorer(small_model, **kw)
    res, ref = scorer.score_videos(nvs, boxes=boxes), plain.score_videos(crops)
    assert torch.isfinite(ref.window_logits).all() and ref.window_logits.shape[0] == len(plan.starts)
    for i in range(6):
        assert torch.equal(res[i], ref[i]), video.VideoSetScore._fields[i]
    nv, b, c = nvs[1], boxes[1], crops[1]
    assert torch.equal(scorer.score(nv, boxes=b).window_logits, plain.score(c).window_logits)

    def stream(s, frames, table):
        outs = []
        for lo in range(0, 9, 2):
            outs.append(s.push(frames[lo:lo + 2], boxes=None if table is None else table[lo:lo + 2].contiguous()))
        outs.append(s.flush())
        return torch.cat([l for l, _ in outs]), torch.cat([st for _, st in outs]).tolist()
    got, want = stream(scorer, nv, b), stream(plain, c, None)
    assert want[1] == video.window_starts(9, 4, 3, True) and got[1] == want[1]
    assert torch.equal(got[0], want[0])
    ex, exr = scorer.explain(nv, boxes=b), plain.explain(c)
    assert float(exr.frame_s.abs().max()) > 0
    for name in ('frame_s', 'frame_t', 'frame_weight'):
        assert torch.equal(getattr(ex, name), getattr(exr, name)), name
