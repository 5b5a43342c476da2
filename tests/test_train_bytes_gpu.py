"""Training from bytes (DESIGN.md "Training from bytes") on a real MI355X: the three kernels that read a view of decoded
frames against their float twins on the float32 tensor the HOST makes of the same view (clips.to_float, then uploaded --
the device's division differs in the last bit), bit for bit, and the model fed uint8 clips with views against the model fed
that float tensor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
DTYPES = [torch.float32, torch.bfloat16]
IDS = ['f32', 'bf16']


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _video(n, h, w, seed):
    """uint8 (n, h, w, 3) in which every channel takes every byte value (the first 256 pixels of frame 0, permuted per
    channel) and the rest is random (as test_video_gpu._video)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    flat = v.view(-1, 3)
    for c in range(3):
        flat[:256, c] = torch.randperm(256, generator=g).to(torch.uint8)
    assert all(len(torch.unique(v[..., c])) == 256 for c in range(3))
    return v


def _cases(S, n=3, seed=0):
    """(name, source uint8 (n, Hs, Ws, 3), per-frame view or None): the identity view of crop-sized frames, and per-frame
    views (corners, flips) of an odd-sized larger source"""
    Hs, Ws = S + 13, S + 21
    view = torch.tensor([[0, 0, 1], [Hs - S, Ws - S, 0], [5, 7, 1], [Hs - S, 0, 1], [3, Ws - S, 0]][:n], dtype=torch.int32)
    return [('identity', _video(n, S, S, S + seed), None), ('views', _video(n, Hs, Ws, S + seed + 1), view)]


def _norm_dev(norm):
    return torch.tensor(norm[0]).cuda(), torch.tensor(norm[1]).cuda()


# ---- kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('side', [96, 139, 224, 300])
def test_conv1_fwd_from_a_view_bit_identical(pkg, side, dtype):
    from istvt_amd import clips, ops
    norm = IMAGENET if side % 2 else HALF
    m, s = _norm_dev(norm)
    w = torch.randn((32, 3, 3, 3), generator=torch.Generator().manual_seed(side + 1)).cuda()
    Ho = (side - 3) // 2 + 1
    for name, u8, view in _cases(side):
        ref = ops.conv1_fwd(clips.to_float(u8, norm[0], norm[1], view, side).cuda(), w, dtype)
        assert torch.isfinite(ref.float()).all() and float(ref.float().abs().max()) > 0
        dev = u8.cuda()
        out = ops.conv1_fwd_u8_view(dev, view, side, m, s, w, dtype)
        assert torch.equal(out, ref), name
        # a slice that starts in the middle of the allocation (frame 1 on: an odd byte offset at odd sizes)
        out1 = ops.conv1_fwd_u8_view(dev[1:], None if view is None else view[1:].contiguous(), side, m, s, w, dtype)
        assert torch.equal(out1, ref[Ho * Ho:]), name
    with pytest.raises(ValueError):
        ops.conv1_fwd_u8_view(dev, None, side, m, s, w, dtype)                 # a larger source needs a view
    bad = view.clone()
    bad[0, 0] = u8.shape[1] - side + 1
    with pytest.raises(ValueError):
        ops.conv1_fwd_u8_view(dev, bad, side, m, s, w, dtype)
    with pytest.raises(TypeError):
        ops.conv1_fwd_u8_view(dev.float(), view, side, m, s, w, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('side', [33, 96, 224, 257])
def test_conv1_wgrad_from_bytes_bit_identical(pkg, side, dtype):
    import gpu_checks
    from istvt_amd import clips, ops
    norm = IMAGENET if side % 2 else HALF
    m, s = _norm_dev(norm)
    Ho = (side - 3) // 2 + 1
    for name, u8, view in _cases(side):
        n = u8.shape[0]
        du1 = torch.randn((n * Ho * Ho, 32), generator=torch.Generator().manual_seed(side)).cuda().to(dtype)
        x = clips.to_float(u8, norm[0], norm[1], view, side)
        ref = ops.conv1_wgrad(du1, x.cuda())
        dev = u8.cuda()
        out = ops.conv1_wgrad_u8(du1, dev, view, side, m, s)
        assert float(ref.abs().max()) > 0
        assert torch.equal(out, ref), name
        assert float(out[:, 27:].abs().max()) == 0.0
        out1 = ops.conv1_wgrad_u8(du1[Ho * Ho:], dev[1:], None if view is None else view[1:].contiguous(), side, m, s)
        assert torch.equal(out1, ops.conv1_wgrad(du1[Ho * Ho:], x[1:].cuda())), name
        # float64 conv2d backward on bf16-rounded patches and du1 (what the MFMA is fed), as gpu_checks.conv_dense_check
        xq = x.to(torch.bfloat16).double()
        wd = torch.zeros((32, 3, 3, 3), dtype=torch.float64, requires_grad=True)
        g = du1.cpu().to(torch.bfloat16).double().view(n, Ho, Ho, 32).permute(0, 3, 1, 2)
        torch.nn.functional.conv2d(xq, wd, None, 2, 0).backward(g)
        e = gpu_checks.relerr(out[:, :27].reshape(32, 3, 3, 3).cpu(), wd.grad)
        print('conv1_wgrad_u8 S=%d %s %s: relerr vs float64 = %.3e (tolerance %.1e)' % (side, name, dtype, e, gpu_checks.TOL[dtype]))
        assert e <= gpu_checks.TOL[dtype]


def test_conv1_wgrad_from_bytes_shape_limit(pkg):
    """Ho > 128 (the native 300^2 geometry) is the float kernel's limit too: the shape error, no launch"""
    from istvt_amd import ops
    m, s = _norm_dev(HALF)
    u8 = _video(1, 300, 300, 1).cuda()
    du1 = torch.zeros((149 * 149, 32), dtype=torch.bfloat16, device='cuda')
    with pytest.raises(RuntimeError, match='invalid shape'):
        ops.conv1_wgrad_u8(du1, u8, None, 300, m, s)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('side', [96, 300])
def test_im2col_from_bytes_bit_identical(pkg, side, dtype):
    from istvt_amd import clips, ops
    norm = IMAGENET if side == 300 else HALF
    m, s = _norm_dev(norm)
    Ho = (side - 3) // 2 + 1
    for name, u8, view in _cases(side):
        ref = ops.im2col_conv1(clips.to_float(u8, norm[0], norm[1], view, side).cuda(), dtype)
        dev = u8.cuda()
        out = ops.im2col_conv1_u8(dev, view, side, m, s, dtype)
        assert torch.equal(out, ref), name
        assert float(out[:, 27:].float().abs().max()) == 0.0
        out1 = ops.im2col_conv1_u8(dev[1:], None if view is None else view[1:].contiguous(), side, m, s, dtype)
        assert torch.equal(out1, ref[Ho * Ho:]), name


def test_independent_of_the_surroundings(pkg):
    """the same crop embedded in two sources that differ in every byte outside it: the same bits from all three kernels,
    and a second run of each gives the same bits"""
    from istvt_amd import ops
    S, Hs, Ws, n = 97, 120, 131, 3
    m, s = _norm_dev(IMAGENET)
    w = torch.randn((32, 3, 3, 3), generator=torch.Generator().manual_seed(2)).cuda()
    view = torch.tensor([[11, 17, 1], [0, 34, 0], [23, 0, 1]], dtype=torch.int32)
    a = _video(n, Hs, Ws, 5)
    b = a ^ 0xFF                                               # differs in every byte ...
    for f in range(n):
        y0, x0 = int(view[f, 0]), int(view[f, 1])
        b[f, y0:y0 + S, x0:x0 + S] = a[f, y0:y0 + S, x0:x0 + S]    # ... outside the crop
    Ho = (S - 3) // 2 + 1
    du1 = torch.randn((n * Ho * Ho, 32), generator=torch.Generator().manual_seed(3)).cuda().to(torch.bfloat16)
    res = []
    for src in (a, b, a):
        dev = src.cuda()
        res.append((ops.conv1_fwd_u8_view(dev, view, S, m, s, w, torch.bfloat16), ops.conv1_wgrad_u8(du1, dev, view, S, m, s),
                    ops.im2col_conv1_u8(dev, view, S, m, s, torch.float32)))
    for k in range(3):
        assert torch.equal(res[0][k], res[1][k]) and torch.equal(res[0][k], res[2][k]), k


# ---- the model -------------------------------------------------------------------------------------------------------
def _train_pair(dtype, T, grid, depth, graphs=False):
    from istvt_amd import parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    made = []
    for _ in range(2):
        torch.manual_seed(5)
        model = XceptionVidTr(num_frames=T, grid=grid, depth=depth, compute_dtype=dtype).cuda().train()
        live = [p for _, p in parallel.live_named_parameters(model)]
        bucket = parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
        opt = parallel.FusedSGD(bucket, lr=1e-2, momentum=0.9, zero_grad=True)
        made.append((model, bucket, opt))
    if graphs:
        made[0][0].enable_step_graphs(True)
    return made


def _run_steps(made, u8s, views, S, ys, steps, norm=None):
    """made[0] gets the bytes and the views, made[1] the float tensor the host makes of them; everything compared"""
    from istvt_amd import clips, video
    mean, std = norm or (video.DEFAULT_MEAN, video.DEFAULT_STD)
    crit = torch.nn.BCEWithLogitsLoss()
    (mb, bb, ob), (mf, bf, of) = made
    if norm is not None:
        mb.set_input_normalisation(mean, std)
    for i in range(steps):
        u8, view, y = u8s[i % len(u8s)], views[i % len(views)], ys[i % len(ys)]
        xf = clips.to_float(u8, mean, std, view, S).cuda()
        xb = u8.cuda()
        # one whole forward + backward per model, one after the other (as the loop would run it), then compared
        ob.zero_grad()
        lb = mb(xb, view=view, crop=S) if view is not None else mb(xb)
        lossb = crit(lb.view(-1), y)
        lossb.backward()
        assert xb.grad is None
        of.zero_grad()
        lf = mf(xf)
        lossf = crit(lf.view(-1), y)
        lossf.backward()
        assert torch.equal(lb, lf), 'logits, step %d' % i
        assert lossb.item() == lossf.item()
        assert float(bf.flat.abs().max()) > 0
        for (name, p), (_, q) in zip(mb.named_parameters(), mf.named_parameters()):
            if q.grad is not None or p.grad is not None:
                assert torch.equal(p.grad, q.grad), 'gradient of %s, step %d' % (name, i)
        ob.step(); of.step()
    torch.cuda.synchronize()
    running = [k for k in mf.state_dict() if 'running' in k]
    stem_bn = [k for k in running if any(('xcep.model.%s.' % b) in k for b in __import__('istvt_amd.stem', fromlist=['x']).bn_names())]
    assert len(stem_bn) == 22                                   # the eleven BatchNorms of the entry flow
    sb, sf = mb.state_dict(), mf.state_dict()
    for k in running:
        assert torch.equal(sb[k], sf[k]), k
    for (name, p), (_, q) in zip(mb.named_parameters(), mf.named_parameters()):
        assert torch.equal(p, q), name
    assert torch.equal(bb.flat_params, bf.flat_params)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_model_trains_from_bytes_bit_identical(pkg, dtype):
    """XceptionVidTr(num_frames=4, grid=6, depth=2), S = 96 from 112 x 120 sources with mixed views, FusedSGD on the fused
    bucket: logits, loss, every parameter gradient, the BatchNorm running buffers and every parameter after 3 steps"""
    B, T, S, Hs, Ws = 3, 4, 96, 112, 120
    made = _train_pair(dtype, T, 6, 2)
    g = torch.Generator().manual_seed(6)
    u8s = [_video(B * T, Hs, Ws, 20 + i).view(B, T, Hs, Ws, 3) for i in range(2)]
    views = [torch.tensor([[0, 0, 0], [16, 24, 1], [7, 13, 1]], dtype=torch.int32),
             torch.tensor([[16, 0, 1], [3, 24, 0], [9, 9, 0]], dtype=torch.int32)]
    ys = [(torch.rand((B,), generator=g) > 0.5).float().cuda() for _ in range(2)]
    _run_steps(made, u8s, views, S, ys, 3, norm=IMAGENET)


def test_model_trains_from_bytes_native_geometry(pkg):
    """S = 300, T = 6, depth 1, B = 1, bf16: Ho = 149 > 128, the weight gradient takes the im2col route; the crop side is
    the model's own (grid 19 -> 300)"""
    B, T, S, Hs, Ws = 1, 6, 300, 317, 331
    made = _train_pair(torch.bfloat16, T, 19, 1)
    u8 = _video(B * T, Hs, Ws, 31).view(B, T, Hs, Ws, 3)
    view = torch.tensor([[17, 30, 1]], dtype=torch.int32)
    y = torch.ones((B,), device='cuda')
    assert made[0][0].crop_side == 300
    from istvt_amd import clips, video
    crit = torch.nn.BCEWithLogitsLoss()
    (mb, bb, ob), (mf, bf, of) = made
    xf = clips.to_float(u8, video.DEFAULT_MEAN, video.DEFAULT_STD, view, S).cuda()
    ob.zero_grad()
    lb = mb(u8.cuda(), view=view)                              # crop: the model's setting
    crit(lb.view(-1), y).backward()
    of.zero_grad()
    lf = mf(xf)
    crit(lf.view(-1), y).backward()
    assert torch.equal(lb, lf)
    assert float(bf.flat.abs().max()) > 0 and torch.equal(bb.flat, bf.flat)
    ob.step(); of.step()
    assert torch.equal(bb.flat_params, bf.flat_params)
    for k, v in mf.state_dict().items():
        if 'running' in k:
            assert torch.equal(mb.state_dict()[k], v), k


def test_model_from_bytes_without_view_and_eval(pkg):
    """crop-sized frames need no view; eval mode under no_grad: bf16 equal, f32 to 1e-5 (the float path keeps im2col + GEMM
    for conv1 there and the byte path follows it, so equal bits are expected -- printed)"""
    from istvt_amd import clips, video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    B, T, S = 2, 4, 96
    u8 = _video(B * T, S, S, 41).view(B, T, S, S, 3)
    xf = clips.to_float(u8, video.DEFAULT_MEAN, video.DEFAULT_STD).cuda()
    for dtype in DTYPES:
        torch.manual_seed(9)
        model = XceptionVidTr(num_frames=T, grid=6, depth=2, compute_dtype=dtype).cuda().eval()
        with torch.no_grad():
            yb, yf = model(u8.cuda()), model(xf)
        same = torch.equal(yb, yf)
        print('eval %s: byte and float logits bit-identical: %s, max |diff| = %.3e' % (dtype, same, float((yb.float() - yf.float()).abs().max())))
        if dtype == torch.bfloat16:
            assert same
        else:
            assert float((yb - yf).abs().max()) <= 1e-5 * max(1.0, float(yf.abs().max()))
        with pytest.raises(ValueError):
            model(torch.zeros((B, T, 112, 120, 3), dtype=torch.uint8, device='cuda'))      # a larger source needs a view
        with pytest.raises(ValueError):
            model(torch.zeros((B, T, 112, 120, 3), dtype=torch.uint8, device='cuda'),
                  view=torch.zeros((B, 3), dtype=torch.int32))                              # grid 6 names no crop side
    # train mode without a view: the same contract
    made = _train_pair(torch.bfloat16, T, 6, 2)
    ys = [torch.tensor([1.0, 0.0], device='cuda')]
    _run_steps(made, [u8], [None], S, ys, 2)


def test_step_graphs_run_bytes_launch_by_launch(pkg):
    """with enable_step_graphs() a uint8 step runs launch by launch, equals the eager result and says why; a float step
    afterwards is still replayed"""
    from istvt_amd import clips, video
    B, T, S, Hs, Ws = 2, 4, 96, 112, 120
    made = _train_pair(torch.bfloat16, T, 6, 2, graphs=True)
    (mg, bg, og), (me, be, oe) = made                          # graphs on / launch by launch
    crit = torch.nn.BCEWithLogitsLoss()
    gen = torch.Generator().manual_seed(8)
    xs = torch.randn((B, T, 3, S, S), generator=gen).cuda()
    u8 = _video(B * T, Hs, Ws, 51).view(B, T, Hs, Ws, 3).cuda()
    view = clips.random_views(B, Hs, Ws, S, gen)
    y = torch.tensor([1.0, 0.0], device='cuda')
    g = mg._step_graphs

    def step(kind):
        outs = []
        for m, b, o in made:
            o.zero_grad()
            logits = m(xs) if kind == 'float' else m(u8, view=view, crop=S)
            crit(logits.view(-1), y).backward()
            o.step()
            outs.append((logits.detach().clone(), b.flat_params.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), kind
    for _ in range(3):
        step('float')                                          # two warm-up calls, one capture + replay
    assert g.stats['captures'] == 1 and g.stats['replays'] == 1
    n_eager = g.stats['eager']
    step('bytes')
    assert g.stats['eager'] == n_eager + 1 and g.stats['captures'] == 1 and g.stats['replays'] == 1
    assert g.last_reason == 'uint8 input: the byte path is not captured'
    step('float')
    assert g.stats['replays'] == 2 and g.stats['captures'] == 1
    step('bytes')
    step('float')
    assert g.stats['replays'] == 3 and g.stats['captures'] == 1
