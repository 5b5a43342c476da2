"""The fused criterion on a real MI355X: istvt_bce_logits / istvt_bce_logits_bwd against the float64
restatement loss.bce_logits_ref and against torch's own CUDA criterion, the run-to-run bits, autograd, the meter, capture in a
torch.cuda.graph, and one training step of the model.

Tolerance: the project's float32 kernel tolerance against a float64 restatement, 2e-5 relative (tests/gpu_checks.py TOL),
norm-wise for vectors; every count is exact."""
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 2e-5
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099]
KINDS = [torch.float32, torch.int64, torch.int32, torch.uint8, torch.bool]
EXTREME = [0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4]
COUNTS = ('seen', 'correct', 'tp', 'tn', 'fp', 'fn')


@pytest.fixture(scope='module')
def M():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import loss, ops

    class Mods:
        pass
    m = Mods()
    m.loss, m.ops = loss, ops
    return m


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _inputs(n, seed, stride=1):
    g = torch.Generator().manual_seed(seed)
    zbuf = (torch.randn(n * stride, generator=g) * 3).cuda()
    y = (torch.rand(n, generator=g) > 0.4).float().cuda()
    w = (torch.rand(n, generator=g) + 0.25).cuda()
    return zbuf[::stride], y, w


def _meter_words(t):
    t = t.cpu()
    return t[:2].view(torch.float64).tolist(), t[2:].tolist()


def _new_meter():
    return torch.zeros(10, dtype=torch.int64, device='cuda')


@pytest.mark.parametrize('n', SIZES)
def test_kernel_against_float64_restatement(M, n):
    """every target kind, stride 1 and 2, with and without per-sample weights, pos_weight 3, label smoothing 0.1, the three
    reductions: losses, reduced loss and gradient to 2e-5, counts exact, the meter's loss sum = the fp64 sum of the kernel's
    own per-sample losses"""
    worst = 0.0
    for stride in (1, 2):
        z, y, w = _inputs(n, 100 + n, stride)
        assert n == 1 or z.stride(0) == stride
        for use_w in (False, True):
            for reduction in ('mean', 'sum', 'none'):
                ref = M.loss.bce_logits_ref(z, y, w if use_w else None, 3.0, 0.1, reduction)
                for kind in KINDS:
                    meter = _new_meter()
                    loss, reduced, d = M.ops.bce_logits(z, y.to(kind), w if use_w else None, 3.0, 0.1, reduction, 0.0,
                                                        want_loss=True, want_reduced=True, want_grad=True, meter=meter)
                    errs = (relerr(loss, ref['loss']), relerr(reduced, ref['reduced']), relerr(d, ref['grad']))
                    worst = max(worst, *errs)
                    assert max(errs) <= TOL, (stride, use_w, reduction, kind, errs)
                    (loss_sum, batch_sum), words = _meter_words(meter)
                    assert words[:6] == [ref['counts'][k] for k in COUNTS] and words[6:] == [1, 0]
                    own = float(loss.double().sum())
                    assert abs(loss_sum - own) <= 1e-12 * abs(own)
                    assert batch_sum == float(reduced)               # the fp32 value returned, added to a zero block: exact
    print('n=%d worst relative error %.3e' % (n, worst))


@pytest.mark.parametrize('n', SIZES)
def test_kernel_against_torch_cuda_criterion(M, n):
    z, y, w = _inputs(n, 200 + n)
    for use_w, p, eps in ((False, 1.0, 0.0), (True, 3.0, 0.1)):
        for reduction in ('mean', 'sum'):
            zt = z.clone().requires_grad_()
            t = F.binary_cross_entropy_with_logits(zt, y * (1 - eps) + eps / 2, weight=w if use_w else None, reduction=reduction,
                                                   pos_weight=torch.tensor(p, device='cuda'))
            t.backward()
            _, reduced, d = M.ops.bce_logits(z, y, w if use_w else None, p, eps, reduction)
            errs = (relerr(reduced, t), relerr(d, zt.grad))
            assert max(errs) <= TOL, (use_w, p, eps, reduction, errs)


def test_extreme_logits(M):
    """0, +-1e-3, +-20, +-100, +-1e4 against both labels: everything finite, |z| of loss on the wrong side, gradient +-w (x p)"""
    z = torch.tensor(EXTREME * 2).cuda()
    y = torch.cat([torch.zeros(9), torch.ones(9)]).cuda()
    w = torch.linspace(0.5, 2.0, 18).cuda()
    p = 3.0
    for eps in (0.0, 0.1):
        ref = M.loss.bce_logits_ref(z, y, w, p, eps, 'sum')
        loss, reduced, d = M.ops.bce_logits(z, y, w, p, eps, 'sum', want_loss=True)
        assert torch.isfinite(loss).all() and torch.isfinite(d).all() and torch.isfinite(reduced).all()
        assert relerr(loss, ref['loss']) <= TOL and relerr(d, ref['grad']) <= TOL and relerr(reduced, ref['reduced']) <= TOL
    # eps = 0, elementwise: indices 5 / 7 are z = 100 / 1e4 with y = 0; 9 + 6 / 9 + 8 are z = -100 / -1e4 with y = 1
    loss, _, d = M.ops.bce_logits(z, y, w, p, 0.0, 'sum', want_loss=True)
    loss, d, wc = loss.double().cpu().tolist(), d.double().cpu().tolist(), w.double().cpu().tolist()
    for i, zi in ((5, 100.0), (7, 1e4)):
        assert abs(float(loss[i]) - wc[i] * zi) <= TOL * wc[i] * zi and abs(float(d[i]) - wc[i]) <= TOL * wc[i]
    for i, zi in ((15, 100.0), (17, 1e4)):
        assert abs(float(loss[i]) - p * wc[i] * zi) <= TOL * p * wc[i] * zi and abs(float(d[i]) + p * wc[i]) <= TOL * p * wc[i]
    # the right side of a huge logit costs (almost) nothing and pulls (almost) nowhere
    for i in (6, 8, 9 + 5, 9 + 7):
        assert 0.0 <= float(loss[i]) <= 1e-30 and abs(float(d[i])) <= 1e-30
    # z = -20, y = 0 and z = 20, y = 1: exp(-20), kept in fp32 (the regrouped formula does not cancel it away)
    for i, scale in ((4, 1.0), (9 + 3, p)):
        want = scale * float(wc[i]) * 2.061153622e-9
        assert abs(float(loss[i]) - want) <= 1e-5 * want and abs(abs(float(d[i])) - want) <= 1e-5 * want


def test_nan_logit_follows_the_comparison(M):
    z = torch.tensor([float('nan'), float('nan'), 2.0, -2.0]).cuda()
    y = torch.tensor([1, 0, 1, 0]).cuda()
    meter = _new_meter()
    _, reduced, _ = M.ops.bce_logits(z, y, meter=meter)
    (loss_sum, _), words = _meter_words(meter)
    assert words[:6] == [4, 3, 1, 2, 0, 1]                  # NaN > 0 is false: predicted negative, right for y = 0
    assert loss_sum != loss_sum and bool(torch.isnan(reduced).all())


@pytest.mark.parametrize('n', [65, 4099])
def test_two_calls_give_the_same_bits(M, n):
    z, y, w = _inputs(n, 300 + n, 2)
    for reduction in ('mean', 'none'):
        got = []
        for _ in range(2):
            meter = _new_meter()
            out = M.ops.bce_logits(z, y, w, 3.0, 0.1, reduction, want_loss=True, meter=meter)
            got.append(list(out) + [meter, M.ops.bce_logits_bwd(out[2], out[1] if reduction == 'mean' else out[0])])
        for a, b in zip(*got):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_autograd_matches_torch_criterion(M):
    n = 77
    z, y, w = _inputs(n, 400, 2)
    gvec = torch.linspace(-1, 2, n).cuda()
    for kw_mine, kw_t in ((dict(), dict()), (dict(weight=w, pos_weight=3.0), dict(weight=w, pos_weight=torch.tensor(3.0).cuda()))):
        for reduction in ('mean', 'sum', 'none'):
            for scale in (None, 128.0):
                grads = []
                for crit in (M.loss.BCEWithLogitsLoss(reduction=reduction, **kw_mine),
                             torch.nn.BCEWithLogitsLoss(reduction=reduction, **kw_t)):
                    base = z.clone().requires_grad_()               # the same leaf logits
                    out = crit(base, y)
                    assert out.shape == ((n,) if reduction == 'none' else ())
                    if scale is not None:
                        out = out * scale
                    if reduction == 'none':
                        out.backward(gvec)                          # a vector gradient
                    else:
                        out.backward()                              # autograd's ones, on the device
                    grads.append((out.detach(), base.grad))
                assert relerr(grads[0][0], grads[1][0]) <= TOL and relerr(grads[0][1], grads[1][1]) <= TOL, (reduction, scale)
    # a column of a (B, 2) tensor: no copy, the gradient lands in the column
    base = torch.randn(n, 2, device='cuda', requires_grad=True)
    M.loss.BCEWithLogitsLoss()(base[:, 1], y.long()).backward()
    ref = M.loss.bce_logits_ref(base[:, 1], y)
    assert relerr(base.grad[:, 1], ref['grad']) <= TOL and not base.grad[:, 0].any()


def test_no_grad_feeds_the_meter_and_writes_no_gradient(M, monkeypatch):
    z, y, _ = _inputs(40, 500)
    meter = M.loss.TrainMeter('cuda')
    crit = M.loss.BCEWithLogitsLoss(meter=meter)
    seen = []
    real = M.ops.bce_logits

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw['want_grad'], out[2]))
        return out
    monkeypatch.setattr(M.ops, 'bce_logits', spy)
    with torch.no_grad():
        out = crit(z.requires_grad_(), y)
    assert seen == [(False, None)] and not out.requires_grad and out.grad_fn is None
    out2 = crit(z, y)                                               # gradients on: the same value, and a gradient buffer
    assert seen[1][0] is True and seen[1][1] is not None and torch.equal(out, out2.detach())
    assert meter.snapshot().counts['calls'] == 2 and meter.snapshot().counts['seen'] == 80


def test_meter_accumulates_resets_and_reads_without_draining(M):
    meter = M.loss.TrainMeter('cuda')
    crit = M.loss.BCEWithLogitsLoss(pos_weight=2.0, meter=meter)
    assert tuple(meter.tensor.shape) == (10,) and meter.tensor.dtype == torch.int64
    host = {k: 0 for k in COUNTS}
    loss_sum, batch_sum, total = 0.0, 0.0, 0
    for i, n in enumerate((32, 7, 300)):
        z, y, _ = _inputs(n, 600 + i)
        out = crit(z, y)
        ref = M.loss.bce_logits_ref(z, y, None, 2.0)
        for k in COUNTS:
            host[k] += ref['counts'][k]
        loss_sum += float(ref['loss'].sum())
        batch_sum += out.item()                                     # train_loss += loss.item()
        total += n
    snap = meter.snapshot()
    assert snap.counts == dict(host, calls=3)
    assert snap.batch_loss_sum == batch_sum                         # the same fp32 values added in the same order in fp64
    assert abs(snap.loss_mean - loss_sum / total) <= TOL * loss_sum / total
    assert snap.accuracy == host['correct'] / total
    assert snap.apcer == host['fn'] / (host['tp'] + host['fn']) and snap.bpcer == host['fp'] / (host['tn'] + host['fp'])
    assert snap.acer == (snap.apcer + snap.bpcer) / 2
    # a snapshot keeps the values of ITS point of the stream: a long launch and another call enqueued behind it change nothing
    big = torch.randn(4096, 4096, device='cuda')
    early = meter.snapshot()
    for _ in range(10):
        big = big @ big * 1e-2
    z, y, _ = _inputs(5, 700)
    crit(z, y)
    late = meter.snapshot()
    assert early.counts == dict(host, calls=3) and early.batch_loss_sum == batch_sum
    assert late.counts['calls'] == 4 and late.counts['seen'] == total + 5
    meter.reset()
    zero = meter.snapshot()
    assert zero.counts == {k: 0 for k in COUNTS + ('calls',)} and zero.loss_sum == 0.0 and zero.batch_loss_sum == 0.0
    assert not meter.tensor.any()


def _dot_edges(path):
    text = open(path).read()
    return re.findall(r'"?([\w.]+)"?\s*->\s*"?([\w.]+)"?', text), text


def test_capture_in_one_graph(M, tmp_path):
    """forward + backward of the criterion captured in one torch.cuda.graph and replayed with new logits: the eager call's
    bits, `calls` advanced once per replay, and a graph whose nodes form one chain"""
    n = 96
    meter = M.loss.TrainMeter('cuda')
    crit = M.loss.BCEWithLogitsLoss(pos_weight=3.0, label_smoothing=0.1, meter=meter)
    batches = [_inputs(n, 800 + i) for i in range(3)]
    static_z = batches[0][0].clone().requires_grad_()
    y = batches[0][1].long()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        torch.autograd.grad(crit(static_z, y), static_z)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    meter.reset()
    graph = torch.cuda.CUDAGraph(keep_graph=True)                   # the captured graph stays, for the dump below
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        static_loss = crit(static_z, y)
        static_grad, = torch.autograd.grad(static_loss, static_z)
    graph.instantiate()
    assert meter.snapshot().counts['calls'] == 0                    # captured, not run
    for i, (z, _, _) in enumerate(batches[1:]):
        with torch.no_grad():
            static_z.copy_(z)
        graph.replay()
        got = (static_loss.clone(), static_grad.clone())
        eager_meter = M.loss.TrainMeter('cuda')
        leaf = z.clone().requires_grad_()
        loss = M.loss.BCEWithLogitsLoss(pos_weight=3.0, label_smoothing=0.1, meter=eager_meter)(leaf, y)
        grad, = torch.autograd.grad(loss, leaf)
        assert torch.equal(got[0].view(torch.int32), loss.detach().view(torch.int32))
        assert torch.equal(got[1].view(torch.int32), grad.view(torch.int32))
        assert meter.snapshot().counts['calls'] == i + 1
    assert meter.snapshot().counts['seen'] == 2 * n
    dot = str(tmp_path / 'criterion_graph.dot')
    graph.debug_dump(dot)
    edges, text = _dot_edges(dot)
    nodes = {a for e in edges for a in e}
    assert len(nodes) >= 2, text                                    # at least the two kernels of this pull request
    assert len(edges) == len(nodes) - 1, text
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges), text   # no fork, no join


# ---- the model: the smallest full-step configuration of tests/test_model_gpu.py (float32, B = 2, T = 4, 96^2, depth 2) ----
def _model_case(seed=0):
    from oracle import istvt_ref as R
    B, T, side, depth = 2, 4, 96, 2
    grid = R.stem_out_side(side)
    shapes = {'xcep.model.' + k: v for k, v in R.stem_param_shapes().items()}
    shapes.update({'vit.' + k: v for k, v in R.dsttr_param_shapes(T, grid, depth=depth).items()})
    p = R.random_params(shapes, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((B, T, 3, side, side), generator=g).cuda()
    labels = torch.tensor([1.0, 0.0]).cuda()
    return p, x, labels, T, grid, depth


def _trainer(p, T, grid, depth, graphs=False):
    from istvt_amd import parallel
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=T, grid=grid, depth=depth, compute_dtype=torch.float32)
    sd = model.state_dict()
    sd.update(p)
    model.load_state_dict(sd)
    model = model.cuda().train()
    live = [q for _, q in parallel.live_named_parameters(model)]
    bucket = parallel.GradBucket(live, fuse_accumulate=True, flatten_params=True)
    opt = parallel.FusedSGD(bucket, lr=0.05, momentum=0.9, zero_grad=True)
    if graphs:
        model.enable_step_graphs(True)
    return model, bucket, opt


def test_model_step_with_fused_criterion_matches_torch_criterion(M):
    """one SGD step from identical weights with the fused and with the torch criterion: the same logits in bits (the forward
    is the same), the flat gradient bucket within 2e-5 relative L2 (the backward is linear in the logit gradient, which
    differs by fp32 rounding)"""
    p, x, labels, T, grid, depth = _model_case()
    runs = []
    for crit in (torch.nn.BCEWithLogitsLoss(), M.loss.BCEWithLogitsLoss(meter=M.loss.TrainMeter('cuda'))):
        model, bucket, opt = _trainer(p, T, grid, depth)
        opt.zero_grad()
        logits = model(x)
        loss = crit(logits.view(-1), labels)
        loss.backward()
        grads = bucket.flat.clone()
        opt.step()
        torch.cuda.synchronize()
        runs.append((logits.detach().clone(), loss.item(), grads, bucket.flat_params.detach().clone()))
    (la, lossa, ga, pa), (lb, lossb, gb, pb) = runs
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    err = relerr(gb, ga)
    print('fused against torch criterion: loss %.9g vs %.9g, flat gradient relative L2 %.3e, parameters after the step %.3e'
          % (lossb, lossa, err, relerr(pb, pa)))
    assert float(ga.norm()) > 0 and abs(lossb - lossa) <= TOL * abs(lossa)
    assert err <= TOL, err


def test_step_graphs_with_fused_criterion_give_the_launch_by_launch_bits(M):
    p, x, labels, T, grid, depth = _model_case()
    seqs = []
    for graphs in (False, True):
        meter = M.loss.TrainMeter('cuda')
        crit = M.loss.BCEWithLogitsLoss(meter=meter)
        model, bucket, opt = _trainer(p, T, grid, depth, graphs)
        seq = []
        for _ in range(3):
            opt.zero_grad()
            loss = crit(model(x).view(-1), labels)
            loss.backward()
            opt.step()
            seq.append(loss.detach().clone())
        torch.cuda.synchronize()
        if graphs:
            st = model._step_graphs.stats
            assert st['captures'] == 1 and st['replays'] == 1 and st['eager'] == 2, st
        seqs.append(([v.item() for v in seq], torch.stack(seq).view(torch.int32), meter.snapshot()))
    assert torch.equal(seqs[0][1], seqs[1][1]), (seqs[0][0], seqs[1][0])
    assert seqs[0][0][0] != seqs[0][0][2]                            # the steps did change the loss
    assert seqs[0][2].counts == seqs[1][2].counts and seqs[0][2].counts['calls'] == 3
    assert seqs[0][2].batch_loss_sum == seqs[1][2].batch_loss_sum == sum(seqs[0][0])
