"""Fused optimizers on a real MI355X: parameter groups, the gradient-norm kernel, clipping, the
non-finite skip and multi-group checkpoints, against torch.optim.SGD / AdamW with the same groups.

The bound against torch is the one tests/test_model_gpu.py::test_fused_optimizers_match_torch already holds the fused
optimizers to (relerr < 2e-6).  On these inputs torch's own float32 run stays within 8.1e-8 of its float64 run, per
parameter and step, with and without clipping (measured on the CPU), so one more rounding -- the clip coefficient folded
into the gradient scale -- has an order of magnitude of room."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(37, 5), (1001,), (8, 3, 3, 3), (3,), (1,), (4097,)]      # segment starts 0, 185, 1186, 1402, 1405, 1406: every residue mod 4
N = 5503                                                            # 3 elements behind the last whole 16-byte quad
TOL = 2e-6
STEPS = 4
KW = {'sgd': dict(lr=0.02, momentum=0.9, weight_decay=1e-2, nesterov=True),
      'adamw': dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)}


@pytest.fixture(scope='module')
def parallel():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import parallel
    return parallel


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def inputs(device='cuda'):
    """initial values and STEPS gradient sets, alternately large (x 3) and small (x 0.01)"""
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(s, generator=gen) for s in SHAPES]
    grads = [[(torch.randn(s, generator=gen) * (3.0 if step % 2 == 0 else 0.01)).to(device) for s in SHAPES]
             for step in range(STEPS)]
    return init, grads


def three_groups(ps):
    """{0, 2, 4}: lr 0.05 without decay; {1, 3}: lr 0.01; parameter 5: named nowhere, the defaults"""
    return [{'params': [ps[0], ps[2], ps[4]], 'lr': 0.05, 'weight_decay': 0.0}, {'params': [ps[1], ps[3]], 'lr': 0.01}]


def torch_optimizer(kind, ps, groups=three_groups):
    spec = groups(ps)
    named = set(id(q) for g in spec for q in g['params'])
    rest = [q for q in ps if id(q) not in named]
    spec = spec + ([{'params': rest}] if rest else [])
    return (torch.optim.SGD if kind == 'sgd' else torch.optim.AdamW)(spec, **KW[kind])


def fused_optimizer(parallel, kind, init, groups=three_groups, **extra):
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    bucket = parallel.GradBucket(ps, flatten_params=True)
    cls = parallel.FusedSGD if kind == 'sgd' else parallel.FusedAdamW
    opt = cls(bucket, param_groups=None if groups is None else groups(ps), **KW[kind], **extra)
    return ps, bucket, opt


def state_buffers(opt):
    return [getattr(opt, name) for name in opt._state_names]


def run_against_torch(parallel, kind, steps=STEPS, clip=None, bad=None, grad_mult=1.0, **extra):
    """the loop of the issue: `steps` steps, every group's lr x 0.7 after each, torch (with clip_grad_norm_ in front when
    `clip`) against the fused optimizer, compared after every step.  bad = (step, value): that step's gradient of the fused
    side gets one `value` (inf / NaN) and torch does not step on that iteration.  Returns (params, bucket, optimizer, norms)."""
    init, grads = inputs()
    ref_p = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    ref = torch_optimizer(kind, ref_p)
    ps, bucket, opt = fused_optimizer(parallel, kind, init, max_grad_norm=clip, **extra)
    assert len(opt.param_groups) == 3 and [len(g['params']) for g in opt.param_groups] == [3, 2, 1]
    norms = []
    for step in range(steps):
        ref.zero_grad()
        opt.zero_grad()
        for p_, q_, gv in zip(ref_p, ps, grads[step]):
            p_.grad = gv.clone()
            q_.grad.add_(gv * grad_mult)                # accumulate into the bucket view, as the kernels do
        skipped = bad is not None and bad[0] == step
        if skipped:
            ps[1].grad.view(-1)[500] = bad[1]
            before = [q_.detach().clone() for q_ in ps] + [t.clone() for t in state_buffers(opt)]
        if grad_mult != 1.0:
            bucket.grad_scale = 1.0 / grad_mult
        ref_norm = torch.nn.utils.clip_grad_norm_(ref_p, clip if clip is not None else 1e30)
        if not skipped:
            ref.step()
        opt.step()
        assert bucket.grad_scale == 1.0
        if skipped:
            after = [q_.detach() for q_ in ps] + state_buffers(opt)
            assert all(torch.equal(a, b) for a, b in zip(before, after)), (kind, bad)
        if opt.fused_zero_grad:
            assert float(bucket.flat.abs().max()) == 0.0, (kind, step)
        if opt._info is not None:
            norms.append((float(opt.grad_norm()), float(ref_norm)))
        for i, (p_, q_) in enumerate(zip(ref_p, ps)):
            err = relerr(q_, p_)
            print('%s clip=%s bad=%s step %d parameter %d: relerr %.3g' % (kind, clip, bad, step, i, err))
            assert err < TOL, (kind, clip, bad, step, i, err)
        for g in list(ref.param_groups) + list(opt.param_groups):
            g['lr'] *= 0.7
    return ps, bucket, opt, norms


# ---- 1. groups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fz', [False, True])
@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_three_groups_match_torch_every_step(parallel, kind, fz):
    ps, bucket, opt, _ = run_against_torch(parallel, kind, zero_grad=fz)
    assert opt.hyper is opt.param_groups[0] and abs(opt.hyper['lr'] - 0.05 * 0.7 ** STEPS) < 1e-12
    assert opt.steps == STEPS and opt.applied_steps() == STEPS
    with pytest.raises(RuntimeError):
        opt.grad_norm()                                 # no clipping, no skip: no norm pass ran
    # hyper-parameters the kernels take once must still agree at step()
    opt.param_groups[1]['momentum' if kind == 'sgd' else 'eps'] = 0.123
    with pytest.raises(ValueError, match='same in every param group'):
        opt.step()


def test_schedulers_act_on_every_group(parallel):
    init, _ = inputs()
    _, _, opt = fused_optimizer(parallel, 'sgd', init)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    opt.step()
    sched.step()
    assert [round(g['lr'], 12) for g in opt.param_groups] == [0.025, 0.005, 0.01]


# ---- 2. one group through the grouped entry point == the plain entry point ------------------------------------------------
@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_one_group_through_groups_entry_is_bit_identical(parallel, kind):
    from istvt_amd import _lib, ops
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(N, generator=gen).cuda()
    grads = [torch.randn(N, generator=gen).cuda() for _ in range(3)]
    nstate = 1 if kind == 'sgd' else 2
    plain = [p0.clone()] + [torch.zeros(N, device='cuda') for _ in range(nstate)]
    group = [p0.clone()] + [torch.zeros(N, device='cuda') for _ in range(nstate)]
    seg_end = torch.tensor([N], dtype=torch.int64, device='cuda')
    seg_gid = torch.zeros(1, dtype=torch.int32, device='cuda')
    lr, wd = (ctypes.c_float * 1)(0.05), (ctypes.c_float * 1)(0.01)
    for step, gv in enumerate(grads):
        ga, gb = gv.clone(), gv.clone()
        zero = int(step == 1)                           # the fused zero-grad on one of the steps
        if kind == 'sgd':
            _lib.check(lib.istvt_sgd_momentum(plain[0].data_ptr(), ga.data_ptr(), plain[1].data_ptr(), N, 0.05, 0.9, 0.1, 0.01,
                                              0, int(step == 0), zero, 0.5, ops._stream()), 'plain')
            _lib.check(lib.istvt_sgd_momentum_groups(group[0].data_ptr(), gb.data_ptr(), group[1].data_ptr(), N,
                                                     seg_end.data_ptr(), seg_gid.data_ptr(), 1, lr, wd, 1, 0.9, 0.1, 0,
                                                     int(step == 0), zero, 0.5, None, 0, ops._stream()), 'groups')
        else:
            _lib.check(lib.istvt_adamw(plain[0].data_ptr(), ga.data_ptr(), plain[1].data_ptr(), plain[2].data_ptr(), N, 0.05,
                                       0.9, 0.999, 1e-8, 0.01, step + 1, zero, 0.5, ops._stream()), 'plain')
            _lib.check(lib.istvt_adamw_groups(group[0].data_ptr(), gb.data_ptr(), group[1].data_ptr(), group[2].data_ptr(), N,
                                              seg_end.data_ptr(), seg_gid.data_ptr(), 1, lr, wd, 1, 0.9, 0.999, 1e-8,
                                              step + 1, zero, 0.5, None, 0, ops._stream()), 'groups')
        torch.cuda.synchronize()
        for a, b in zip(plain + [ga], group + [gb]):
            assert torch.equal(a, b), (kind, step)
        assert float(ga.abs().max()) == 0.0 if zero else torch.equal(ga, gv)
    assert not torch.equal(plain[0], p0)


# ---- 3. the norm kernel -------------------------------------------------------------------------------------------------
def _norm_sizes(parallel):
    c = parallel.GRAD_NORM_CHUNK
    return [1, 3, 255, 1025, c + 1, 3 * c + 5]


def test_grad_norm_is_exact_on_integers(parallel):
    gen = torch.Generator().manual_seed(7)
    for n in _norm_sizes(parallel):
        q = torch.nn.Parameter(torch.zeros(n, device='cuda'))
        bucket = parallel.GradBucket([q], flatten_params=True)
        opt = parallel.FusedSGD(bucket, lr=0.1, max_grad_norm=1e30)
        g = torch.randint(-3, 4, (n,), generator=gen)
        g[-1] = 3                                       # the last element counts (and the norm is never 0)
        bucket.flat.copy_(g.float())
        opt.step()
        want = np.float32(np.sqrt(np.float64(int((g.long() ** 2).sum()))))
        got = opt.grad_norm().item()
        assert np.float32(got) == want, (n, got, want)


def test_grad_norm_repeats_its_bits_and_matches_float64(parallel):
    from istvt_amd import _lib, ops
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(8)
    for n in _norm_sizes(parallel)[2:]:
        g = torch.randn(n, generator=gen)
        gd = g.cuda()
        ws = torch.empty(lib.istvt_grad_norm_ws_elems(n), dtype=torch.float64, device='cuda')
        infos = [torch.zeros(8, dtype=torch.int32, device='cuda') for _ in range(2)]
        for info in infos:
            ws.fill_(float('nan'))                      # the workspace's contents do not matter
            _lib.check(lib.istvt_grad_norm(gd.data_ptr(), n, 0.5, 0.0, 0, ws.data_ptr(), ws.numel(), info.data_ptr(),
                                           ops._stream()), 'istvt_grad_norm')
        assert torch.equal(infos[0], infos[1])
        norm, scale = infos[0][:2].view(torch.float32).tolist()
        want = float((0.5 * g.double()).norm())
        print('n = %d: norm %.9g, float64 %.9g, relative %.3g' % (n, norm, want, abs(norm - want) / want))
        assert abs(norm - want) <= 1e-6 * want
        assert scale == 0.5 and infos[0][2:].tolist() == [1, 0, 0, 0, 0, 0]     # no clipping, no skip mode: counters untouched


# ---- 4. clipping --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_clipping_matches_clip_grad_norm(parallel, kind):
    _, _, _, norms = run_against_torch(parallel, kind, clip=1.0, zero_grad=True)
    assert [n > 1.0 for n, _ in norms] == [True, False, True, False]        # large steps clip, small ones do not
    for mine, ref in norms:
        assert abs(mine - ref) <= 1e-6 * ref


@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_step_below_the_threshold_equals_the_unclipped_step(parallel, kind):
    init, grads = inputs()
    sides = [fused_optimizer(parallel, kind, init, max_grad_norm=clip) for clip in (1.0, None)]
    for ps, bucket, opt in sides:
        for q_, gv in zip(ps, grads[1]):                # a small set: norm ~ 0.74
            q_.grad.add_(gv)
        opt.step()
    assert 0.1 < float(sides[0][2].grad_norm()) < 1.0
    (pa, _, oa), (pb, _, ob) = sides
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert all(torch.equal(a, b) for a, b in zip(state_buffers(oa), state_buffers(ob)))
    assert not torch.equal(pa[0].detach().cpu(), init[0])


@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_clipping_sees_the_mean_gradient_under_a_pending_scale(parallel, kind):
    pa, _, _, na = run_against_torch(parallel, kind, steps=2, clip=1.0)
    pb, _, _, nb = run_against_torch(parallel, kind, steps=2, clip=1.0, grad_mult=4.0)      # the sum of a 4-rank world
    for (a, _), (b, _) in zip(na, nb):
        assert abs(a - b) <= 1e-6 * a
    for a, b in zip(pa, pb):
        assert relerr(b, a) < TOL


# ---- 5. skipping a non-finite step ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad_step', [0, 2])
@pytest.mark.parametrize('value', [float('inf'), float('nan')])
@pytest.mark.parametrize('kind', ['sgd', 'adamw'])
def test_nonfinite_step_is_skipped_without_a_trace(parallel, kind, value, bad_step):
    ps, bucket, opt, norms = run_against_torch(parallel, kind, bad=(bad_step, value), skip_nonfinite=True, zero_grad=True)
    assert int(opt.skipped_steps()) == 1
    assert not np.isfinite(norms[bad_step][0]) and all(np.isfinite(n) for i, (n, _) in enumerate(norms) if i != bad_step)
    assert opt.applied_steps() == STEPS - 1 and opt.steps == STEPS
    sd = opt.state_dict()
    assert sd['fused_steps'] == STEPS - 1 and set(sd['state']) == set(range(len(SHAPES)))
    if kind == 'adamw':
        assert all(float(st['step']) == STEPS - 1 for st in sd['state'].values())


# ---- 6. checkpoints -----------------------------------------------------------------------------------------------------
def two_groups(ps):
    return [{'params': [ps[0], ps[2], ps[4]], 'lr': 0.05, 'weight_decay': 0.0}, {'params': [ps[1], ps[3], ps[5]], 'lr': 0.01}]


@pytest.mark.parametrize('skip', [False, True])
def test_two_group_checkpoint_round_trips_through_torch(parallel, skip):
    init, grads = inputs()
    ps, bucket, opt = fused_optimizer(parallel, 'adamw', init, groups=two_groups, skip_nonfinite=skip)
    for step in range(2):
        opt.zero_grad()
        for q_, gv in zip(ps, grads[step]):
            q_.grad.add_(gv)
        opt.step()
    sd = opt.state_dict()
    assert [g['params'] for g in sd['param_groups']] == [[0, 1, 2], [3, 4, 5]]         # torch's numbering: group by group
    assert sd['state'][1]['exp_avg'].shape == ps[2].shape and sd['state'][3]['exp_avg'].shape == ps[1].shape
    assert all(float(st['step']) == 2 for st in sd['state'].values())
    # fused -> torch
    t_p = [torch.nn.Parameter(q_.detach().clone()) for q_ in ps]
    t_o = torch_optimizer('adamw', t_p, groups=two_groups)
    t_o.load_state_dict({'state': sd['state'], 'param_groups': sd['param_groups']})
    # torch -> a fresh fused optimizer
    ps2, bucket2, opt2 = fused_optimizer(parallel, 'adamw', [q_.detach().cpu() for q_ in ps], groups=two_groups,
                                         skip_nonfinite=skip)
    opt2.load_state_dict(t_o.state_dict())
    assert opt2.applied_steps() == 2
    for p_, q_, r_, gv in zip(t_p, ps, ps2, grads[2]):
        p_.grad = gv.clone()
        q_.grad.copy_(gv)
        r_.grad.copy_(gv)
    t_o.step(); opt.step(); opt2.step()
    for p_, q_, r_ in zip(t_p, ps, ps2):
        assert relerr(q_, p_) < TOL and torch.equal(q_, r_)
    # a checkpoint with another number of groups (or another split) is refused
    _, _, one = fused_optimizer(parallel, 'adamw', init, groups=None)
    with pytest.raises(ValueError, match='param group'):
        opt.load_state_dict(one.state_dict())
    with pytest.raises(ValueError, match='param group'):
        one.load_state_dict(sd)
    _, _, other = fused_optimizer(parallel, 'adamw', init)                              # three groups: 3 + 2 + 1
    with pytest.raises(ValueError, match='param group'):
        other.load_state_dict(sd)
