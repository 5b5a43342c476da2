"""The fused backward of a separable unit's BatchNorm + 1x1 convolution (csrc/pw_bwd.hip, ops.pw_bwd,
stem.pointwise_bn_backward) against the three launches it replaces, which stay in the tree as the fallback:
stem.bn_backward + ops.linear_dgrad + ops.linear_wgrad, plus a float64 restatement of the weight gradient.

Bounds (u = 2^-24, the unit roundoff of fp32; du = the three-launch path's bf16 du):
  dgamma, dbeta   equal in every bit (the same s2 / s1 added once).
  dd              |new - old| <= 2^-7 |old| + 2 Cout u sum_c |du_c| |w_c|: both sides sum the same exact products in fp32,
                  possibly in another order (second term), then round once to bf16 (first term: one bf16 ulp is 2^-7
                  relative at most).
  dW              |new - (P + dW_64)| <= M u (sum_m |du_mn| |d_mk| + |P|), P the value the output held before: the fp32
                  summation bound for the M + 1 terms (M additions) of which the pre-filled value is the first.  With
                  P = 0 this is the M u sum |du| |d| of a plain weight gradient.  (Without the |P| term no fp32 result
                  can hold the bound at M = 1: there the only rounding is that of P + du d.)
                  And: equal in every bit to ops.linear_wgrad(du, d, out=P).  The kernel cuts the rows into the chunks that
                  weight gradient's reduction split cuts them into and feeds its MFMA chain in the same order, so that
                  a training run keeps the trajectory of the three launches.

Rows: a launch over M rows has G(M) = ops.pw_bwd_geometry(M)[0] workgroups (the reduction split of linear_wgrad: 1 below
1024 rows, 256 from 131072), each with one contiguous chunk of rows, a multiple of 64, in blocks of R = 128.  M = 1, R - 1,
R, R + 1: one workgroup, one or two blocks.  256 R + 77 = 32845: 58 chunks of 576 rows (four and a half blocks; the
last chunk 13 rows).  128 R + 5 = 16389: 29 chunks.  131269: 228 chunks, the split's cap in play.

Measured on an MI355X: dd equal in every bit in all 56 runs; dW equal in every bit to linear_wgrad's; against float64 the
worst error / bound is 1.0 at M = 1 with a pre-filled value (that one rounding), 1.3e-2 at M = 127 .. 129, below 3e-5 from
M = 16389; whole stem: worst cosine 1 - 2e-16.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
PAIRS = ((64, 128), (128, 128))


def _mods():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import _lib, ops, stem
    return _lib, ops, stem


def _m_values():
    _, ops, _ = _mods()
    G, R = 256, ops.pw_bwd_geometry(1)[1]         # G: the workgroups a launch aims for
    return {'one': 1, 'R-1': R - 1, 'R': R, 'R+1': R + 1, 'GR+77': G * R + 77, 'below': (G // 2) * R + 5, 'many': 131269}


_CASES = {}


def _case(cin, cout, mkey, training):
    """inputs, the three-launch reference and the float64 weight gradient of one case, computed once"""
    key = (cin, cout, mkey, training)
    if key in _CASES:
        return _CASES[key]
    _lib, ops, stem = _mods()
    M = _m_values()[mkey]
    dev = torch.device('cuda')
    gen = torch.Generator(device='cuda').manual_seed(1000 * cin + 10 * len(mkey) + int(training) + M)
    rn = lambda *s: torch.randn(*s, generator=gen, device=dev)              # noqa: E731
    dz = rn(M, cout).to(torch.bfloat16)
    u = (rn(M, cout) * 1.5 + 0.25).to(torch.bfloat16)
    d = rn(M, cin).to(torch.bfloat16)
    w = (rn(cout, cin) / cin ** 0.5).to(torch.bfloat16)
    gamma = (1.0 + 0.2 * rn(cout)).contiguous()
    beta = (0.1 * rn(cout)).contiguous()
    rmean, rvar = (0.1 * rn(cout)).contiguous(), (1.0 + 0.1 * rn(cout).abs()).contiguous()
    # the BatchNorm pack and the backward sums come from the project's own statistics kernels
    st = stem.bn_forward_stats(u, M, cout, gamma, beta, rmean, rvar, training)
    R_ = int(_lib.lib().istvt_stats_replicas())
    acc = torch.zeros((R_, 2, cout), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().istvt_bn_bwd_stats(dz.data_ptr(), u.data_ptr(), st.ptr(), acc[0, 0].data_ptr(), acc[0, 1].data_ptr(),
                                             M, cout, ops.dtype_code(u), ops._stream()), 'istvt_bn_bwd_stats')
    dg0, db0 = 0.5 * rn(cout), 0.5 * rn(cout)                              # what dgamma / dbeta hold before
    dg_old, db_old = dg0.clone(), db0.clone()
    du, _, _ = stem.bn_backward(dz, u, st, gamma, M, cout, stats=acc.clone(), dg=dg_old, db=db_old, training=training)
    dd_old = ops.linear_dgrad(du, w, blocked=False)
    du64, d64 = du.double(), d.double()
    c = dict(M=M, dz=dz, u=u, d=d, w=w, gamma=gamma, st=st, acc=acc, dg0=dg0, db0=db0, dg_old=dg_old, db_old=db_old, du=du,
             dd_old=dd_old, dd_slack=2.0 * cout * U24 * (du64.abs() @ w.double().abs()),
             dW64=du64.t() @ d64, dW_abs=du64.abs().t() @ d64.abs(), training=training)
    torch.cuda.synchronize()
    _CASES[key] = c
    return c


def _fused(c, cin, cout, prefill):
    _, _, stem = _mods()
    out = prefill.clone()
    dg, db = c['dg0'].clone(), c['db0'].clone()
    dd, dW = stem.pointwise_bn_backward(c['dz'], c['u'], c['st'], c['gamma'], c['M'], cout, c['d'], c['w'], cin,
                                        c['acc'].clone(), dg, db, out, c['training'])
    assert dW is None
    return dd, out, dg, db


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('mkey', ['one', 'R-1', 'R', 'R+1', 'GR+77', 'below', 'many'])
@pytest.mark.parametrize('pair', PAIRS, ids=['64to128', '128to128'])
def test_fused_matches_three_launches(pair, mkey, training, monkeypatch):
    monkeypatch.setenv('ISTVT_STEM_PW_BWD_FUSED', '1')
    _, ops, _ = _mods()
    cin, cout = pair
    c = _case(cin, cout, mkey, training)
    M = c['M']
    assert ops.pw_bwd_fusable(c['dz'], c['d'], c['w'])
    gen = torch.Generator(device='cuda').manual_seed(7)
    fills = {'zeros': torch.zeros((cout, cin), device='cuda'),
             'nonzero': torch.randn((cout, cin), generator=gen, device='cuda') + 0.5}
    for name, P in fills.items():
        dd, out, dg, db = _fused(c, cin, cout, P)
        # 1: BatchNorm parameter gradients, every bit
        assert torch.equal(dg, c['dg_old']) and torch.equal(db, c['db_old']), (name, 'dgamma / dbeta')
        # 2: input gradient
        old = c['dd_old'].double()
        err = (dd.double() - old).abs()
        lim = 2.0 ** -7 * old.abs() + c['dd_slack']
        same = int((dd.view(torch.int16) == c['dd_old'].view(torch.int16)).sum())
        print('%s M=%d %s prefill %s: dd bit-equal %d of %d, worst err/bound %.3f'
              % (pair, M, 'train' if training else 'eval', name, same, dd.numel(), float((err / lim.clamp_min(1e-300)).max())))
        assert tuple(dd.shape) == (M, cin) and bool((err <= lim).all()), (name, 'dd', float((err - lim).max()))
        # 3: weight gradient against float64, the pre-filled value on both sides
        ref = P.double() + c['dW64']
        errw = (out.double() - ref).abs()
        limw = M * U24 * (c['dW_abs'] + P.double().abs())
        print('   dW worst err/bound %.3e' % float((errw / limw.clamp_min(1e-300)).max()))
        assert bool((errw <= limw).all()), (name, 'dW', float((errw - limw).max()))
        assert torch.equal(out, ops.linear_wgrad(c['du'], c['d'], out=P.clone())), (name, 'dW bits of linear_wgrad')
        # 4: a second run gives the same bits
        dd2, out2, _, _ = _fused(c, cin, cout, P)
        assert torch.equal(dd2.view(torch.int16), dd.view(torch.int16)) and torch.equal(out2, out), (name, 'run to run')


@pytest.mark.parametrize('shape', [(64, 64), (128, 256), (32, 128), (256, 128)])
def test_other_shapes_are_refused_and_touch_nothing(shape):
    """(Cin, Cout) outside the two instantiated pairs: the library's shape error, before any launch"""
    _lib, ops, stem = _mods()
    cin, cout = shape
    M = 300
    dev = torch.device('cuda')
    dz = torch.randn(M, cout, device=dev).to(torch.bfloat16)
    u = torch.randn(M, cout, device=dev).to(torch.bfloat16)
    d = torch.randn(M, cin, device=dev).to(torch.bfloat16)
    w = torch.randn(cout, cin, device=dev).to(torch.bfloat16)
    assert not ops.pw_bwd_fusable(dz, d, w)
    pack = torch.ones((4, cout), device=dev)
    gamma = torch.ones(cout, device=dev)
    acc = torch.ones((int(_lib.lib().istvt_stats_replicas()), 2, cout), dtype=torch.float64, device=dev)
    out, dg, db = torch.full((cout, cin), 3.0, device=dev), torch.full((cout,), 4.0, device=dev), torch.full((cout,), 5.0, device=dev)
    dd = torch.full((M, cin), 7.0, device=dev).to(torch.bfloat16)
    wt = w.t().contiguous()
    ws = torch.full((ops.pw_bwd_geometry(M)[0], cout * cin), 9.0, device=dev)
    rc = _lib.lib().istvt_pw_bwd(dz.data_ptr(), u.data_ptr(), pack.data_ptr(), gamma.data_ptr(), acc[0, 0].data_ptr(),
                                 acc[0, 1].data_ptr(), d.data_ptr(), cin, wt.data_ptr(), cout, dd.data_ptr(), ws.data_ptr(),
                                 out.data_ptr(), dg.data_ptr(), db.data_ptr(), M, cin, cout, 1, ops.dtype_code(dz), ops._stream())
    torch.cuda.synchronize()
    assert rc == -3                                                        # ISTVT_ERR_SHAPE
    assert bool((out == 3.0).all()) and bool((dg == 4.0).all()) and bool((db == 5.0).all())
    assert bool((dd.float() == 7.0).all()) and bool((ws == 9.0).all())
    with pytest.raises(RuntimeError, match='invalid shape'):
        ops.pw_bwd(dz, u, pack, gamma, acc, d, w, out, dg, db, True)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((dg == 4.0).all()) and bool((db == 5.0).all())


def test_float32_is_refused():
    _lib, ops, stem = _mods()
    dev = torch.device('cuda')
    dz, d, w = torch.randn(256, 128, device=dev), torch.randn(256, 64, device=dev), torch.randn(128, 64, device=dev)
    assert not ops.pw_bwd_fusable(dz, d, w)


# the bounds tests/test_model_gpu.py holds the bf16 stem's gradients to (direction and norm), taken from that file
def _stem_bounds():
    import test_model_gpu as T
    return T.BF16_STEM_COS, T.BF16_STEM_NORM


def _stem_grads(fused, training):
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import stem
    from istvt_amd.network import xception as X
    os.environ['ISTVT_STEM_PW_BWD_FUSED'] = '1' if fused else '0'
    torch.manual_seed(11)
    net = X.xception(pretrained=False).cuda()
    net = net.train() if training else net.eval()
    gen = torch.Generator().manual_seed(12)
    x = torch.randn((2, 3, 35, 35), generator=gen).cuda().requires_grad_(True)
    y = stem.stem_forward(x, net, torch.bfloat16)
    coef = torch.randn(tuple(y.shape), generator=gen).cuda().to(y.dtype)
    (y.float() * coef.float()).sum().backward()
    torch.cuda.synchronize()
    names = set(stem.param_names())
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if k in names}
    return grads, x.grad.detach().clone(), y.detach().clone()


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_whole_stem_backward_fused_against_fallback(training, monkeypatch):
    """StemFn forward + backward, 2 frames of 35 x 35 (block1 at M = 450), bf16, with the switch at 0 and at 1.  Everything
    upstream of the first fused launch -- block3, block2, block1's skip path and the BatchNorm of block1's second unit --
    is computed from identical inputs: identical bits.  Behind it the input gradient differs by the fp32 summation order
    inside one bf16 rounding, and every tensor stays within the direction / norm bounds of tests/test_model_gpu.py."""
    monkeypatch.setenv('ISTVT_STEM_PW_BWD_FUSED', '1')                      # (restored after the test)
    cos_min, norm_tol = _stem_bounds()
    g0, dx0, y0 = _stem_grads(False, training)
    g1, dx1, y1 = _stem_grads(True, training)
    assert torch.equal(y0, y1)
    assert len(g0) == len(g1) >= 39
    upstream = ('block2.', 'block3.', 'block1.skip', 'block1.rep.4.')
    rows = []
    for k in sorted(g0):
        a, b = g1[k].double().flatten(), g0[k].double().flatten()
        if k.startswith(upstream):
            assert torch.equal(g1[k], g0[k]), k
            continue
        cos = float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))
        ratio = float(a.norm() / b.norm().clamp_min(1e-300))
        rows.append((cos, ratio, k))
        assert cos > cos_min and abs(ratio - 1.0) < norm_tol, (k, cos, ratio)
    a, b = dx1.double().flatten(), dx0.double().flatten()
    cos, ratio = float((a @ b) / (a.norm() * b.norm())), float(a.norm() / b.norm())
    print('stem %s: worst cosine %s, dx cosine %.6f ratio %.5f' % ('train' if training else 'eval', min(rows)[::2], cos, ratio))
    assert cos > cos_min and abs(ratio - 1.0) < norm_tol
