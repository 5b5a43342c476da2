"""The fused criterion, host side: the float64 restatement against torch's own
binary_cross_entropy_with_logits; the meter's ratios; the argument checks, all of which fire before a device is asked for.  No GPU and no kernel runs here."""
import math

import pytest
import torch
import torch.nn.functional as F

EXTREME = [0.0, 1e-3, -1e-3, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4]


@pytest.fixture(scope='module')
def L():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import loss
    return loss


def relerr(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _cases():
    g = torch.Generator().manual_seed(3)
    z = torch.cat([torch.tensor(EXTREME).repeat(2), torch.randn(31, generator=g) * 3]).double()
    y = torch.cat([torch.zeros(9), torch.ones(9), (torch.rand(31, generator=g) > 0.5).float()]).double()
    w = (torch.rand(z.shape[0], generator=g) + 0.25).double()
    return z, y, w


@pytest.mark.parametrize('reduction', ['mean', 'sum', 'none'])
@pytest.mark.parametrize('use_w, p', [(False, None), (True, None), (False, 3.0), (True, 3.0)],
                         ids=['plain', 'weight', 'pos_weight', 'both'])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_ref_matches_torch_float64(L, reduction, use_w, p, eps):
    z, y, w = _cases()
    w = w if use_w else None
    zt = z.clone().requires_grad_()
    ys = y * (1 - eps) + eps / 2                                    # smoothed targets passed to torch
    t = F.binary_cross_entropy_with_logits(zt, ys, weight=w, reduction=reduction,
                                           pos_weight=None if p is None else torch.tensor(p, dtype=torch.float64))
    t.sum().backward()
    r = L.bce_logits_ref(z, y, weight=w, pos_weight=1.0 if p is None else p, label_smoothing=eps, reduction=reduction)
    assert relerr(r['loss'] if reduction == 'none' else r['reduced'], t.detach()) <= 1e-12
    assert relerr(r['grad'], zt.grad) <= 1e-12
    assert torch.isfinite(r['loss']).all() and torch.isfinite(r['grad']).all()
    # the wrong side of a huge logit costs |z| (times pos_weight for a missed positive)
    if eps == 0.0 and w is None:
        assert float(r['loss'][7]) == 1e4 and float(r['loss'][9 + 8]) == 1e4 * (p or 1.0)
    c = r['counts']
    assert c['seen'] == z.shape[0] and c['correct'] == c['tp'] + c['tn'] and c['tp'] + c['tn'] + c['fp'] + c['fn'] == c['seen']
    assert c['correct'] == int(((z > 0) == (y > 0.5)).sum())


def test_ref_threshold_and_nan_follow_the_comparison(L):
    z = torch.tensor([float('nan'), float('nan'), 0.5, 0.5, 2.0])
    y = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])
    c = L.bce_logits_ref(z, y, threshold=1.0)['counts']
    # NaN > t is false: predicted negative; 0.5 is below the threshold of 1
    assert (c['tp'], c['tn'], c['fp'], c['fn']) == (1, 2, 0, 2)


def test_meter_arithmetic(L):
    s = L.MeterSnapshot(loss_sum=12.0, batch_loss_sum=1.5, seen=48, correct=36, tp=20, tn=16, fp=8, fn=4, calls=3)
    assert s.loss_mean == 0.25 and s.batch_loss_sum == 1.5 and s.accuracy == 0.75
    assert s.apcer == 4 / 24 and s.bpcer == 8 / 24 and s.acer == (4 / 24 + 8 / 24) / 2
    assert s.counts == {'seen': 48, 'correct': 36, 'tp': 20, 'tn': 16, 'fp': 8, 'fn': 4, 'calls': 3}
    empty = L.MeterSnapshot()
    assert all(math.isnan(v) for v in (empty.loss_mean, empty.accuracy, empty.apcer, empty.bpcer, empty.acer))
    only_real = L.MeterSnapshot(loss_sum=1.0, seen=4, correct=3, tn=3, fp=1, calls=1)      # no attack seen: APCER undefined
    assert math.isnan(only_real.apcer) and only_real.bpcer == 0.25 and math.isnan(only_real.acer)
    only_attack = L.MeterSnapshot(loss_sum=1.0, seen=4, correct=4, tp=4, calls=1)
    assert only_attack.apcer == 0.0 and math.isnan(only_attack.bpcer)


def test_argument_validation(L):
    crit = L.BCEWithLogitsLoss()
    z, y = torch.zeros(4), torch.zeros(4)
    with pytest.raises(RuntimeError, match='ROCm device'):                  # wrong device: no CPU path
        crit(z, y)
    with pytest.raises(RuntimeError, match='ROCm device'):
        L.TrainMeter('cpu')
    with pytest.raises(TypeError, match='float32'):                         # wrong dtypes
        crit(z.double(), y)
    with pytest.raises(TypeError, match='float32'):
        crit(z.bfloat16(), y)
    with pytest.raises(TypeError, match='targets'):
        crit(z, y.to(torch.int16))
    with pytest.raises(RuntimeError, match=r'view\(-1\)'):                  # 2-D logits
        crit(torch.zeros(4, 1), y)
    with pytest.raises(RuntimeError, match='4 logits'):                     # length mismatch
        crit(z, torch.zeros(5))
    with pytest.raises(RuntimeError, match='per-sample weight'):
        L.BCEWithLogitsLoss(weight=torch.ones(3))(z, y)
    with pytest.raises(TypeError, match='weight'):
        L.BCEWithLogitsLoss(weight=torch.ones(4, dtype=torch.float64))
    for eps in (-0.1, 1.0, 1.5):                                            # label smoothing outside [0, 1)
        with pytest.raises(ValueError, match='label_smoothing'):
            L.BCEWithLogitsLoss(label_smoothing=eps)
    with pytest.raises(ValueError, match='reduction'):
        L.BCEWithLogitsLoss(reduction='batchmean')
    with pytest.raises(ValueError, match='pos_weight'):
        L.BCEWithLogitsLoss(pos_weight=torch.ones(2))
    with pytest.raises(TypeError, match='TrainMeter'):
        L.BCEWithLogitsLoss(meter=torch.zeros(10, dtype=torch.int64))
    assert L.BCEWithLogitsLoss(pos_weight=torch.tensor([2.5])).pos_weight == 2.5       # read once, here


def test_c_abi_refuses_bad_arguments(L):
    """the entry points validate before they launch: these calls return -2 / -3 without touching a device"""
    from istvt_amd import _lib
    lib = _lib.lib()
    ok = dict(z=8, stride=1, y=8, kind=0, w=None, p=1.0, eps=0.0, red=1, thr=0.0, n=4)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.istvt_bce_logits(a['z'], a['stride'], a['y'], a['kind'], a['w'], a['p'], a['eps'], a['red'], a['thr'], a['n'],
                                    None, None, None, None, None)
    assert call(z=None) == -3 and call(y=None) == -3 and call(n=0) == -3 and call(n=(1 << 30) + 1) == -3
    assert call(stride=0) == -3 and call(red=3) == -3 and call(eps=1.0) == -3 and call(eps=-0.5) == -3
    assert call(eps=float('nan')) == -3 and call(kind=4) == -2 and call(kind=-1) == -2
    assert lib.istvt_bce_logits_bwd(None, 8, 0, 8, 4, None) == -3 and lib.istvt_bce_logits_bwd(8, 8, 0, 8, 0, None) == -3
