"""CPU tests of tests/fp8_emulation.py, the fp64 restatement the fp8 spatial-attention kernels are judged against
(gpu_checks.attn_spatial_fp8_emulated): the formulas (quantisation off == autograd), torch's e4m3 rounding on known
values, how loose the old reference (float64 attention of the unquantised inputs) is and what the new one sees, and how
little of a kernel-vs-restatement difference rounding flips of the quantised probabilities could explain."""
import pytest
import torch

import fp8_emulation as E

SHAPES = [(P, dh) for P in (37, 197, 362) for dh in (32, 64)]


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _inputs(P, dh, heads=2, BF=2, seed=0):
    """bf16-representable q, k, v, dout [BF, heads, P, dh] in float64 (|x| < 448 by a wide margin)"""
    g = torch.Generator().manual_seed(seed + 1000 * P + dh)
    return tuple(torch.randn((BF, heads, P, dh), generator=g).to(torch.bfloat16).double() for _ in range(4))


def _true_attention(q, k, v, dout):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = ((q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5).softmax(-1) @ v
    out.backward(dout)
    return {'out': out.detach(), 'dq': q.grad, 'dk': k.grad, 'dv': v.grad}


@pytest.mark.parametrize('P,dh', SHAPES)
def test_quantisation_off_is_autograd_attention(P, dh):
    q, k, v, dout = _inputs(P, dh)
    ref = _true_attention(q, k, v, dout)
    for chunk in (E.CHUNK, None):
        r = E.attention(q, k, v, dout, quantise=False, chunk=chunk)
        for n in ('out', 'dq', 'dk', 'dv'):
            assert relerr(r[n], ref[n]) <= 1e-12, (n, relerr(r[n], ref[n]))
    S = (q @ k.transpose(-1, -2)) * dh ** -0.5
    assert torch.equal(r['m'], S.amax(-1))
    assert relerr(r['inv_l'], 1.0 / torch.exp(S - S.amax(-1, keepdim=True)).sum(-1)) <= 1e-14


def test_packed_layout_matches_per_head():
    BF, P, heads, dh = 2, 37, 2, 32
    q, k, v, dout = _inputs(P, dh, heads, BF)

    def merge(t):
        return t.transpose(1, 2).reshape(BF * P, heads * dh)
    qkv = torch.cat([merge(t) for t in (q, k, v)], dim=-1)
    out, lse, dqkv = E.spatial_attention(qkv, merge(dout), BF, P, heads, dh)
    r = E.attention(q, k, v, dout)
    assert torch.equal(out, merge(r['out']))
    assert torch.equal(dqkv, torch.cat([merge(r[n]) for n in ('dq', 'dk', 'dv')], dim=-1))
    assert tuple(lse.shape) == (BF * P, heads, 2)
    assert torch.equal(lse[:, :, 1].reshape(BF, P, heads).transpose(1, 2), r['inv_l'])
    assert torch.equal(lse[:, :, 0].reshape(BF, P, heads).transpose(1, 2), r['m'] * 1.4426950408889634)


def test_e4m3_known_values():
    """what torch's float8_e4m3fn conversion gives today; pinned against a torch upgrade (round to nearest even on 3
    mantissa bits, subnormals down to 2^-9, 448 finite)"""
    cases = [(17.0, 16.0), (19.0, 20.0), (18.0, 18.0), (448.0, 448.0), (2.0 ** -9, 2.0 ** -9), (2.0 ** -10, 0.0),
             (1.5 * 2.0 ** -9, 2.0 ** -8), (256.0, 256.0), (-17.0, -16.0), (-2.0, -2.0), (1.0, 1.0), (0.0, 0.0)]
    x = torch.tensor([c[0] for c in cases], dtype=torch.float64)
    want = torch.tensor([c[1] for c in cases], dtype=torch.float64)
    got = E.e4m3(x)
    assert got.dtype == torch.float64 and torch.equal(got, want), (got, want)
    assert torch.equal(E.e4m3(x.float()), want.float())
    # integers -2..2 (the exact-valued GPU checks' data) are representable
    ints = torch.arange(-2, 3, dtype=torch.float64)
    assert torch.equal(E.e4m3(ints), ints)


# (a row, b row, what one v_mfma_f32_16x16x32_fp8_fp8 on a zero accumulator returned on MI355X, the exact dot product):
# two products in one 8-group, a whole 8-group of operands spanning 2^-6 .. 2^6, an 8-group of normal data, and K = 32
MFMA_RECORDED = [
    ([-0.75, -0.0234375], [-40.0, -0.5625], 30.01171875, 30.01318359375),
    ([-0.75, -0.0234375], [30.0, 0.05078125], -22.5009765625, -22.501190185546875),
    ([64.0, 15.0], [-40.0, -0.5625], -2568.25, -2568.4375),
    ([64.0, 15.0], [30.0, 0.05078125], 1920.75, 1920.76171875),
    ([-10.0, -13.0], [30.0, 0.05078125], -300.65625, -300.66015625),
    ([-1.875, -22.0], [-1.625, -64.0], 1411.0, 1411.046875),
    ([-1.375, 80.0, -64.0, 18.0, -9.0, -0.0546875, 0.5, -0.9375],
     [-10.0, 0.1171875, -0.46875, -6.0, -3.75, 12.0, -0.04296875, -4.0], -18.046875, -18.052734375),
    ([-1.375, 80.0, -64.0, 18.0, -9.0, -0.0546875, 0.5, -0.9375],
     [-9.0, 0.029296875, 0.4375, 0.0859375, 0.9375, -0.021484375, -0.234375, -2.25], -18.1796875, -18.178512573242188),
    ([-1.375, 80.0, -64.0, 18.0, -9.0, -0.0546875, 0.5, -0.9375],
     [0.28125, 64.0, -1.375, 0.1015625, -0.1875, 9.0, -15.0, 1.375], 5202.5, 5201.84765625),
    ([0.05859375, -0.9375, 1.125, -0.1875, 0.6875, 0.75, 1.0, -0.8125],
     [-0.140625, -0.9375, 0.375, 0.21875, -0.078125, -0.04296875, 1.25, 1.0], 1.6031494140625, 1.60308837890625),
    ([0.05859375, -0.9375, 1.125, -0.1875, 0.6875, 0.75, 1.0, -0.8125],
     [-0.0859375, -1.375, -1.375, -1.5, 0.125, -1.125, -0.5625, 0.203125], -1.4669189453125, -1.466949462890625),
    ([0.05859375, -0.9375, 1.125, -0.1875, 0.6875, 0.75, 1.0, -0.8125],
     [0.1015625, -1.5, -0.234375, 0.5625, 0.5, 0.1875, 1.625, -0.9375], 3.9140625, 3.914154052734375),
    ([-1.5, -0.75, -0.625, -1.625, -0.1015625, -0.625, -1.0, -1.625, -0.6875, 0.3125, -0.75, -0.25, -0.21875, 1.625,
      0.234375, 0.46875, -0.6875, -1.125, 0.6875, 0.203125, 0.875, 0.25, -0.6875, 0.8125, 1.125, -0.171875, -2.25, -1.5,
      0.0625, -0.625, -0.8125, -0.125],
     [-0.109375, -0.75, 0.15625, 2.0, -0.203125, 0.6875, -0.15625, -1.375, 1.125, -0.46875, -1.125, -0.171875, -0.5, 2.0,
      0.28125, -2.0, 1.375, 0.40625, -1.5, -1.5, 0.9375, 0.3125, 0.140625, -0.9375, -0.5, -0.04296875, 1.0, 0.6875,
      0.6875, -0.40625, 0.125, -0.1171875], -4.509765625, -4.50958251953125),
    ([1.875, -0.0703125, 0.15625, -0.75, 0.203125, 0.046875, 0.15625, -0.46875, -0.109375, 0.28125, -0.15625,
      -0.029296875, 2.25, -1.0, 1.625, -0.625, -0.9375, 0.5625, 0.0625, -0.4375, 0.75, 0.4375, 1.125, 2.0, 0.140625,
      0.9375, -0.1875, -0.625, 1.5, -0.875, -3.25, -0.75],
     [0.375, -0.4375, -1.375, -0.15625, 0.75, 0.6875, 1.375, 1.125, 1.0, 0.625, 0.625, -0.28125, -1.25, 0.9375, 1.25,
      0.6875, 1.75, 1.125, -1.5, 1.125, -0.6875, 0.75, 1.5, -1.0, -0.6875, 0.9375, -0.5, -1.375, -1.0, 2.0, -0.15625,
      0.0234375], -4.781494140625, -4.78131103515625),
]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mfma_fp8_dot_reproduces_recorded_results(dtype):
    """mfma_fp8_dot on operands whose MFMA result was recorded on MI355X: bit-equal to the instruction (every recorded
    case is one where the instruction is NOT the rounded exact product), in both dtypes the restatement is run in"""
    for a, b, got, exact in MFMA_RECORDED:
        a, b = torch.tensor([a], dtype=dtype), torch.tensor([b], dtype=dtype)
        assert torch.equal(E.e4m3(a), a) and torch.equal(E.e4m3(b), b)
        assert float((a.double() * b.double()).sum()) == exact and float(torch.tensor(exact).float()) != got
        assert float(E.mfma_fp8_dot(a, b)) == got, (a, b, float(E.mfma_fp8_dot(a, b)), got)
    # integer-valued operands in -2..2 (the exact-valued GPU checks): every product is inside the window
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randint(-2, 3, (50, 64), generator=g).to(dtype) for _ in range(2))
    assert torch.equal(E.mfma_fp8_dot(a, b), a @ b.t())


@pytest.mark.parametrize('P,dh', SHAPES)
def test_mfma_window_moves_the_statistics(P, dh):
    """what the accumulation window of the fp8 MFMA does to the restatement: the statistics move by more than their
    float32 bound, so it has to be modelled; the output and the gradients (printed) move by up to a quarter of theirs,
    through probabilities that land on the other side of an e4m3 rounding boundary"""
    q, k, v, dout = _inputs(P, dh)
    a = E.attention(q, k, v, dout)
    b = E.attention(q, k, v, dout, mfma_window=False)
    m_err = float(((a['m'] - b['m']).abs() / b['m'].abs()).max())
    l_err = float(((a['inv_l'] - b['inv_l']).abs() / b['inv_l']).max())
    vals = {n: relerr(a[n], b[n]) for n in ('out', 'dq', 'dk', 'dv')}
    print('P=%d dh=%d: with vs without the MFMA window: m %.2e 1/l %.2e (element-wise)' % (P, dh, m_err, l_err),
          ' '.join('%s %.2e' % kv for kv in vals.items()))
    assert max(m_err, l_err) > 2e-5


@pytest.mark.parametrize('P,dh', SHAPES)
def test_old_reference_is_loose_and_new_one_sees_a_dropped_key(P, dh):
    q, k, v, dout = _inputs(P, dh)
    ref = _true_attention(q, k, v, dout)
    r = E.attention(q, k, v, dout)
    floor = {n: relerr(r[n], ref[n]) for n in ('out', 'dq', 'dk', 'dv')}
    print('P=%d dh=%d: restatement vs float64 attention of the unquantised inputs:' % (P, dh),
          ' '.join('%s %.2e' % kv for kv in floor.items()))
    # the floor a bound against true attention carries whatever the kernel does
    assert min(floor.values()) > 2e-2, floor
    # the same restatement with the last key removed from K and V: what the new bound must see
    d = E.attention(q, k[..., :-1, :], v[..., :-1, :], dout)
    drop = {'out': relerr(d['out'], r['out']), 'dq': relerr(d['dq'], r['dq'])}
    print('P=%d dh=%d: last key dropped vs restatement: out %.2e dq %.2e (bound %.0e; 8e-2 vs true attention: %.2e)'
          % (P, dh, drop['out'], drop['dq'], E.TOL_BF16_ONE_ROUNDING, relerr(d['out'], ref['out'])))
    assert drop['out'] > 10 * E.TOL_BF16_ONE_ROUNDING, drop
    # the online softmax: quantising every chunk's probabilities at the running maximum instead of the final one is a
    # difference the bound sees too, so the restatement has to walk the chunks as the kernels do
    one = E.attention(q, k, v, dout, chunk=None)
    print('P=%d dh=%d: one-chunk formula vs chunks of %d: out %.2e' % (P, dh, E.CHUNK, relerr(one['out'], r['out'])))
    if P <= E.CHUNK:
        assert torch.equal(one['out'], r['out'])


@pytest.mark.parametrize('P,dh', SHAPES)
def test_self_noise_float32_vs_float64(P, dh):
    """the restatement evaluated in float32 and in float64, P and dS additionally rounded to bf16 as the kernels round
    them: what separates the two is flips of quantised probabilities / bf16 roundings that sit on a rounding boundary.
    Below 5e-4 = 1/8 of the bound of the GPU check, so flips cannot explain a failure there."""
    q, k, v, dout = _inputs(P, dh)
    a = E.attention(q, k, v, dout, dtype=torch.float32, round_bf16=True)
    b = E.attention(q, k, v, dout, dtype=torch.float64, round_bf16=True)
    noise = {n: relerr(a[n], b[n]) for n in ('out', 'dq', 'dk', 'dv')}
    print('P=%d dh=%d: restatement float32 vs float64:' % (P, dh), ' '.join('%s %.2e' % kv for kv in noise.items()))
    assert max(noise.values()) < 5e-4, noise
    assert relerr(a['inv_l'], b['inv_l']) < 1e-5 and relerr(a['m'], b['m']) < 1e-5
