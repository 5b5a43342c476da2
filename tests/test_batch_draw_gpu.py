"""The batch draw (DESIGN.md "Batch draw") on a real MI355X: ops.batch_draw against the definition clips.batch_draw_host, bit
for bit and across the carry of the step counter; what the kernel writes of its draw block and what it leaves alone (the
block's guard band); a doctored header; ops.jpeg_decode_drawn_u8 against the indexed decode of the definition's index;
ops.draw_clips against the chain of existing calls on the definition's host tables, eager and as a replayed graph; the model's
view_checked=True.  tools/batch_draw_check.cpp, csrc/batch_draw.h under AddressSanitizer and UBSan on the host, has passed
before the kernel ran on a device: DESIGN.md has the command and its counts."""
import json
import os

import pytest
import torch

from test_batch_draw_cpu import FILL, after_draw, long_videos, refused, small_plan
from test_jpeg_split_cpu import _smooth

pytestmark = pytest.mark.gpu

TABLES = ('index', 'boxes', 'quality', 'view', 'perturb', 'label')
S = 16


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.fixture(scope='module')
def record(golden_dir):
    with open(os.path.join(golden_dir, 'B1_batch_draw.json')) as fh:
        return json.load(fh)


def _same(draw, want):
    return all(torch.equal(getattr(draw, name).cpu(), getattr(want, name)) for name in TABLES)


def _step_of(words):
    lo, hi = (int(v) & 0xffffffff for v in words.cpu().tolist())
    return lo | hi << 32


def test_the_draw_is_the_definition(pkg, record):
    from istvt_amd import clips, ops
    first = 2 ** 32 - 2
    plan = small_plan(clips, record).seek(first)
    host, parts = plan.block_host()
    plan.on('cuda')
    assert plan.step == first
    for i in range(3):                                             # 2^32 - 2, 2^32 - 1, 2^32: the carry
        draw = ops.batch_draw(plan)
        assert draw is plan.draw and _same(draw, clips.batch_draw_host(plan, first + i)), i
        assert int(draw.status) == 0 and _step_of(draw.drawn) == first + i
        host[clips.DRAW_STEP_WORD], host[clips.DRAW_STEP_WORD + 1] = clips._i32(first + i), clips._i32((first + i) >> 32)
        host = after_draw(clips, plan, host, parts, first + i)
        assert torch.equal(plan.block.cpu(), host), i                # every int of the block, the header included
    assert plan.step == 2 ** 32 + 1
    assert _same(ops.batch_draw(plan.seek(7)), clips.batch_draw_host(plan, 7)) and plan.step == 8
    # one clip of one frame; more clips than the workgroup has lanes; a stride
    for over, step in ((dict(B=1, T=1), 0), (dict(B=300), 2 ** 64 - 1), (dict(B=257, stride=2, videos=long_videos(record)), 3)):
        p = small_plan(clips, record, **over).seek(step).on('cuda')
        assert _same(ops.batch_draw(p), clips.batch_draw_host(p, step)), over
        assert int(p.draw.status) == 0 and p.step == (step + 1) % 2 ** 64
    off = small_plan(clips, record, jpeg=None, perturb_p=None).on('cuda')
    assert _same(ops.batch_draw(off), clips.batch_draw_host(off, 0)) and off.taps_dev is None


def test_the_block_outside_its_output_slices(pkg, record):
    """the draw block's guard band: sentinels between the parts and behind the block, the input tables, and a refused block"""
    from istvt_amd import clips, ops
    step, tail = 11, 64
    plan = small_plan(clips, record).seek(step)
    host, parts = plan.block_host(gap=5, fill=FILL)
    plan.on('cuda', gap=5, tail=tail, fill=FILL)
    assert plan.storage.numel() == host.numel() + tail and plan.block.data_ptr() == plan.storage.data_ptr()
    before = plan.block.cpu()
    assert torch.equal(before, host) and int((host == FILL).sum()) >= 130 + 10 * 5    # the six output parts, the gaps
    ops.batch_draw(plan)
    got = plan.storage.cpu()
    want = after_draw(clips, plan, host, parts, step)
    assert torch.equal(got[:host.numel()], want) and bool((got[host.numel():] == FILL).all())
    for name in ('videos', 'base', 'shapes', 'kinds'):
        off, length = parts[name]
        assert torch.equal(got[off:off + length], getattr(plan, name).reshape(-1)), name
    covered = torch.zeros(host.numel(), dtype=torch.bool)
    covered[:clips.DRAW_HEADER_INTS] = True
    for off, length in parts.values():
        covered[off:off + length] = True
    assert int((~covered).sum()) >= 9 * 5 and bool((got[:host.numel()][~covered] == FILL).all())
    # doctored headers: the refusal status, and every other int as it was -- the output slices at their sentinels
    fresh = small_plan(clips, record).seek(step).on('cuda', gap=5, tail=tail, fill=FILL)
    W = clips.DRAW_OFFSET_WORD
    moves = [(2, 6), (1, host.numel() + tail), (W + 4, host.numel() - 59), (W + 8, parts['perturb'][0] + 19), (W + 5, -1),
             (W + 1, 2 ** 31 - 8)]
    for word, value in moves:
        bad = host.clone()
        bad[word] = value
        fresh.block.copy_(bad)
        ops.batch_draw(fresh)
        got = fresh.storage.cpu()
        assert torch.equal(got[:host.numel()], refused(clips, bad, 1)), (word, value)
        assert bool((got[host.numel():] == FILL).all()) and fresh.step == step
        for name in TABLES:
            assert bool((getattr(fresh.draw, name) == FILL).all()), (word, name)
    bad = host.clone()
    bad[parts['videos'][0] + 10] = 13                             # video 3 = places [14, 27) of 26
    fresh.block.copy_(bad)
    ops.batch_draw(fresh)
    assert torch.equal(fresh.block.cpu(), refused(clips, bad, 2)) and bool((fresh.storage[host.numel():] == FILL).all())
    fresh.block.copy_(host)                                       # the block as it was is drawn again
    assert _same(ops.batch_draw(fresh), clips.batch_draw_host(fresh, step)) and int(fresh.draw.status) == 0
    # the scalars the entry itself refuses
    import ctypes
    from istvt_amd import _lib
    args = _lib.JpegDecodeArgs(images_host=fresh.block.data_ptr(), stream=None)
    entry = _lib.lib().istvt_batch_draw
    for B, T, ints in ((0, 3, host.numel()), (5, 0, host.numel()), (5, 3, clips.DRAW_HEADER_INTS + 14), (2 ** 20, 2 ** 10, 2 ** 31 - 1)):
        assert entry(ctypes.byref(args), B, T, ints) == -3
    assert entry(ctypes.byref(_lib.JpegDecodeArgs()), 5, 3, host.numel()) == -3
    torch.cuda.synchronize()
    assert fresh.step == step + 1


@pytest.fixture(scope='module')
def banked(pkg):
    """12 host-encoded files, places 0..4 of 24 x 40 and 5..11 of 17 x 33, place 7 emptied (no segments: status 5) ->
    (bank, the arguments of a plan over its two videos)"""
    from istvt_amd import clips
    files = [clips.jpeg_encode_host(_smooth(*((24, 40) if i < 5 else (17, 33)), 60 + i), 70 + 2 * i,
                                    restart_interval=(1, 'row', 0)[i % 3]) for i in range(12)]
    bank = clips.jpeg_bank(files)
    bank.images[7, 17] = 0
    assert (bank.Hmax, bank.Wmax) == (24, 40) and bank.n == 12
    base = [[0, 0, h, w] for h, w in bank.sizes]
    base[2], base[9] = [3, 5, 18, 30], [1, 2, 15, 20]
    return bank, dict(videos=[(0, 5, 0), (5, 7, 1)], T=3, B=6, base=torch.tensor(base, dtype=torch.int32), K=16, seed=77)


def _pick_step(clips, plan, want):
    """the first step whose batch satisfies `want` (searched with the definition, on the host)"""
    return next(s for s in range(500) if want(clips.batch_draw_host(plan, s)))


def test_decode_drawn(pkg, banked):
    from istvt_amd import clips, ops
    bank, args = banked
    plan = clips.BatchPlan(bank, **args)
    step = _pick_step(clips, plan, lambda d: 7 in d.index.tolist() and len(set(d.label.tolist())) == 2)
    plan.seek(step).on('cuda')
    d = clips.batch_draw_host(plan, step)
    frames, sizes, status, draw = ops.jpeg_decode_drawn_u8(bank, plan)
    want = ops.jpeg_decode_indexed_u8(bank, d.index)
    assert _same(draw, d) and tuple(frames.shape) == (18, 24, 40, 3)
    assert torch.equal(frames, want[0]) and torch.equal(sizes, want[1]) and torch.equal(status, want[2])
    st = status.cpu().tolist()
    assert [s == 5 for s in st] == [i == 7 for i in d.index.tolist()] and set(st) == {0, 5}
    assert {tuple(r) for r in sizes.cpu().tolist()} == {(24, 40), (17, 33), (0, 0)}
    other = clips.BatchPlan(bank.sizes[:11], [(0, 5, 0)], T=3, B=6).on('cuda')
    with pytest.raises(ValueError, match='built for a bank of 11 places, this one has 12'):
        ops.jpeg_decode_drawn_u8(bank, other)
    with pytest.raises(ValueError, match='the canvas must hold every image of the bank'):
        ops.jpeg_decode_drawn_u8(bank, plan, canvas=(23, 40))


def _chain(clips, ops, bank, plan, step):
    """the input side of a step as it was: the definition's host tables through the existing calls"""
    d = clips.batch_draw_host(plan, step)
    B, T = plan.B, plan.T
    frames, _, status = ops.jpeg_decode_indexed_u8(bank, d.index)
    u8 = ops.crop_resize_u8(frames, d.boxes, S)
    if plan.thr_jpeg:
        u8 = ops.jpeg_roundtrip_u8(u8, d.quality)
    u8 = u8.view(B, T, S, S, 3)
    if plan.thr_perturb:
        u8 = ops.perturb_u8(u8, d.perturb, plan.taps, plan.seed)
    return u8.cpu(), d.view, d.label, status.cpu()


def _mixed(d):
    """some clips recompressed and some not, some perturbed and some not, noise among the kinds"""
    q, k = d.quality.view(-1, 3)[:, 0], d.perturb[:, 0]
    return 0 < int((q > 0).sum()) < len(q) and 0 < int((k > 0).sum()) < len(k) and 4 in k.tolist()


@pytest.mark.parametrize('augment', [True, False], ids=['jpeg+perturb', 'plain'])
def test_draw_clips(pkg, banked, augment):
    from istvt_amd import clips, ops
    bank, args = banked
    plan = clips.BatchPlan(bank, **args) if augment else clips.BatchPlan(bank, jpeg=None, perturb=None, **args)
    step = _pick_step(clips, plan, _mixed) if augment else 5
    want = _chain(clips, ops, bank, plan, step)
    plan.seek(step).on('cuda')
    u8, view, label, status = ops.draw_clips(bank, plan, S)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (6, 3, S, S, 3)
    assert torch.equal(u8.cpu(), want[0]) and torch.equal(view.cpu(), want[1]) and torch.equal(label.cpu(), want[2])
    assert torch.equal(status.cpu(), want[3]) and plan.step == step + 1
    if augment:                                                    # the stages did something: not the plain crops
        plain = clips.BatchPlan(bank, jpeg=None, perturb=None, **args).seek(step).on('cuda')
        assert not torch.equal(ops.draw_clips(bank, plain, S)[0], u8)
    with pytest.raises(ValueError, match=r'boxes of at most 32 \(8 x the output side 4\)'):
        ops.draw_clips(bank, plan, 4)
    with pytest.raises(RuntimeError, match='out must be contiguous uint8'):
        ops.draw_clips(bank, plan, S, out=torch.empty((18, S, S, 3), dtype=torch.uint8, device='cuda'))


def test_captured_in_a_graph(pkg, banked):
    """draw_clips with out= captured on one stream: replay i holds the batch of step s + i, because the step is device state,
    and after seek(s) a replay gives step s again"""
    from istvt_amd import clips, ops
    bank, args = banked
    plan = clips.BatchPlan(bank, **args)
    s = _pick_step(clips, plan, _mixed)
    wants = [_chain(clips, ops, bank, plan, s + i) for i in range(3)]
    assert not torch.equal(wants[0][0], wants[1][0])
    plan.on('cuda')
    out = torch.zeros((6, 3, S, S, 3), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # warm-up off the default stream, as torch asks
        ops.draw_clips(bank, plan, S, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out.zero_()
    plan.seek(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        u8, view, label, status = ops.draw_clips(bank, plan, S, out=out)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0 and plan.step == s and u8.data_ptr() == out.data_ptr()      # captured, not run
    for i in list(range(3)) + [0]:
        if i == 0:
            plan.seek(s)
        graph.replay()
        torch.cuda.synchronize()
        got = (out.cpu(), view.cpu(), label.cpu(), status.cpu())
        assert all(torch.equal(g, w) for g, w in zip(got, wants[i])), i
        assert plan.step == s + i + 1


def test_the_checked_view(pkg, monkeypatch):
    """model(u8, view=device view, view_checked=True) against model(u8, view=host view): logits and the conv1 weight gradient
    bit for bit, and no validation on the host.  XceptionVidTr(num_frames=4, grid=6, depth=2) at S = 96, as
    test_train_bytes_gpu.py takes it."""
    from istvt_amd import clips
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    B, T, side = 3, 4, 96
    torch.manual_seed(5)
    model = XceptionVidTr(num_frames=T, grid=6, depth=2, compute_dtype=torch.bfloat16).cuda().train()
    conv1 = next(p for n, p in model.named_parameters() if n.endswith('xcep.model.conv1.weight'))
    u8 = torch.randint(0, 256, (B, T, side, side, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).cuda()
    host = torch.tensor([[0, 0, 1], [0, 0, 0], [0, 0, 1]], dtype=torch.int32)
    results = []
    for checked in (False, True):
        model.zero_grad(set_to_none=True)
        if checked:
            monkeypatch.setattr(clips, 'check_views', lambda *a, **k: (_ for _ in ()).throw(AssertionError('validated on the host')))
        logits = model(u8, view=host.cuda(), crop=side, view_checked=True) if checked else model(u8, view=host, crop=side)
        logits.float().sum().backward()
        results.append((logits.detach().clone(), conv1.grad.detach().clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert float(results[0][1].abs().max()) > 0 and bool(torch.isfinite(results[0][0]).all())
    flipped = model(u8, view=torch.zeros((B, 3), dtype=torch.int32, device='cuda'), crop=side, view_checked=True)
    assert not torch.equal(flipped, results[0][0])                 # the view is read, not ignored
    for bad in (host, host.cuda().long(), host.cuda()[:2], host.cuda().view(-1), None):
        with pytest.raises(RuntimeError, match=r'a checked view is int32 \(3, 3\) on cuda'):
            model(u8, view=bad, crop=side, view_checked=True)
    with pytest.raises(AssertionError, match='validated on the host'):          # without the keyword the call is what it was
        model(u8, view=host, crop=side)
    with pytest.raises(RuntimeError, match='view / crop apply to uint8 clips'):
        model(torch.zeros((B, T, 3, side, side), device='cuda'), view_checked=True)
