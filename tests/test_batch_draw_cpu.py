"""The batch draw (DESIGN.md "Batch draw") on the CPU: the properties of the definition clips.batch_draw_host over 200 steps of
one small plan, the pinned record tests/golden/B1_batch_draw.json, every refusal of clips.BatchPlan, the two new entry points
against the header, and csrc/batch_draw.h compiled for the host (tools/batch_draw_check.cpp, built plain) against vectors of
the definition, doctored blocks among them."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from make_batch_draw_golden import STEPS, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


@pytest.fixture(scope='module')
def record(golden_dir):
    with open(os.path.join(golden_dir, 'B1_batch_draw.json')) as fh:
        return json.load(fh)


def small_plan(clips, record, **over):
    """the plan of the record: V = 4 videos of 3, 4, 7 and 12 frames, T = 3, K = 16, ragged base boxes; `over` its arguments"""
    return build(clips, record['plan'], **over)


def long_videos(record):
    """the 7- and 12-frame videos: what a clip of T = 3 at stride 2 (5 frames) fits in"""
    return [v for v in record['plan']['videos'] if v[1] >= 5]


def after_draw(clips, plan, block, parts, step):
    """the draw block `block` (a host tensor whose step word holds `step`) as a draw leaves it, by the definition"""
    out = block.clone()
    d = clips.batch_draw_host(plan, step)
    for name in ('index', 'boxes', 'quality', 'view', 'perturb', 'label'):
        off, length = parts[name]
        out[off:off + length] = getattr(d, name).reshape(-1)
    nxt = (step + 1) & (2 ** 64 - 1)
    out[clips.DRAW_STEP_WORD], out[clips.DRAW_STEP_WORD + 1] = clips._i32(nxt), clips._i32(nxt >> 32)
    out[clips.DRAW_DRAWN_WORD], out[clips.DRAW_DRAWN_WORD + 1] = clips._i32(step), clips._i32(step >> 32)
    out[clips.DRAW_STATUS_WORD] = 0
    return out


def refused(clips, block, status):
    out = block.clone()
    out[clips.DRAW_STATUS_WORD] = status
    return out


def _within(count, n, p):
    """a count of n trials lies within five binomial standard deviations of n p"""
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize('stride', [1, 2])
def test_properties_of_the_definition(clips, record, stride):
    B, T, S, steps = 16, 3, 16, 200
    videos = record['plan']['videos'] if stride == 1 else long_videos(record)
    plan = small_plan(clips, record, B=B, stride=stride, videos=videos)
    V, K = len(videos), 16
    sizes = record['plan']['sizes']
    Hc, Wc = max(h for h, _ in sizes), max(w for _, w in sizes)
    assert plan.max_side <= 8 * S and (plan.Hmax, plan.Wmax) == (Hc, Wc)
    counts = dict(flip=0, jpeg=0, perturb=0, video=[0] * V, kind=[0] * 7)
    assert len(set(map(tuple, plan.shapes.tolist()))) == K == plan.shapes.shape[0]
    for s in range(steps):
        d = clips.batch_draw_host(plan, s)
        assert all(t.dtype == torch.int32 for t in (d.index, d.boxes, d.quality, d.view, d.perturb, d.label))
        index = d.index.view(B, T)
        for b in range(B):
            v = next(i for i, (first, count, _) in enumerate(videos) if first <= int(index[b, 0]) < first + count)
            first, count, label = videos[v]
            start = int(index[b, 0]) - first
            assert index[b].tolist() == [first + start + t * stride for t in range(T)] and start + (T - 1) * stride < count
            assert int(d.label[b]) == label
            counts['video'][v] += 1
        base = plan.base[d.index.long()]
        assert bool((d.boxes[:, 0] >= base[:, 0]).all()) and bool((d.boxes[:, 1] >= base[:, 1]).all())
        assert bool((d.boxes[:, 0] + d.boxes[:, 2] <= base[:, 0] + base[:, 2]).all())
        assert bool((d.boxes[:, 1] + d.boxes[:, 3] <= base[:, 1] + base[:, 3]).all())
        clips.check_boxes(d.boxes, B * T, Hc, Wc, S)
        for f in range(B * T):                                     # ... and inside the frame's own image, not the canvas alone
            h, w = sizes[int(d.index[f])]
            assert int(d.boxes[f, 0] + d.boxes[f, 2]) <= h and int(d.boxes[f, 1] + d.boxes[f, 3]) <= w
        clips.check_qualities(d.quality, B * T)
        clips.check_perturbations(d.perturb, B, plan.taps)
        clips.check_views(d.view, B, S, S, S)
        assert d.perturb[:, 3].tolist() == list(range(B))          # two clips of a batch differ in stream
        assert int(d.perturb[:, 2].max()) < 2 ** 30
        q = d.quality.view(B, T)
        assert bool((q == q[:, :1]).all()) and bool(((q[:, 0] == 0) | ((q[:, 0] >= 30) & (q[:, 0] <= 95))).all())
        counts['flip'] += int(d.view[:, 2].sum())
        counts['jpeg'] += int((q[:, 0] > 0).sum())
        counts['perturb'] += int((d.perturb[:, 0] > 0).sum())
        for kind in d.perturb[:, 0].tolist():
            counts['kind'][kind] += 1
    n = steps * B
    assert _within(counts['flip'], n, 0.5) and _within(counts['jpeg'], n, 0.5) and _within(counts['perturb'], n, 0.5)
    assert all(_within(c, n, 1.0 / V) for c in counts['video']), counts['video']
    assert all(_within(c, counts['perturb'], 1.0 / 6) for c in counts['kind'][1:]), counts['kind']
    # step s gives the same whatever was drawn before: the draw has no state
    again = clips.batch_draw_host(plan, 17)
    clips.batch_draw_host(plan, 3)
    for name in ('index', 'boxes', 'quality', 'view', 'perturb', 'label'):
        assert torch.equal(getattr(again, name), getattr(clips.batch_draw_host(plan, 17), name)), name
    assert not torch.equal(again.boxes, clips.batch_draw_host(plan, 18).boxes)


def test_every_shape_row_is_drawn_as_often(clips, record):
    """the marginal of the shape row, read off the word that draws it: u(w3, K) over 200 steps of 16 clips"""
    plan = small_plan(clips, record, B=16)
    K, n = 16, 200 * 16
    seen = [0] * K
    b = torch.arange(16, dtype=torch.int64)
    for s in range(200):
        w3 = clips.philox4x32_10((s, 0, b, 0), (plan.seed & 0xffffffff, plan.seed >> 32))[3]
        for k in ((w3 * K) >> 32).tolist():
            seen[k] += 1
    assert all(_within(c, n, 1.0 / K) for c in seen), seen
    # ... and that is the row the definition uses: a square whole-image base box gives (m rh, m rw) of that row back
    square = clips.BatchPlan([(64, 64)] * 8, [(0, 8, 1)], T=3, B=16, K=K, seed=plan.seed)
    for s in (0, 1, 199):
        w3 = clips.philox4x32_10((s, 0, b, 0), (plan.seed & 0xffffffff, plan.seed >> 32))[3]
        rows = square.shapes.long()[(w3 * K) >> 32]
        want = ((64 * rows + 32768) >> 16).clamp(1, 64).repeat_interleave(3, dim=0)
        assert torch.equal(clips.batch_draw_host(square, s).boxes[:, 2:].long(), want)


def test_never_and_always(clips, record):
    never = small_plan(clips, record, flip_p=0.0, jpeg=[0.0, 30, 95], perturb_p=0.0, B=16)
    always = small_plan(clips, record, flip_p=1.0, jpeg=[1.0, 40, 40], perturb_p=1.0, B=16)
    off = small_plan(clips, record, jpeg=None, perturb_p=None, B=16)
    assert (never.thr_flip, always.thr_flip, off.thr_jpeg, off.thr_perturb, off.kinds.numel()) == (0, 2 ** 32, 0, 0, 0)
    for s in list(range(40)) + [2 ** 32 - 1, 2 ** 64 - 1]:
        a, b, c = (clips.batch_draw_host(p, s) for p in (never, always, off))
        assert not bool(a.view.any()) and not bool(a.quality.any()) and not bool(a.perturb[:, :2].any())
        assert bool((b.view[:, 2] == 1).all()) and bool((b.quality == 40).all()) and bool((b.perturb[:, 0] > 0).all())
        assert not bool(c.quality.any()) and not bool(c.perturb[:, :2].any())
        assert torch.equal(a.index, b.index) and torch.equal(a.boxes, c.boxes)      # the other words are not touched


def test_the_pinned_record(clips, record):
    plan = small_plan(clips, record)
    assert plan.shapes.tolist() == record['shapes'] and plan.kinds.tolist() == record['kinds']
    assert sorted(int(s) for s in record['steps']) == sorted(STEPS) and 2 ** 32 - 1 in STEPS and 2 ** 32 in STEPS
    for s, want in record['steps'].items():
        d = clips.batch_draw_host(plan, int(s))
        for name, table in want.items():
            assert getattr(d, name).tolist() == table, (s, name)
    # the carry: step 2^32 is not step 0 again
    assert clips.batch_draw_host(plan, 2 ** 32).boxes.tolist() != clips.batch_draw_host(plan, 0).boxes.tolist()


def test_the_shape_bank(clips):
    shapes = clips.draw_shapes(1024)
    assert shapes.dtype == torch.int32 and tuple(shapes.shape) == (1024, 2)
    area = shapes[:, 0].double() * shapes[:, 1].double() / 65536.0 ** 2
    aspect = shapes[:, 1].double() / shapes[:, 0].double()
    assert 0.5 <= float(area.min()) < 0.501 and 0.999 < float(area.max()) <= 1.0
    assert 0.75 <= float(aspect.min()) < 0.7504 and 1.3328 < float(aspect.max()) <= 4 / 3 + 1e-4
    assert abs(float(area.mean()) - 0.75) < 1e-3 and abs(float(aspect.log().mean())) < 1e-3
    # random_boxes' formulas: the sides of area a and aspect r on a square of side m are m sqrt(a / r) and m sqrt(a r)
    one = clips.draw_shapes(1, scale=(0.64, 0.64), ratio=(1.0, 1.0))
    assert one.tolist() == [[round(0.8 * 65536), round(0.8 * 65536)]]


def test_refusals(clips, record):
    a = record['plan']
    sizes = [tuple(s) for s in a['sizes']]
    with pytest.raises(ValueError, match=r'video 0 has 3 frames, a clip of T=3 at stride 2 spans 5'):
        small_plan(clips, record, stride=2)
    with pytest.raises(ValueError, match=r'video 0 has 4 frames, a clip of T=5 at stride 1 spans 5'):
        small_plan(clips, record, T=5, videos=a['videos'][1:])
    base = [list(b) for b in a['base']]
    base[15] = [0, 4, 17, 30]                                     # 4 + 30 > 33
    with pytest.raises(IndexError, match=r'the base box \[0, 4, 17, 30\] of place 15 lies outside its 17 x 33 image'):
        small_plan(clips, record, base=base)
    base[15] = [0, 0, 0, 5]
    with pytest.raises(IndexError, match='of place 15 lies outside'):
        small_plan(clips, record, base=base)
    with pytest.raises(ValueError, match=r'base must be int32 \(26, 4\)'):
        clips.BatchPlan(sizes, a['videos'], T=3, B=5, base=torch.zeros((25, 4), dtype=torch.int32))
    for K in (0, -1, 1.5):
        with pytest.raises(ValueError, match='the shape bank needs 1 <= K'):
            small_plan(clips, record, K=K)
    for over in (dict(flip_p=1.5), dict(flip_p=-0.1), dict(jpeg=[2.0, 30, 95]), dict(perturb_p=-1.0), dict(flip_p=float('nan'))):
        with pytest.raises(ValueError, match=r'must be a probability in \[0, 1\]'):
            small_plan(clips, record, **over)
    with pytest.raises(ValueError, match=r'jpeg = \(p, lo, hi\) needs ints 1 <= lo <= hi <= 100, got lo=60 hi=50'):
        small_plan(clips, record, jpeg=[0.5, 60, 50])
    with pytest.raises(ValueError, match=r'the range of noise must be \(low, high\) with low <= high'):
        clips.BatchPlan(sizes, a['videos'], T=3, B=5, perturb=(0.5, ('noise',), {'noise': (9.0, 3.0)}))
    with pytest.raises(ValueError, match='perturbation: noise = 80.0 gives param'):          # perturbation()'s own refusal
        clips.BatchPlan(sizes, a['videos'], T=3, B=5, perturb=(0.5, ('noise',), {'noise': (2.0, 80.0)}))
    with pytest.raises(ValueError, match='the kinds of perturb must name some of'):
        clips.BatchPlan(sizes, a['videos'], T=3, B=5, perturb=(0.5, ('copy',), None))
    for seed in (-1, 2 ** 64, 1.0):
        with pytest.raises(ValueError, match=r'the seed must lie in \[0, 2\^64\)'):
            small_plan(clips, record, seed=seed)
    for videos in ([[20, 7, 0]], [[-1, 5, 0]], [[26, 3, 1]]):
        with pytest.raises(IndexError, match=r'video 0 = places \[-?\d+, \d+\) leaves the bank of 26 places'):
            small_plan(clips, record, videos=videos)
    with pytest.raises(ValueError, match=r'videos must be an integer table \(V, 3\)'):
        small_plan(clips, record, videos=[[0, 3]])
    for over in (dict(T=0), dict(B=0), dict(stride=0)):
        with pytest.raises(ValueError, match='must be an int >= 1'):
            small_plan(clips, record, **over)
    plan = small_plan(clips, record)
    for step in (-1, 2 ** 64):
        with pytest.raises(ValueError, match=r'the step must lie in \[0, 2\^64\)'):
            clips.batch_draw_host(plan, step)
        with pytest.raises(ValueError, match=r'the step must lie in \[0, 2\^64\)'):
            plan.seek(step)
    assert plan.seek(41).step == 41                               # on the host until the plan is uploaded
    # the front end: what is wrong with the arguments is said before a device is asked for
    from istvt_amd import ops
    with pytest.raises(TypeError, match='batch_draw expects a clips.BatchPlan'):
        ops.batch_draw(None)
    for call in (lambda: ops.batch_draw(plan), lambda: ops.draw_clips(None, plan, 16)):
        with pytest.raises(RuntimeError, match=r'upload it first, plan.on\(device\)'):
            call()
    with pytest.raises(TypeError, match='jpeg_decode_drawn_u8 expects a clips.JpegBank'):
        ops.jpeg_decode_drawn_u8(sizes, plan)


def test_block_layout(clips, record):
    plan = small_plan(clips, record).seek(2 ** 32 + 5)
    for gap in (0, 3):
        block, parts = plan.block_host(gap=gap, fill=FILL)
        head = block[:clips.DRAW_HEADER_INTS].tolist()
        assert head[0] == clips.DRAW_MAGIC and head[1] == block.numel() and head[2:9] == [5, 3, 1, 4, 26, 16, 6]
        assert head[clips.DRAW_STEP_WORD:clips.DRAW_STEP_WORD + 2] == [5, 1] and parts['index'] == (clips.DRAW_HEADER_INTS, 15)
        assert head[12:18] == [-2 ** 31, 0] * 3                    # 2^31 as a (low, high) pair of int32 words
        assert head[clips.DRAW_OFFSET_WORD:clips.DRAW_OFFSET_WORD + 9] == [parts[n][0] for n in clips.DRAW_PARTS]
        at = clips.DRAW_HEADER_INTS + 15
        covered = torch.zeros(block.numel(), dtype=torch.bool)
        covered[:at] = True
        for name in clips.DRAW_PARTS:                               # in order, apart, inside
            off, length = parts[name]
            assert off >= at + gap and off % 4 == 0 and off + length + gap <= block.numel()
            covered[off:off + length] = True
            at = off + length
        assert bool((block[~covered] == FILL).all()) and int((~covered).sum()) >= 9 * gap
        assert torch.equal(block[parts['base'][0]:parts['base'][0] + 104].view(26, 4), plan.base)


def test_entry_points_declared(clips):
    import abi_header as H
    from istvt_amd import _lib, frames, ops
    with open(os.path.join(ROOT, 'include', 'istvt_hip.h')) as fh:
        protos = H.prototypes(fh.read())
    assert protos['istvt_batch_draw'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'B'), ('int', 'T'), ('int', 'block_ints')]
    assert protos['istvt_jpeg_decode_drawn_u8'] == [('const istvt_jpeg_decode_args*', 'a'), ('int', 'B'), ('int', 'T'),
                                                    ('int', 'block_ints'), ('int', 'seg_max'), ('int', 'block_stride'),
                                                    ('int', 'Hmax'), ('int', 'Wmax')]
    I = ctypes.c_int
    assert _lib.SIGNATURES['istvt_batch_draw'] == [ctypes.POINTER(_lib.JpegDecodeArgs), I, I, I]
    assert _lib.SIGNATURES['istvt_jpeg_decode_drawn_u8'] == [ctypes.POINTER(_lib.JpegDecodeArgs)] + [I] * 7
    for name in ('istvt_batch_draw', 'istvt_jpeg_decode_drawn_u8'):
        assert ctypes.c_void_p not in _lib.SIGNATURES[name]
    assert ops.batch_draw is frames.batch_draw and ops.draw_clips is frames.draw_clips
    assert ops.jpeg_decode_drawn_u8 is frames.jpeg_decode_drawn_u8
    with open(os.path.join(os.path.dirname(frames.__file__), 'csrc', 'batch_draw.h')) as fh:
        text = fh.read()
    assert 'BD_HEADER_INTS = %d;' % clips.DRAW_HEADER_INTS in text and 'BD_MAGIC_VALUE = 0x%X;' % clips.DRAW_MAGIC in text
    assert 'BD_STEP = %d, BD_STATUS = %d,' % (clips.DRAW_STEP_WORD, clips.DRAW_STATUS_WORD) in text
    assert 'BD_DRAWN = %d, BD_OFF_VIDEOS = %d,' % (clips.DRAW_DRAWN_WORD, clips.DRAW_OFFSET_WORD) in text


def checker_cases(clips, record):
    """[(B, T, status expected, block before, block after)]: draws of the small plan and its variants, and refused blocks"""
    cases = []

    def add(plan, step, gap=0):
        block, parts = plan.seek(step).block_host(gap=gap, fill=FILL)
        cases.append((plan.B, plan.T, 0, block, after_draw(clips, plan, block, parts, step)))
        return block, parts

    block, parts = add(small_plan(clips, record), 2 ** 32 - 1, gap=3)
    add(small_plan(clips, record), 2 ** 32)
    add(small_plan(clips, record, stride=2, videos=long_videos(record)), 5, gap=1)
    add(small_plan(clips, record, B=1, T=1), 0)
    add(small_plan(clips, record, B=300), 2 ** 64 - 1)
    add(small_plan(clips, record, jpeg=None, perturb_p=None, flip_p=1.0), 9)
    W = clips.DRAW_OFFSET_WORD

    def doctored(word, value, status=1, B=5, T=3):
        bad = block.clone()
        bad[word] = value
        cases.append((B, T, status, bad, refused(clips, bad, status)))

    doctored(0, 0)                                                # the magic
    doctored(1, block.numel() + 1)                                # a longer block than the call's
    doctored(2, 6)                                                # B of the header is not the call's
    cases.append((3, 5, 1, block, refused(clips, block, 1)))      # ... nor the call's the header's
    doctored(4, 0)                                                # stride
    doctored(5, 0)                                                # V
    doctored(7, 0)                                                # K = 0
    doctored(8, 0)                                                # perturb on, no kinds
    doctored(13, 2)                                               # a threshold above 2^32
    doctored(10, 101)                                             # a quality above 100
    for i, name in enumerate(clips.DRAW_PARTS):
        off, length = parts[name]
        doctored(W + i, block.numel() - length + 1)               # one int past the block's end
        doctored(W + i, -4)
        doctored(W + i, 2 ** 31 - 4)
        prev = parts['index'] if i == 0 else parts[clips.DRAW_PARTS[i - 1]]
        doctored(W + i, prev[0] + prev[1] - 1)                    # one int into the part before it
    moved = block.clone()                                         # the last part ends with the block: fine, and drawn there
    moved[W + 8] = block.numel() - 5
    cases.append((5, 3, 0, moved, after_draw(clips, small_plan(clips, record), moved,
                                             dict(parts, label=(block.numel() - 5, 5)), 2 ** 32 - 1)))
    # a row of videos that leaves the base table, and one shorter than a clip: nothing is drawn
    v = parts['videos'][0]
    doctored(v + 3 * 3 + 1, 13, status=2)                         # places [14, 27) of 26
    doctored(v + 1, 2, status=2)
    doctored(v, -1, status=2)
    return cases


def test_the_checker_built_plain(clips, record, tmp_path):
    """tools/batch_draw_check.cpp without sanitizers (the sanitizer build is a hand run: DESIGN.md has it)"""
    from istvt_amd import build
    cases = checker_cases(clips, record)
    vectors = tmp_path / 'vectors.bin'
    with open(vectors, 'wb') as fh:
        fh.write(np.array([len(cases)], dtype='<i4').tobytes())
        for B, T, status, block, after in cases:
            assert block.numel() == after.numel()
            fh.write(np.array([B, T, block.numel(), status], dtype='<i4').tobytes())
            fh.write(block.numpy().astype('<i4').tobytes())
            fh.write(after.numpy().astype('<i4').tobytes())
    clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', 'clang++')
    assert os.path.exists(clang), clang
    exe = tmp_path / 'batch_draw_check'
    r = subprocess.run([clang, '-std=c++17', '-O2', '-I', os.path.join(ROOT, 'include'),
                        '-I', os.path.join(os.path.dirname(build.__file__), 'csrc'),
                        os.path.join(ROOT, 'tools', 'batch_draw_check.cpp'), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == 'ok' and len(lines) == 2, r.stdout + r.stderr
    drawn = sum(B for B, _, status, _, _ in cases if status == 0)
    assert lines[0] == 'draw: %d cases, %d clips, %d refused' % (len(cases), drawn, sum(1 for c in cases if c[2]))
    assert drawn >= 300 + 5 and sum(1 for c in cases if c[2]) >= 40
    # the check can fail: one word of an expected block changed
    B, T, status, block, after = cases[0]
    wrong = after.clone()
    wrong[clips.DRAW_HEADER_INTS + 1] += 1
    with open(vectors, 'wb') as fh:
        fh.write(np.array([1, B, T, block.numel(), status], dtype='<i4').tobytes())
        fh.write(block.numpy().astype('<i4').tobytes() + wrong.numpy().astype('<i4').tobytes())
    r = subprocess.run([str(exe), str(vectors)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and 'case 0: word %d is' % (clips.DRAW_HEADER_INTS + 1) in r.stderr
