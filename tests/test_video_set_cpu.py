"""Scoring a set of videos (DESIGN.md "Scoring a set of videos"), the host side: SetPlan replayed on its own tables, the
input checks of score_videos, and the float64 restatements of the two reductions against brute force.  No device and no
kernel runs here; the two new entry points are only looked up in the built library."""
import math

import pytest
import torch

T = 4
COUNTS = ([4], [4, 4, 4], [4, 5, 9, 13], [11, 4, 30])


@pytest.fixture(scope='module')
def video():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import video
    return video


def _replay(video, counts, stride, cover_tail, frame_batch, window_batch, capacity):
    """Run the plan on a bank of frame numbers.  -> the plan"""
    plan = video.SetPlan(counts, T, stride, cover_tail, frame_batch, window_batch, capacity)
    cap = plan.capacity
    assert cap == (capacity if capacity is not None else -(-(frame_batch + window_batch * T) // 8) * 8)
    foff = [sum(counts[:v]) for v in range(len(counts) + 1)]
    G = foff[-1]
    want = [(v, s) for v, n in enumerate(counts) for s in video.window_starts(n, T, stride, cover_tail)]
    W = len(want)
    assert plan.window_video == [v for v, _ in want] and plan.starts == [s for _, s in want]
    assert plan.frame_offsets == foff
    assert plan.offsets == [sum(1 for v, _ in want if v < u) for u in range(len(counts) + 1)]
    readers = [0] * G                      # windows still to run that read the frame
    for v, s in want:
        for t in range(T):
            readers[foff[v] + s + t] += 1
    bank = [None] * cap                    # the frame every slot holds
    g = wi = 0
    wsteps = [i for i, st in enumerate(plan.steps) if st.kind == 'windows']
    for i, st in enumerate(plan.steps):
        if st.kind == 'frames':
            assert st.first == g and 1 <= st.count <= frame_batch and len(st.slots) == st.count
            assert len(set(st.slots)) == st.count and all(0 <= s < plan.slots_used <= cap for s in st.slots)
            for k, s in enumerate(st.slots):
                # no slot is overwritten while a window that has not run yet reads the frame in it
                assert bank[s] is None or readers[bank[s]] == 0, (counts, stride, i, s, bank[s])
                bank[s] = g + k
            g += st.count
            pieces = plan.pieces(st.first, st.count)
            assert [foff[v] + f for v, lo, hi in pieces for f in range(lo, hi)] == list(range(st.first, g))
            assert all(0 <= lo < hi <= counts[v] for v, lo, hi in pieces)
        else:
            assert st.kind == 'windows' and st.first == wi and 1 <= st.count <= window_batch
            assert st.idx.dtype == torch.int32 and tuple(st.idx.shape) == (st.count, T) and len(st.starts) == st.count
            if st.count < window_batch and i != wsteps[-1]:
                # a partial batch that is not the last one: only because the next frame batch had no room without it
                nxt = plan.steps[i + 1]
                room = sum(1 for f in bank if f is None or readers[f] == 0)
                assert capacity is not None, 'the default capacity never cuts a batch'
                assert nxt.kind == 'frames' and room < nxt.count, (counts, stride, i, room, nxt.count)
            for k in range(st.count):
                v, s = want[wi]
                assert st.starts[k] == s
                for t in range(T):
                    f = foff[v] + s + t
                    assert f < g and bank[int(st.idx[k, t])] == f, (counts, stride, i, k, t)
                    readers[f] -= 1
                wi += 1
    assert g == G and wi == W and not any(readers)
    assert plan.full_batches + plan.partial_batches == len(wsteps)
    assert plan.full_batches == sum(1 for i in wsteps if plan.steps[i].count == window_batch)
    return plan


@pytest.mark.parametrize('default_capacity', [False, True], ids=['min', 'default'])
@pytest.mark.parametrize('counts', COUNTS, ids=lambda c: '-'.join(str(n) for n in c))
def test_set_plan_replay(video, counts, default_capacity):
    for stride in (1, 3, 5):
        for frame_batch in (3, 5):
            for window_batch in (2, 3):
                for tail in (True, False):
                    cap = None if default_capacity else frame_batch + T
                    plan = _replay(video, counts, stride, tail, frame_batch, window_batch, cap)
                    if default_capacity:
                        assert plan.partial_batches <= 1
                        assert all(st.count == window_batch for st in plan.steps[:-1] if st.kind == 'windows')


def test_set_plan_crosses_videos_and_reuses_slots(video):
    """the GPU test's plan (a): frame batches straddle video boundaries, window batches mix videos, slots are reused"""
    plan = _replay(video, [4, 5, 9, 13], 3, True, 5, 3, 9)
    assert any(len(plan.pieces(st.first, st.count)) > 1 for st in plan.steps if st.kind == 'frames')
    assert plan.slots_used <= 9 < sum([4, 5, 9, 13]) and plan.partial_batches > 1
    # with room in the bank (the default capacity) the window batches are full and mix the windows of several videos
    plan = _replay(video, [4, 5, 9, 13], 3, True, 5, 3, None)
    assert any(len({plan.window_video[w] for w in range(st.first, st.first + st.count)}) > 1
               for st in plan.steps if st.kind == 'windows')
    assert plan.partial_batches == 1 and plan.full_batches == 3          # 10 windows


def test_set_plan_errors(video):
    with pytest.raises(ValueError, match='video 2 has 3 frames'):
        video.SetPlan([4, 9, 3, 8], T)
    with pytest.raises(ValueError, match='too small'):
        video.SetPlan([4, 9], T, frame_batch=5, capacity=5 + T - 1)
    with pytest.raises(ValueError):
        video.SetPlan([], T)
    with pytest.raises(ValueError):
        video.SetPlan([4], T, stride=0)
    video.SetPlan([4, 9], T, frame_batch=5, capacity=5 + T)


def test_score_videos_refuses_bad_sets_before_any_launch(video):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=T, grid=6, depth=1)              # on the host: nothing may be launched
    scorer = video.VideoScorer(model)
    u8 = torch.zeros((5, 96, 96, 3), dtype=torch.uint8)
    f32 = torch.zeros((5, 3, 96, 96))
    with pytest.raises(ValueError, match='all uint8 or all float'):
        scorer.score_videos([u8, f32])
    with pytest.raises(ValueError, match='one crop side'):
        scorer.score_videos([u8, torch.zeros((5, 64, 64, 3), dtype=torch.uint8)])
    with pytest.raises(ValueError, match='video 1 has 3 frames'):
        scorer.score_videos([u8, u8[:3]])
    with pytest.raises(ValueError):
        scorer.score_videos([])
    with pytest.raises(ValueError):
        scorer.score_videos(u8)
    with pytest.raises(ValueError, match='labels'):
        scorer.score_videos([u8, u8], labels=[1])
    with pytest.raises(ValueError, match='too small'):
        video.VideoScorer(model, frame_batch=8, capacity=8 + T - 1).score_videos([u8])
    with pytest.raises(ValueError, match='one table per video'):
        video.VideoScorer(model, side=96).score_videos([u8, u8], boxes=[torch.zeros((5, 4), dtype=torch.int32)])
    with pytest.raises(RuntimeError, match='ROCm device'):
        scorer.score_videos([u8, u8])                                  # a valid set: only the missing device stops it
    assert callable(XceptionVidTr.score_videos)


def test_score_videos_refuses_bad_labels_before_any_launch(video):
    """label values are checked where their shape is: on the host, before the device is asked for"""
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    scorer = video.VideoScorer(XceptionVidTr(num_frames=T, grid=6, depth=1))     # on the host: nothing may be launched
    u8 = torch.zeros((5, 96, 96, 3), dtype=torch.uint8)
    for labels in ([0, 2], torch.tensor([0, 2])):
        with pytest.raises(ValueError, match='0 or 1'):                          # not the RuntimeError about the ROCm device
            scorer.score_videos([u8, u8], labels=labels)


def test_entry_points_declared_and_exported(video):
    from istvt_amd import ops                               # (header, table and library: test_abi_cpu.py)
    assert callable(ops.windows_reduce) and callable(ops.auc_pairs)
    assert video.VideoSetScore._fields == ('window_logits', 'window_video', 'starts', 'offsets', 'logit_mean', 'prob_mean',
                                           'metrics')


def test_window_offsets_checked(video):
    from istvt_amd import ops
    assert ops.check_window_offsets([0, 1, 2, 70, 71, 400], 400) == [0, 1, 2, 70, 71, 400]
    assert ops.check_window_offsets(torch.tensor([0, 3], dtype=torch.int32), 3) == [0, 3]
    for bad in ([0], [1, 400], [0, 399], [0, 5, 5, 400], [0, 7, 3, 400], []):
        with pytest.raises(ValueError):
            ops.check_window_offsets(bad, 400)


def test_reduce_restatement_vs_brute_force(video):
    g = torch.Generator().manual_seed(3)
    off = [0, 1, 2, 70, 71, 400]
    for nc in (1, 3):
        x = (torch.rand((400, nc), generator=g) * 60 - 30).float()
        lm, pm = video.windows_reduce_ref(x, off)
        assert lm.dtype == pm.dtype == torch.float64 and tuple(lm.shape) == tuple(pm.shape) == (5, nc)
        for v, (a, b) in enumerate(zip(off, off[1:])):
            for c in range(nc):
                vals = [float(x[w, c]) for w in range(a, b)]
                assert abs(float(lm[v, c]) - math.fsum(vals) / (b - a)) <= 1e-13 * 30
                assert abs(float(pm[v, c]) - math.fsum(1.0 / (1.0 + math.exp(-u)) for u in vals) / (b - a)) <= 1e-13


def _brute_metrics(scores, labels, threshold=0.0):
    s = [float(v) for v in scores]
    lab = [int(v) for v in labels]
    pos = [i for i, l in enumerate(lab) if l == 1]
    neg = [i for i, l in enumerate(lab) if l == 0]
    fin = [math.isfinite(v) for v in s]
    greater = sum(1 for p in pos for n in neg if fin[p] and fin[n] and s[p] > s[n])
    equal = sum(1 for p in pos for n in neg if fin[p] and fin[n] and s[p] == s[n])
    auc = (greater + 0.5 * equal) / (len(pos) * len(neg)) if pos and neg else float('nan')
    correct = sum(1 for i, v in enumerate(s) if fin[i] and (v > threshold) == (lab[i] == 1))
    return dict(correct=correct, positives=len(pos), negatives=len(neg), nonfinite=fin.count(False), auc=auc, greater=greater,
                equal=equal)


def metric_cases():
    """(name, scores float32, labels int64): heavy ties, all scores equal, one empty class, a NaN and an infinity"""
    g = torch.Generator().manual_seed(7)
    out = []
    for V in (1, 2, 257, 1000):
        ties = torch.randint(0, 8, (V,), generator=g).float()
        lab = torch.randint(0, 2, (V,), generator=g)
        if V > 1:
            lab[0], lab[1] = 1, 0
        out.append(('ties-%d' % V, ties, lab))
        out.append(('real-%d' % V, torch.randn((V,), generator=g), lab))
        out.append(('all-equal-%d' % V, torch.full((V,), 0.25), lab))
        out.append(('no-negatives-%d' % V, ties, torch.ones_like(lab)))
        out.append(('no-positives-%d' % V, ties, torch.zeros_like(lab)))
        nan = ties.clone()
        nan[V // 2] = float('nan')
        out.append(('nan-%d' % V, nan, lab))
        if V > 2:
            inf = torch.randn((V,), generator=g)
            inf[0], inf[1], inf[2] = float('inf'), float('-inf'), float('nan')
            out.append(('inf-%d' % V, inf, lab))
    return out


def same_metrics(a, b):
    for k in ('correct', 'positives', 'negatives', 'nonfinite', 'greater', 'equal'):
        assert int(a[k]) == int(b[k]), (k, int(a[k]), int(b[k]))
    x, y = float(a['auc']), float(b['auc'])
    assert (math.isnan(x) and math.isnan(y)) or x == y, (x, y)


def test_metrics_restatement_vs_brute_force(video):
    for name, s, lab in metric_cases():
        for thr in (0.0, 3.0):
            ref = video.set_metrics_ref(s, lab, thr)
            same_metrics(ref, _brute_metrics(s, lab, thr))
        if name.startswith('no-'):
            assert math.isnan(ref['auc'])
        if name.startswith('all-equal') and ref['positives'] and ref['negatives']:
            assert ref['auc'] == 0.5
    # a hand-checked case: positives 3, 1, 1; negatives 1, 0 -> greater 4 (3 > 1, 3 > 0, 1 > 0, 1 > 0), equal 2
    ref = video.set_metrics_ref([3., 1., 1., 1., 0.], [1, 1, 1, 0, 0])
    assert (ref['greater'], ref['equal'], ref['auc']) == (4, 2, 5.0 / 6.0)
