"""Video scoring (DESIGN.md "Video scoring"), the host side: the window plan, the ring schedule and the input checks.
No device and no kernel runs here."""
import pytest
import torch


@pytest.fixture(scope='module')
def video():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import video
    return video


def _brute_starts(n, T, stride, cover_tail):
    """every frame index tried as a start, kept when it is on the stride grid and the window fits; then the tail"""
    starts = [s for s in range(n) if s % stride == 0 and s + T <= n]
    if cover_tail and starts[-1] + T != n:
        starts.append(n - T)
    return starts


def test_window_starts_brute_force(video):
    for T in range(1, 10):
        for stride in range(1, 11):
            for n in range(T, 41):
                for tail in (False, True):
                    got = video.window_starts(n, T, stride, tail)
                    assert got == _brute_starts(n, T, stride, tail), (n, T, stride, tail)
                    assert all(0 <= s and s + T <= n for s in got)
                    assert all(a < b for a, b in zip(got, got[1:]))
                    assert got[0] == 0
                    if tail:
                        assert got[-1] + T == n


def test_window_starts_short_video(video):
    with pytest.raises(ValueError):
        video.window_starts(3, 4, 1)
    with pytest.raises(ValueError):
        video.window_starts(8, 4, 0)


def _simulate(video, T, stride, capacity, fb, wb, chunks, cover_tail=True):
    """Run a RingPlan on the index tables alone: `held[slot]` is the frame a slot holds.  Every window must find each of
    its frames in the slot its table names at the moment it runs -- a slot reused while a window still needed it fails here."""
    plan = video.RingPlan(T, stride, capacity, fb, wb)
    held, got = {}, []

    def run(steps):
        for st in steps:
            if st.kind == 'frames':
                assert 1 <= st.count <= fb and len(st.slots) == st.count
                for i, slot in enumerate(st.slots):
                    assert 0 <= slot < capacity
                    held[slot] = st.first + i
            else:
                assert st.kind == 'windows' and 1 <= st.count <= wb
                assert st.idx.dtype == torch.int32 and tuple(st.idx.shape) == (st.count, T)
                for w, s0 in enumerate(st.starts):
                    for t in range(T):
                        assert held.get(int(st.idx[w, t])) == s0 + t, (T, stride, capacity, fb, wb, chunks, s0, t)
                got.extend(st.starts)
    first = 0
    for k in chunks:
        before = len(got)
        run(plan.push(k))
        first += k
        # a push returns every window its frames complete
        assert got[before:] == [s for s in video.window_starts(max(first, T), T, stride, False)
                                if first >= T and s + T > first - k and s + T <= first]
    run(plan.flush(cover_tail))
    return got


@pytest.mark.parametrize('T,stride,fb,wb', [(4, 1, 5, 3), (8, 1, 8, 32), (8, 3, 16, 4), (6, 2, 7, 32), (3, 7, 4, 2),
                                            (8, 8, 64, 32)])
def test_ring_schedule_matches_whole_video(video, T, stride, fb, wb):
    n = 3 * (fb + 1) + 5
    want = video.window_starts(n, T, stride, True)
    default_cap = -(-(T + fb) // 8) * 8
    for capacity in (T + 1, T + fb, default_cap, n):
        for chunk in (1, 3, fb, fb + 1):
            got = _simulate(video, T, stride, capacity, fb, wb, [chunk] * (n // chunk) + ([n % chunk] if n % chunk else []))
            assert got == want, (capacity, chunk)
    # the whole video at once, as score() plans it: the tail window joins the last batch
    plan = video.RingPlan(T, stride, n, fb, wb)
    steps = plan.push(n, drain=False) + plan.flush(True)
    assert [s for st in steps if st.kind == 'windows' for s in st.starts] == want
    assert sum(st.count for st in steps if st.kind == 'frames') == n
    assert all(st.count == wb for st in steps[:-1] if st.kind == 'windows')
    # without the tail window
    assert _simulate(video, T, stride, T + fb, fb, wb, [n], cover_tail=False) == video.window_starts(n, T, stride, False)


def test_ring_refuses_what_it_cannot_hold(video):
    with pytest.raises(ValueError):
        video.RingPlan(8, 1, 7, 4, 4)
    plan = video.RingPlan(4, 1, 16, 4, 4)
    plan.push(3)
    with pytest.raises(ValueError):
        plan.flush()                                       # 3 frames, T = 4
    plan = video.RingPlan(4, 1, 16, 4, 4)
    plan.push(9)
    plan.flush()
    with pytest.raises(RuntimeError):
        plan.push(1)


def test_input_errors(video):
    assert video.check_frames(torch.zeros((5, 8, 8, 3), dtype=torch.uint8)) == 'u8'
    assert video.check_frames(torch.zeros((5, 3, 8, 8))) == 'f32'
    with pytest.raises(ValueError, match='rank'):
        video.check_frames(torch.zeros((2, 5, 3, 8, 8)))                       # float clips, not frames
    with pytest.raises(ValueError, match='channels-last'):
        video.check_frames(torch.zeros((5, 3, 8, 8), dtype=torch.uint8))       # uint8 NCHW
    with pytest.raises(ValueError):
        video.check_frames(torch.zeros((5, 8, 8, 3)))                          # float NHWC
    with pytest.raises(ValueError):
        video.check_frames(torch.zeros((5, 3, 8, 8), dtype=torch.float64))


@pytest.mark.parametrize('slots,runs', [((2, 3, 4, 5), 1),           # one consecutive run
                                        ((6, 7, 0, 1), 2),           # a ring of 8 slots wraps
                                        ((0, 3, 4), 2),              # scattered over a pool
                                        ((0, 1, 4, 5, 2), 3),
                                        ((5,), 1)])                  # a single slot
def test_slot_runs_cover_every_slot_once_and_in_order(video, slots, runs):
    got = video.slot_runs(slots)
    assert len(got) == runs and all(k >= 1 for _, k in got)
    assert tuple(s0 + i for s0, k in got for i in range(k)) == slots
    assert all(a + k != b for (a, k), (b, _) in zip(got, got[1:]))   # the runs are maximal


def test_scorer_checks_before_any_device_work(video):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    scorer = video.VideoScorer(model, stride=2)
    assert scorer.T == 4
    with pytest.raises(ValueError, match='shorter'):
        scorer.score(torch.zeros((3, 96, 96, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match='shorter'):
        model.score_video(torch.zeros((3, 96, 96, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match='rank'):
        scorer.score(torch.zeros((1, 8, 3, 96, 96)))
    with pytest.raises(ValueError, match='channels-last'):
        scorer.push(torch.zeros((8, 3, 96, 96), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='ROCm device'):
        scorer.score(torch.zeros((8, 96, 96, 3), dtype=torch.uint8))           # a model on the host: no fallback
    with pytest.raises(ValueError):
        video.VideoScorer(model, capacity=4)
    with pytest.raises(ValueError):
        video.VideoScorer(model, std=(0.5, 0.0, 0.5))
    with pytest.raises(TypeError):
        video.VideoScorer(torch.nn.Linear(2, 2))


def test_stem_inference_entry_refuses_training(video):
    """uint8 frames reach no backward: refused in train mode and with gradients enabled, before any launch"""
    from istvt_amd import stem
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    xcep = XceptionVidTr(num_frames=4, grid=6, depth=1).xcep.model
    u8 = torch.zeros((2, 96, 96, 3), dtype=torch.uint8)
    xcep.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match='eval mode'):
        stem.stem_forward(u8, xcep, torch.float32, (0.5,) * 3, (0.5,) * 3)
    xcep.eval()
    with pytest.raises(RuntimeError, match='no_grad'):
        stem.stem_forward(u8, xcep, torch.float32, (0.5,) * 3, (0.5,) * 3)
    with torch.no_grad(), pytest.raises(RuntimeError, match='mean and std'):
        stem.stem_forward(u8, xcep, torch.float32)
    with torch.no_grad(), pytest.raises(RuntimeError, match='already normalised'):
        stem.stem_forward(torch.zeros((2, 3, 96, 96)), xcep, torch.float32, (0.5,) * 3, (0.5,) * 3)
