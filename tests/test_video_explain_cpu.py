"""Explaining whole videos (DESIGN.md "Explaining whole videos"), the parts that need no device: which windows cover which
frame, the default colour table, and the validation of window starts."""
import pytest
import torch


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def coverage(starts, n, T):
    """C(n) for every frame: the windows (in ascending window order) with s_w <= n < s_w + T, and their count"""
    cover = [[w for w, s in enumerate(starts) if s <= f < s + T] for f in range(n)]
    return cover, [len(c) for c in cover]


def fuse_ref(r_s, r_t, logits, starts, n, index=0):
    """float64 restatement of the fusion: plain means over C(n) of cam_s, cam_t, r_t[w, 0, t + 1] and logits[w, index]"""
    r_s, r_t, logits = r_s.double().cpu(), r_t.double().cpu(), logits.double().cpu()
    W, F, P = r_s.shape
    T = F - 1
    cover, count = coverage(starts, n, T)
    frame_s, frame_t = torch.zeros((n, P - 1), dtype=torch.float64), torch.zeros((n, P - 1), dtype=torch.float64)
    weight, logit = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for f in range(n):
        for w in cover[f]:
            t = f - starts[w]
            frame_s[f] += r_s[w, t + 1, 1:]
            frame_t[f] += r_t[w, 1:, t + 1]
            weight[f] += r_t[w, 0, t + 1]
            logit[f] += logits[w, index]
        if cover[f]:
            for v in (frame_s, frame_t, weight, logit):
                v[f] /= len(cover[f])
    return frame_s, frame_t, weight, logit, torch.tensor(count, dtype=torch.int32)


T_COV = 4


@pytest.mark.parametrize('cover_tail', [True, False], ids=['tail', 'notail'])
@pytest.mark.parametrize('stride', [1, 3, T_COV, T_COV + 3])
@pytest.mark.parametrize('n', [T_COV, T_COV + 1, 11, 64])
def test_coverage_tables(pkg, n, stride, cover_tail):
    """C(n) and count derived from window_starts by interval arithmetic against the brute-force restatement; the fuse
    restatement's count agrees; stride > T leaves frames uncovered"""
    from istvt_amd import ops, video
    T = T_COV
    starts = video.window_starts(n, T, stride, cover_tail)
    assert ops.check_window_starts(starts, n, T) == starts
    cover, count = coverage(starts, n, T)
    # independent statement: frame f is covered by the regular windows k with k*stride in [f - T + 1, f] that fit, plus the
    # tail window when there is one
    regular = list(range(0, n - T + 1, stride))
    tail = [n - T] if cover_tail and regular[-1] != n - T else []
    for f in range(n):
        want = [k for k in range(len(regular)) if f - T + 1 <= k * stride <= f]
        if tail and tail[0] <= f:
            want.append(len(regular))
        assert cover[f] == want, (f, cover[f], want)
        assert count[f] == len(want)
        assert cover[f] == sorted(cover[f])
    assert sum(count) == len(starts) * T
    if stride <= T:
        assert min(count) >= 1 or not cover_tail
    if stride > T and n >= 2 * stride:
        assert 0 in count                                   # the gap between two windows
    if cover_tail:
        assert count[-1] >= 1
    g = torch.Generator().manual_seed(n * 10 + stride)
    W = len(starts)
    res = fuse_ref(torch.rand((W, T + 1, 5), generator=g), torch.rand((W, 5, T + 1), generator=g),
                   torch.rand((W, 1), generator=g), starts, n)
    assert res[4].tolist() == count
    for f in range(n):
        if count[f] == 0:
            assert all(float(v[f].abs().sum()) == 0.0 for v in res[:4])


def test_default_lut_is_the_closed_form(pkg):
    from istvt_amd import explain
    lut = explain.jet_lut()
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
    for col, c in enumerate((0.75, 0.5, 0.25)):
        for i in range(256):
            want = int(round(255 * min(max(1.5 - abs(4 * i / 255 - 4 * c), 0.0), 1.0)))
            assert int(lut[i, col]) == want, (i, col)
    assert lut[0].tolist() == [0, 0, 128] and lut[255].tolist() == [128, 0, 0]      # blue end, red end
    assert int(lut[:, 1].max()) == 255 and int(lut[:, 0].max()) == 255 and int(lut[:, 2].max()) == 255


def test_starts_validation(pkg):
    from istvt_amd import ops
    assert ops.check_window_starts(torch.tensor([0, 2, 7]), 11, 4) == [0, 2, 7]
    with pytest.raises(ValueError, match='ascend'):
        ops.check_window_starts([0, 3, 2], 11, 4)
    with pytest.raises(ValueError, match='start in'):
        ops.check_window_starts([0, 4, 8], 11, 4)            # 8 > 11 - 4
    with pytest.raises(ValueError, match='start in'):
        ops.check_window_starts([-1, 4], 11, 4)
    with pytest.raises(ValueError):
        ops.check_window_starts([], 11, 4)


def test_api_surface(pkg):
    from istvt_amd import explain, ops, video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    assert callable(video.VideoScorer.explain) and callable(XceptionVidTr.explain_video) and callable(explain.overlay)
    assert video.VideoExplanation._fields == ('score', 'windows', 'frame_s', 'frame_t', 'frame_weight', 'frame_logit', 'count')
    assert callable(ops.relevance_fuse_windows) and callable(ops.relevance_overlay_u8)


def test_explain_refuses_a_cpu_model_and_a_short_video(pkg):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    flags = [m.training for m in model.modules()]
    with pytest.raises(ValueError, match='shorter'):
        model.explain_video(torch.zeros((3, 96, 96, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='ROCm device'):
        model.explain_video(torch.zeros((5, 96, 96, 3), dtype=torch.uint8))
    assert [m.training for m in model.modules()] == flags and all(p.requires_grad for p in model.parameters())
    with pytest.raises(RuntimeError, match='ROCm device'):
        from istvt_amd import explain
        explain.overlay(torch.zeros((1, 96, 96, 3), dtype=torch.uint8), torch.zeros((1, 6, 6)))
