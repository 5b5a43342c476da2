"""Perturbations (DESIGN.md "Perturbations") without a device: Philox known answers, the identities of the integer
definition clips.perturb_host, the taps, the blur against a float64 convolution, the noise statistics, per-clip tables, the
helpers and the validation."""
import math

import numpy as np
import pytest
import torch

SIGMAS = (0.5, 1.0, 2.0, 3.5)


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def _random(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _table(rows):
    return torch.tensor(rows, dtype=torch.int32)


def _philox_numpy(counter, key):
    """Philox4x32-10 restated with numpy's 64-bit unsigned products"""
    c = [np.uint64(v) for v in counter]
    k = [np.uint64(v) for v in key]
    lo32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & lo32, (k[1] + np.uint64(0xBB67AE85)) & lo32]
    return [int(v) for v in c]


def test_philox_known_answers(clips):
    """the published vectors of Philox4x32-10 (Random123's kat_vectors)"""
    cases = {(0,) * 6: (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8),
             (0xffffffff,) * 6: (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)}
    for words, want in cases.items():
        got = clips.philox4x32_10(words[:4], words[4:])
        assert tuple(int(w) for w in got) == want == tuple(_philox_numpy(words[:4], words[4:]))
    # tensors of counters, against the numpy restatement word by word
    c0 = torch.tensor([0, 1, 2, 0xfffffffe, 123456789], dtype=torch.int64)
    got = clips.philox4x32_10((c0, 7, 0x80000001, 0), (0xdeadbeef, 0x12345678))
    for i, v in enumerate(c0.tolist()):
        assert [int(w[i]) for w in got] == _philox_numpy((v, 7, 0x80000001, 0), (0xdeadbeef, 0x12345678))


def test_identities(clips):
    src = _random(2, 9, 11, 1)
    taps = clips.gaussian_taps(list(SIGMAS))
    for kind, p in ((0, 0), (0, 777), (1, 256), (2, 256), (3, 256)):
        assert torch.equal(clips.perturb_host(src, _table([[kind, p, 0, 0]] * 2)), src), (kind, p)
    flat = torch.empty((3, 9, 11, 3), dtype=torch.uint8)
    for c, v in enumerate((0, 93, 255)):
        flat[c] = v
    for row in range(len(SIGMAS)):
        assert torch.equal(clips.perturb_host(flat, _table([[5, row, 0, 0]] * 3), taps), flat)
    for k in (2, 3, 8, 32):
        assert torch.equal(clips.perturb_host(flat, _table([[6, k, 0, 0]] * 3)), flat)
    i32 = src.to(torch.int32)
    Y = (19595 * i32[..., 0] + 38470 * i32[..., 1] + 7471 * i32[..., 2] + 32768) >> 16
    grey = clips.perturb_host(src, _table([[3, 0, 0, 0]] * 2)).to(torch.int32)
    assert all(torch.equal(grey[..., c], Y) for c in range(3))                      # saturation 0: R = G = B = Y
    out = clips.perturb_host(src, _table([[2, 0, 0, 0]] * 2)).to(torch.int64)
    for f in range(2):                                                              # contrast 0: the frame's mean luma
        m = (int(Y[f].to(torch.int64).sum()) + 99 // 2) // 99
        assert bool((out[f] == m).all())
    for k in (11, 32):                                                              # one block: the rounded channel means
        out = clips.perturb_host(src, _table([[6, k, 0, 0]] * 2)).to(torch.int64)
        want = (src.to(torch.int64).sum((1, 2)) + 99 // 2) // 99
        assert bool((out == want[:, None, None, :]).all())


def test_gaussian_taps(clips):
    taps = clips.gaussian_taps(list(SIGMAS))
    assert taps.dtype == torch.int32 and tuple(taps.shape) == (4, 21)
    assert taps.sum(1).tolist() == [2048] * 4 and torch.equal(taps, taps.flip(1)) and bool((taps >= 0).all())
    assert (taps != 0).sum(1).tolist() == [5, 7, 13, 21]
    assert torch.equal(clips.gaussian_taps(2.0), taps[2:3])
    for bad in (0.29, 4.01):
        with pytest.raises(ValueError):
            clips.gaussian_taps([bad])
    with pytest.raises(ValueError):
        clips.gaussian_taps([1.0] * 17)
    clips.check_perturbations(_table([[5, 1, 0, 0]]), 1, clips.gaussian_taps([0.3, 4.0]))


def _blur_float64(img, sigma):
    """an independent separable convolution in float64: the same truncation (|i| <= min(10, ceil(3 sigma))), weights divided by
    their sum, edge replication; img (H, W, 3) -> float64 (H, W, 3), not rounded"""
    R = min(10, math.ceil(3 * sigma))
    w = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 / (2 * sigma * sigma))
    w /= w.sum()
    p = np.pad(img.astype(np.float64), ((R, R), (R, R), (0, 0)), mode='edge')
    h = sum(w[i] * p[:, i:i + img.shape[1]] for i in range(2 * R + 1))
    return sum(w[j] * h[j:j + img.shape[0]] for j in range(2 * R + 1))


@pytest.mark.parametrize('h,w', [(5, 7), (33, 70), (64, 64)])
def test_blur_against_float64(clips, h, w):
    """max |definition - float64 convolution| <= 1.0 grey level: one rounding (0.5) plus the quantisation of the taps"""
    src = _random(1, h, w, h * 100 + w)
    taps = clips.gaussian_taps(list(SIGMAS))
    assert 255 * int(taps.sum(1).max()) ** 2 < 2 ** 31                               # the int32 accumulator at its largest
    for row, sigma in enumerate(SIGMAS):
        got = clips.perturb_host(src, _table([[5, row, 0, 0]]), taps)[0].numpy().astype(np.float64)
        err = float(np.abs(got - _blur_float64(src[0].numpy(), sigma)).max())
        print('%d x %d sigma %.1f: max |definition - float64| = %.3f' % (h, w, sigma, err))
        assert err <= 1.0


def _noise(clips, fid, stream, seed, n=1):
    x = torch.full((n, 64, 64, 3), 128, dtype=torch.uint8)
    return clips.perturb_host(x, _table([[4, 160, fid, stream]] * n), seed=seed).to(torch.float64) - 128


def test_noise_statistics(clips):
    d = _noise(clips, 0, 0, 0)
    std, mean = float(d.std()), float(d.mean())
    print('noise at p = 160: std %.3f, mean %.3f' % (std, mean))
    assert abs(std - 10.0) <= 0.3 and abs(mean) <= 0.2
    two = _noise(clips, 5, 2, 9, n=2)
    assert torch.equal(two[0], two[1])                                              # same (frame_id, stream): same noise
    base = _noise(clips, 5, 2, 9)
    assert torch.equal(base[0], two[0])
    for fid, stream, seed in ((6, 2, 9), (5, 3, 9), (5, 2, 10), (5, 2, 9 + (1 << 32))):
        assert not torch.equal(_noise(clips, fid, stream, seed), base)
    assert torch.equal(clips.perturb_host(torch.full((1, 8, 8, 3), 77, dtype=torch.uint8), _table([[4, 0, 0, 0]])),
                       torch.full((1, 8, 8, 3), 77, dtype=torch.uint8))             # sigma 0
    hi = clips.perturb_host(_random(1, 16, 16, 3), _table([[4, 1023, 0, 0]]))        # the largest products stay in int32
    assert hi.dtype == torch.uint8


def test_per_clip_table(clips):
    src = _random(6, 12, 20, 4).view(2, 3, 12, 20, 3)
    taps = clips.gaussian_taps([1.0])
    for rows in ([[4, 200, 7, 1], [5, 0, 0, 0]], [[2, 400, 0, 0], [6, 3, 1, 1]]):
        got = clips.perturb_host(src, _table(rows), taps, seed=3)
        flat = _table([r[:2] + [r[2] + t, r[3]] for r in rows for t in range(3)])
        assert got.shape == src.shape
        assert torch.equal(got.view(6, 12, 20, 3), clips.perturb_host(src.view(6, 12, 20, 3), flat, taps, seed=3))


def test_validation(clips):
    ok = _table([[1, 100, 0, 0], [6, 2, 3, 4]])
    taps = clips.gaussian_taps([1.0, 2.0])
    assert torch.equal(clips.check_perturbations(ok, 2), ok)
    with pytest.raises(TypeError):
        clips.check_perturbations(ok.long(), 2)
    with pytest.raises(TypeError):
        clips.check_perturbations(ok.tolist(), 2)
    for bad in (ok[:1], ok[:, :3], ok.reshape(-1)):
        with pytest.raises(ValueError):
            clips.check_perturbations(bad.contiguous(), 2)
    rows = [[7, 0, 0, 0], [-1, 0, 0, 0], [1, 1025, 0, 0], [1, -1, 0, 0], [2, 1025, 0, 0], [3, -1, 0, 0], [3, 1025, 0, 0],
            [4, 1024, 0, 0], [4, -1, 0, 0], [6, 1, 0, 0], [6, 33, 0, 0], [1, 5, -1, 0], [1, 5, 0, -1]]
    for r in rows:
        with pytest.raises(ValueError):
            clips.check_perturbations(_table([r]), 1, taps)
    for r in ([1, 1024, 0, 0], [4, 1023, 0, 0], [6, 32, 0, 0], [0, -5, 0, 0], [5, 1, 0, 0]):
        clips.check_perturbations(_table([r]), 1, taps)
    with pytest.raises(ValueError):
        clips.check_perturbations(_table([[5, 0, 0, 0]]), 1)                        # blur without taps
    for r in ([5, 2, 0, 0], [5, -1, 0, 0]):
        with pytest.raises(ValueError):
            clips.check_perturbations(_table([r]), 1, taps)                         # not a row of the bank
    off = taps.clone()
    off[0, 10] += 1
    with pytest.raises(ValueError):
        clips.check_perturbations(ok, 2, off)                                       # 2049, even where no row blurs
    skew = taps.clone()
    skew[1, 9] += 1
    skew[1, 12] -= 1
    neg = taps.clone()
    neg[0, 0], neg[0, 20], neg[0, 10] = -1, -1, neg[0, 10] + 2
    for bad in (skew, neg, taps[:, :20].contiguous(), torch.cat([taps] * 9), taps.long()):
        with pytest.raises((ValueError, TypeError)):
            clips.check_perturbations(ok, 2, bad)
    with pytest.raises(ValueError):
        clips.perturb_host(_random(1, 4, 4, 0).float(), ok[:1])
    with pytest.raises(ValueError):
        clips.perturb_host(_random(1, 4, 4, 0), ok[:1], seed=-1)


def test_helpers(clips):
    assert clips.perturbation('saturation', 0.4) == (3, 102, None)
    assert clips.perturbation('noise', 10.0) == (4, 160, None)
    assert clips.perturbation('pixelate', 4) == (6, 4, None)
    assert clips.perturbation('brightness', 1.0)[:2] == (1, 256) and clips.perturbation('contrast', 4)[:2] == (2, 1024)
    kind, row, taps = clips.perturbation('blur', 2.0)
    assert (kind, row) == (5, 0) and torch.equal(taps, clips.gaussian_taps([2.0]))
    assert clips.perturbation('copy', None) == (0, 0, None)
    for name, value in (('hue', 1.0), ('noise', 64.0), ('noise', -1.0), ('pixelate', 1), ('pixelate', 4.0), ('blur', 5.0),
                        ('contrast', 4.01), ('saturation', float('nan')), ('brightness', '1')):
        with pytest.raises(ValueError):
            clips.perturbation(name, value)
    tab, taps = clips.perturbation_table(5, 'blur', 1.0, first_frame=3, stream=2)
    assert tab.tolist() == [[5, 0, 3 + i, 2] for i in range(5)] and torch.equal(taps, clips.gaussian_taps([1.0]))
    tab, taps = clips.perturbation_table(2, 'noise', 10.0)
    assert tab.tolist() == [[4, 160, 0, 0], [4, 160, 1, 0]] and taps is None
    assert set(clips.PERTURBATION_LEVELS) == set(clips.PERTURBATION_KINDS[1:])
    for name, levels in clips.PERTURBATION_LEVELS.items():
        assert len(levels) == 5
        for v in levels:
            tab, taps = clips.perturbation_table(1, name, v)
            clips.check_perturbations(tab, 1, taps)


def test_random_perturbations(clips):
    g = torch.Generator().manual_seed(5)
    tab, taps = clips.random_perturbations(400, p=0.5, generator=g)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (400, 4) and tuple(taps.shape) == (8, 21)
    clips.check_perturbations(tab, 400, taps)
    again, taps2 = clips.random_perturbations(400, p=0.5, generator=torch.Generator().manual_seed(5))
    assert torch.equal(tab, again) and torch.equal(taps, taps2)
    on = int((tab[:, 0] != 0).sum())
    assert 150 <= on <= 250 and set(tab[:, 0].tolist()) == set(range(7))             # 400 draws at p = 0.5: 200 +- 5 sigma
    assert tab[:, 3].tolist() == list(range(400)) and len(set(tab[:, 2].tolist())) > 390
    g = tab[tab[:, 0] == 1][:, 1]
    assert int(g.min()) >= 154 and int(g.max()) <= 358                              # 0.6 .. 1.4 in Q8
    only, _ = clips.random_perturbations(50, p=1.0, kinds=('pixelate',), pixelate=(3, 5), generator=torch.Generator().manual_seed(1))
    assert set(only[:, 0].tolist()) == {6} and set(only[:, 1].tolist()) == {3, 4, 5}
    none, _ = clips.random_perturbations(10, p=0.0)
    assert none[:, :2].abs().sum() == 0
    for kw in (dict(p=1.5), dict(kinds=('hue',)), dict(kinds=()), dict(noise=(2.0, 70.0)), dict(blur=(3.0, 1.0))):
        with pytest.raises(ValueError):
            clips.random_perturbations(4, **kw)
    with pytest.raises(ValueError):
        clips.random_perturbations(0)


def test_scorer_checks_the_keyword():
    """the constructor refuses a perturbation, and a call refuses float frames, before any device is touched"""
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    for bad in (('hue', 1.0), ('noise', 99.0), ('pixelate', 1), 'blur', ('blur',), ('blur', 2.0, 1)):
        with pytest.raises(ValueError):
            video.VideoScorer(model, perturb=bad)
    with pytest.raises(ValueError):
        video.VideoScorer(model, perturb=('noise', 10.0), perturb_seed=-1)
    scorer = video.VideoScorer(model, perturb=('blur', 2.0), perturb_seed=7)
    assert scorer.perturb[:2] == (5, 0) and scorer.perturb_seed == 7 and video.VideoScorer(model).perturb is None
    with pytest.raises(TypeError):
        scorer.score(torch.zeros((4, 3, 96, 96)))
    with pytest.raises(TypeError):
        model.score_video(torch.zeros((4, 3, 96, 96)), perturb=('noise', 10.0))
