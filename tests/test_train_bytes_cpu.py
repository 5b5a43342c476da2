"""Training from bytes (DESIGN.md "Training from bytes"), the host side: the view helpers of istvt_amd.clips and the input
checks.  No device and no kernel runs here."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def clips():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    return clips


def test_check_views(clips):
    ok = torch.tensor([[0, 0, 0], [2, 4, 1], [1, 3, 0]], dtype=torch.int32)            # 7 x 9 source, S = 5: y0 <= 2, x0 <= 4
    assert torch.equal(clips.check_views(ok, 3, 7, 9, 5), ok)
    assert clips.check_views(None, 3, 5, 5, 5) is None and clips.check_views(None, 3, 5, 5, None) is None
    with pytest.raises(TypeError):
        clips.check_views(ok.long(), 3, 7, 9, 5)                                       # wrong dtype
    with pytest.raises(TypeError):
        clips.check_views(ok.float(), 3, 7, 9, 5)
    with pytest.raises(ValueError):
        clips.check_views(ok, 4, 7, 9, 5)                                              # wrong shape: 3 rows for 4 entries
    with pytest.raises(ValueError):
        clips.check_views(ok[:, :2].contiguous(), 3, 7, 9, 5)
    with pytest.raises(ValueError):
        clips.check_views(ok.view(-1), 3, 7, 9, 5)
    for bad in ([3, 0, 0], [0, 5, 0], [-1, 0, 0], [0, -1, 0]):                         # one past the edge / negative
        v = ok.clone()
        v[1] = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(ValueError):
            clips.check_views(v, 3, 7, 9, 5)
    v = ok.clone()
    v[2, 2] = 2                                                                        # flip = 2
    with pytest.raises(ValueError):
        clips.check_views(v, 3, 7, 9, 5)
    with pytest.raises(ValueError):
        clips.check_views(ok, 3, 7, 9, None)                                           # a view without a crop side
    with pytest.raises(ValueError):
        clips.check_views(None, 3, 7, 9, 5)                                            # a crop without a view
    with pytest.raises(ValueError):
        clips.check_views(ok, 3, 7, 9, 8)                                              # S > Hs
    with pytest.raises(ValueError):
        clips.check_views(ok, 3, 7, 9, 2)                                              # S < 3


def test_to_float_against_numpy(clips):
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (4, 7, 9, 3), generator=g, dtype=torch.uint8)
    view = torch.tensor([[0, 0, 0], [2, 4, 1], [1, 3, 1], [2, 0, 0]], dtype=torch.int32)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    got = clips.to_float(u8, mean, std, view, 5)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, 5, 5) and got.is_contiguous()
    a = u8.numpy()
    want = np.empty((4, 3, 5, 5), dtype=np.float32)
    for f in range(4):
        y0, x0, flip = (int(q) for q in view[f])
        for y in range(5):
            for x in range(5):
                for c in range(3):
                    u = a[f, y0 + y, x0 + (4 - x if flip else x), c]
                    want[f, c, y, x] = (np.float32(u) / np.float32(255) - np.float32(mean[c])) / np.float32(std[c])
    assert np.array_equal(got.numpy(), want)
    # per-clip views on (B, T, Hs, Ws, 3): each clip's view for all of its frames
    clip = u8.view(2, 2, 7, 9, 3)
    got2 = clips.to_float(clip, mean, std, view[1:3].contiguous(), 5)
    per_frame = clips.per_frame_views(view[1:3].contiguous(), 2)
    assert torch.equal(per_frame, view[[1, 1, 2, 2]])
    assert torch.equal(got2.flatten(0, 1), clips.to_float(u8, mean, std, per_frame, 5))
    # no view: the whole (square) frame
    sq = u8[:, :7, :7].contiguous()
    assert torch.equal(clips.to_float(sq, mean, std), clips.to_float(sq, mean, std, torch.zeros((4, 3), dtype=torch.int32), 7))
    with pytest.raises(ValueError):
        clips.to_float(u8, mean, std)                                                  # 7 x 9 without a crop
    with pytest.raises(ValueError):
        clips.to_float(u8.float(), mean, std)


def test_random_views(clips):
    v = clips.random_views(500, 112, 120, 96, torch.Generator().manual_seed(7))
    assert v.dtype == torch.int32 and tuple(v.shape) == (500, 3) and v.is_contiguous() and not v.is_cuda
    clips.check_views(v, 500, 112, 120, 96)
    assert int(v[:, 0].min()) == 0 and int(v[:, 0].max()) == 16 and int(v[:, 1].min()) == 0 and int(v[:, 1].max()) == 24
    assert 0.35 < float(v[:, 2].float().mean()) < 0.65
    assert torch.equal(v, clips.random_views(500, 112, 120, 96, torch.Generator().manual_seed(7)))
    assert not torch.equal(v, clips.random_views(500, 112, 120, 96, torch.Generator().manual_seed(8)))
    assert int(clips.random_views(50, 112, 120, 96, torch.Generator().manual_seed(1), flip_p=0.0)[:, 2].sum()) == 0
    assert int(clips.random_views(50, 112, 120, 96, torch.Generator().manual_seed(1), flip_p=1.0)[:, 2].sum()) == 50
    assert torch.equal(clips.random_views(5, 96, 96, 96, torch.Generator().manual_seed(1), flip_p=0.0), torch.zeros((5, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        clips.random_views(4, 90, 120, 96)


def test_model_on_the_host_refuses_bytes(clips):
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    with pytest.raises(RuntimeError, match='ROCm device'):
        model(torch.zeros((2, 4, 96, 96, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='ROCm device'):
        model(torch.zeros((2, 4, 112, 120, 3), dtype=torch.uint8), view=clips.random_views(2, 112, 120, 96), crop=96)
    with pytest.raises(RuntimeError, match='view / crop'):
        model(torch.zeros((2, 4, 3, 96, 96)), view=clips.random_views(2, 112, 120, 96))
    with pytest.raises(ValueError):
        model.set_input_normalisation(std=(0.5, 0.0, 0.5))
    with pytest.raises(ValueError):
        model.set_input_normalisation(mean=(0.5, 0.5))
