"""frames.py without a device: ops re-exports its entries, crop_frames and paste_maps reach the entry that video.py and
explain.py reached through their own branches, with the arguments those branches passed."""
import types

import pytest
import torch


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


ENTRIES = ('crop_resize_u8', 'crop_resize_nv12', 'nv12_to_rgb_u8', 'warp_similarity_u8', 'warp_similarity_nv12',
           'relevance_paste_u8', 'relevance_paste_nv12', 'jpeg_roundtrip_u8', 'perturb_u8')


@pytest.fixture
def spies(pkg, monkeypatch):
    """every entry of frames.py replaced by a recorder -> the list of (name, args, kwargs)"""
    from istvt_amd import frames
    calls = []
    for name in ENTRIES:
        monkeypatch.setattr(frames, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)) or a[0])
    return calls


def test_ops_reexports_the_entries(pkg):
    from istvt_amd import frames, ops
    for name in ENTRIES:
        assert getattr(ops, name) is getattr(frames, name), name
        assert getattr(frames, name).__doc__
    assert max(len(line) for line in frames.jpeg_roundtrip_u8.__doc__.splitlines()) <= 128


def test_crop_frames_reaches_the_entry_of_every_pair(spies):
    """what VideoScorer._frame_batch chose: the NV12 twins take the matrix, the RGB ones do not; out and checked by keyword"""
    from istvt_amd import frames
    x, table, out = object(), object(), object()
    want = {('rgb24', False): 'crop_resize_u8', ('nv12', False): 'crop_resize_nv12',
            ('rgb24', True): 'warp_similarity_u8', ('nv12', True): 'warp_similarity_nv12'}
    for (fmt, aligned), name in want.items():
        del spies[:]
        frames.crop_frames(fmt, aligned, x, table, 7, 'bt601', out=out, checked=True)
        args = (x, table, 7, 'bt601') if fmt == 'nv12' else (x, table, 7)
        assert spies == [(name, args, {'out': out, 'checked': True})]


def test_frame_batch_crops_through_the_dispatcher(spies, monkeypatch):
    from istvt_amd import video
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda t: t)
    vid = torch.zeros((5, 12, 8), dtype=torch.uint8)
    tables = [torch.zeros((5, 4), dtype=torch.int32)]
    for fmt, aligned, name in (('nv12', True, 'warp_similarity_nv12'), ('rgb24', False, 'crop_resize_u8')):
        del spies[:]
        scorer = types.SimpleNamespace(pixel_format=fmt, yuv_matrix='jfif')
        batch = video.VideoScorer._frame_batch(scorer, [vid], [(0, 1, 3), (0, 4, 5)], tables, 4, 'cpu', aligned)
        assert tuple(batch.shape) == (3, 4, 4, 3) and [c[0] for c in spies] == [name, name]
        (_, a, kw), (_, a2, kw2) = spies
        assert torch.equal(a[0], vid[1:3]) and a[1].data_ptr() == tables[0][1:3].data_ptr() and a[2] == 4
        assert a[3:] == (('jfif',) if fmt == 'nv12' else ())
        assert kw['checked'] is True and kw['out'].data_ptr() == batch[0:2].data_ptr() and tuple(kw['out'].shape) == (2, 4, 4, 3)
        assert kw2['out'].data_ptr() == batch[2:3].data_ptr() and tuple(a2[0].shape) == (1, 12, 8)


def test_both_paste_call_sites_pass_what_they_passed(spies, monkeypatch):
    from istvt_amd import clips, explain, video
    from istvt_amd.network.vivit.vivit import XceptionVidTr
    S = 4
    boxes = torch.tensor([[0, 0, 8, 8], [2, 2, 4, 6]], dtype=torch.int32)
    maps = torch.randn((2, 2, 2), generator=torch.Generator().manual_seed(1))
    rgb, nv = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 12, 8), dtype=torch.uint8)
    lut = explain.jet_lut()
    # explain.overlay_frames: the frames themselves, the maps, the geometry of the boxes, the table in the frames' space
    for fmt, frames, name in (('rgb24', rgb, 'relevance_paste_u8'), ('nv12', nv, 'relevance_paste_nv12')):
        del spies[:]
        explain.overlay_frames(frames, maps, boxes=boxes, side=S, alpha=0.25, lut=lut, pixel_format=fmt, yuv_matrix='bt601',
                               inplace=True)
        A, rect = clips.paste_geometry(2, 8, 8, S, boxes=boxes, even=fmt == 'nv12')
        (got, a, kw), = spies
        assert got == name and kw == {'inplace': True, 'checked': True} and len(a) == 7
        assert a[0] is frames and a[1] is maps and torch.equal(a[2], A) and torch.equal(a[3], rect)
        assert torch.equal(a[4], clips.lut_to_ycc(lut, 'bt601') if fmt == 'nv12' else lut) and a[5] == 0.25 and a[6] == S
    # VideoScorer.render_explanation: frame_batch frames at a time, in place in its own copy, per-frame alpha on the device
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda t: t)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    model = XceptionVidTr(num_frames=4, grid=6, depth=1)
    ex = video.VideoExplanation(None, None, maps.reshape(2, -1), maps.reshape(2, -1), torch.ones(2), torch.zeros(2),
                                torch.ones(2, dtype=torch.int32))
    for fmt, frames, name in (('rgb24', rgb, 'relevance_paste_u8'), ('nv12', nv, 'relevance_paste_nv12')):
        del spies[:]
        scorer = video.VideoScorer(model, side=S, frame_batch=1, pixel_format=fmt)
        monkeypatch.setattr(scorer, '_device', lambda: torch.device('cpu'))
        out = scorer.render_explanation(frames, ex, boxes=boxes, alpha=0.5, weight_frames=False)
        A, rect = clips.paste_geometry(2, 8, 8, S, boxes=boxes, even=fmt == 'nv12')
        assert [c[0] for c in spies] == [name, name]
        for i, (_, a, kw) in enumerate(spies):
            assert kw == {'inplace': True, 'checked': True} and len(a) == 7
            assert a[0].data_ptr() == out[i:i + 1].data_ptr() and tuple(a[0].shape) == (1,) + tuple(frames.shape[1:])
            assert torch.equal(a[1], ex.frame_s[i:i + 1]) and torch.equal(a[2], A[i:i + 1]) and torch.equal(a[3], rect[i:i + 1])
            assert tuple(a[4].shape) == (256, 3) and torch.equal(a[5], torch.full((1,), 0.5)) and a[6] == S
