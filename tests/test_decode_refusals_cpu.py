"""The file decoders' front end (frames.py: jpeg_decode_u8, png_decode_u8, jpeg_decode_indexed_u8, jpeg_decode_drawn_u8)
without a device: every refusal that comes before the device check, by exception type and whole message
(decode_refusal_cases.py has the table and says where its literals come from), and the device check itself."""
import pytest
import torch

import decode_refusal_cases as C


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def test_refusals_before_the_device_check(pkg):
    cases = C.host_cases()
    assert len({c[0] for c in cases}) == len(cases) == 17
    for name, fn, args, kw, kind, message in cases:
        assert C.outcome(fn, args, kw) == [kind, message], name


def test_valid_input_needs_a_device(pkg, monkeypatch):
    """with no device in sight (here: none reported) a call that is right in every other way says so"""
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    x = C.inputs()
    for (fn, message), batches in zip(C.NO_DEVICE, ((x.files, x.batch), (x.pngs, x.png_batch, x.png_bands_batch))):
        for batch in batches:
            assert C.outcome(fn, (batch,), {}) == ['RuntimeError', message], fn


def test_the_public_entries_are_the_front_ends(pkg):
    from istvt_amd import frames, ops
    for fn in ('jpeg_decode_u8', 'png_decode_u8', 'jpeg_decode_indexed_u8', 'jpeg_decode_drawn_u8', 'batch_draw', 'draw_clips',
               'decode_frames'):
        assert getattr(ops, fn) is getattr(frames, fn), fn
