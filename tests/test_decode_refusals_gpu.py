"""The file decoders' front end (frames.py) on the device, at the smallest inputs (decode_refusal_cases.py): the refusals that
need no device once more with one in sight; then, per entry, valid arguments with exactly one thing made wrong -- the canvas,
`out`, each of the caller's `buffers` -- by exception type and whole message, and two calls that are wrong twice, which pin
the order of the checks; and one passing call per entry with `out` and `buffers` given, which gives the clips.*_host definition
bit for bit and records the written name and byte count under ops.kernel_profile."""
import pytest
import torch

import decode_refusal_cases as C

DEVICE_CASES = C.device_cases()
assert len({c[0] for c in DEVICE_CASES}) == len(DEVICE_CASES)


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


@pytest.mark.gpu
def test_refusals_before_the_device_check_on_the_device(pkg):
    for name, fn, args, kw, kind, message in C.host_cases():
        assert C.outcome(fn, args, kw) == [kind, message], name


@pytest.mark.gpu
@pytest.mark.parametrize('case', DEVICE_CASES, ids=[c[0] for c in DEVICE_CASES])
def test_refusal_is_the_written_one(pkg, case):
    _, entry, fault, kind, message = case
    fn, args, kw = C.valid(entry, 'cuda')
    fault(kw, 'cuda')
    assert C.outcome(fn, args, kw) == [kind, message]


@pytest.mark.gpu
@pytest.mark.parametrize('entry', list(C.ENTRIES))
def test_passing_call_gives_the_definition_and_the_written_profile(pkg, entry):
    from istvt_amd import ops
    fn, args, kw = C.valid(entry, 'cuda')
    _, n, (Hc, Wc), _, name, nbytes = C.ENTRIES[entry]
    ops.kernel_profile = []
    try:
        got = getattr(ops, fn)(*args, **kw)
        rec = [[r[0], int(r[3])] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert rec == [[name, nbytes]]
    frames, sizes, status = got[:3]
    assert frames is kw['out'] and sizes is kw['buffers'][1] and status is kw['buffers'][2]
    assert status.cpu().tolist() == [0] * n
    want = C.definition(entry)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (n, Hc, Wc, 3) == tuple(want.shape)
    assert torch.equal(frames.cpu(), want)
    if entry.startswith('drawn'):
        assert got[3] is args[1].draw and got[3].index.cpu().tolist() == [0, 1] and got[3].status.cpu().tolist() == [0]
