"""Per-kernel parity on a real MI355X: HIP kernels (via the C ABI) vs fp64 restatements."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _checks():
    import gpu_checks
    return gpu_checks.all_checks()


def _device_and_checks():
    """the `needs-gpu` case on a GPU: the device is a gfx950 and the per-kernel checks are there, each name once"""
    arch = torch.cuda.get_device_properties(0).gcnArchName
    assert arch.split(':')[0] == 'gfx950', arch
    names = [c[0] for c in _checks()]
    assert names and len(set(names)) == len(names), names
    return 0.0, 0.0


def pytest_generate_tests(metafunc):
    # `needs-gpu` is collected with and without a GPU: it skips without one and checks the device with one
    if 'check' in metafunc.fixturenames:
        if torch.cuda.is_available():
            cs = _checks()
            metafunc.parametrize('check', [_device_and_checks] + [c[1] for c in cs],
                                 ids=['needs-gpu'] + [c[0] for c in cs])
        else:
            metafunc.parametrize('check', [None], ids=['needs-gpu'])


def test_kernel(check):
    if check is None:
        pytest.skip('no GPU')
    err, tol = check()
    assert err <= tol, 'error %.3e > tolerance %.1e' % (err, tol)
