"""What ops.py (the launch wrappers) and weights.py (the parameter-derived copies) both stand on: dtype codes, the raw
stream handle, the row-strided activation layout and the cast launch.  Imports neither of them; ops re-exports every name
here, so the rest of the package and the tests keep saying ``ops.pad_ld`` / ``ops.empty_rows`` / ``ops.cast``."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import _lib

Tensor = torch.Tensor
_DT = {torch.float32: 0, torch.bfloat16: 1}


def dtype_code(t: Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError('istvt_amd supports float32 and bfloat16 activations, got %s' % t.dtype) from None


def _req(t: Tensor, name: str = 'tensor') -> Tensor:
    if not t.is_cuda:
        raise RuntimeError('istvt_amd: %s must be on a ROCm device (no CPU fallback exists for the ISTVT hot path)' % name)
    return t


def _c(t: Tensor) -> Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream() -> int:
    # the raw handle of torch's current stream; torch.cuda.current_stream() builds a Stream object through three
    # Python layers (10 us x ~1500 launches per step)
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


# ------------------------------------------------------------------------------------------
# Row-strided activations.  The GEMMs stage their operands with LDS-DMA, which is priced per cache
# line touched: a [M][728] bf16 tensor has 1456-byte rows, so every 128-byte piece of a row straddles
# two lines.  Transformer activations (and the bf16 operand copies of the weights) are therefore
# allocated with rows padded to a multiple of 64 elements and handed around as [M, D] VIEWS of the
# [M, ld] buffer; every kernel takes the row stride.  Pad columns are never read and never written.
# (No kernel writes them on purpose.  Both halves are checked: tests/gpu_checks.py feeds NaN pad columns, and its guarded_*
# entries run the kernels on outputs whose pad columns and surroundings hold a sentinel that must survive, tests/guard.py.)
ROW_ALIGN = 64


def _parse_pad_mod(spec: str) -> Tuple[int, int]:
    try:
        m, r = (int(v) for v in spec.split(','))
    except ValueError:
        raise ValueError("ISTVT_PAD_MOD must be 'm,r' (lines per row = r mod m), got %r" % (spec,)) from None
    if m < 1 or not 0 <= r < m:
        raise ValueError('ISTVT_PAD_MOD=%r: need m >= 1 and 0 <= r < m' % (spec,))
    return m, r


_PAD_MOD = _parse_pad_mod(os.environ.get('ISTVT_PAD_MOD', '2,1'))   # (m, r): 64-element units per row = r mod m


def pad_ld(n: int) -> int:
    q = (n + ROW_ALIGN - 1) // ROW_ALIGN
    m, r = _PAD_MOD
    return (q + ((r - q) % m)) * ROW_ALIGN


def empty_rows(M: int, D: int, dtype, device, pad: bool = True) -> Tensor:
    ld = pad_ld(D) if pad else D
    buf = torch.empty((M, ld), dtype=dtype, device=device)
    return buf if ld == D else buf[:, :D]


def zeros_rows(M: int, D: int, dtype, device, pad: bool = True) -> Tensor:
    ld = pad_ld(D) if pad else D
    buf = torch.zeros((M, ld), dtype=dtype, device=device)
    return buf if ld == D else buf[:, :D]


def rows(t: Tensor) -> Tuple[Tensor, int]:
    """(2-D view [M, D] with unit column stride, row stride in elements); copies only if the layout is not that."""
    t2 = t if t.dim() == 2 else t.reshape(-1, t.shape[-1])
    M, D = t2.shape
    if M == 1:
        return (t2 if t2.stride(1) == 1 else t2.contiguous()), D
    if t2.stride(1) != 1 or t2.stride(0) < D or t2.stride(0) % 8 != 0 or t2.data_ptr() % 16 != 0:
        t2 = t2.contiguous()
    return t2, t2.stride(0)


G256_MIN = 64          # smallest output edge routed to the 256x256 DMA GEMM (ISTVT_G256_MIN of include/istvt_hip.h)


def cast(t: Tensor, dtype: torch.dtype) -> Tensor:
    _req(t)
    if t.dtype == dtype:
        return t
    t = _c(t)
    out = torch.empty(t.shape, dtype=dtype, device=t.device)
    if t.numel():
        _lib.check(_lib.lib().istvt_cast(t.data_ptr(), dtype_code(t), out.data_ptr(), _DT[dtype], t.numel(), _stream()),
                   'istvt_cast')
    return out
