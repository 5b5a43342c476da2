"""Tensor-level launch wrappers around the C ABI (include/istvt_hip.h).

Every function checks shapes/dtypes in Python *before* launching (so bad geometry raises a
Python exception like the reference does, SURVEY.md 8(b) "Error convention"), passes raw device
pointers + the current torch stream, and never synchronises.  Inputs must live on a ROCm
device: there is deliberately no CPU path.

Here: the GEMMs, the transformer and stem wrappers (the stem's conv1 from decoded bytes included) and the criterion.  The
routines on whole uint8 frames (crops, warps, NV12, JPEG, perturbations, the relevance paste) live in frames.py and are
re-exported below: their callers keep saying ``ops.crop_resize_u8`` ..., and ``kernel_profile`` here is their switch too.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib
# dtype codes, the stream handle, the row-strided activation layout (pad_ld / empty_rows / rows) and the cast launch
from ._common import (G256_MIN, ROW_ALIGN, Tensor, _DT, _c, _ptr, _req, _stream, cast, dtype_code,  # noqa: F401
                      empty_rows, pad_ld, rows, zeros_rows)
# the routines on decoded uint8 frames (frames.py looks prof up here when it launches, so it imports nothing from this module)
from .frames import (batch_draw, crop_resize_nv12, crop_resize_u8, decode_frames, draw_clips, encode_frames,  # noqa: F401
                     jpeg_bank_ingest, jpeg_decode_drawn_u8, jpeg_decode_indexed_u8, jpeg_decode_u8, jpeg_encode_u8,
                     jpeg_roundtrip_u8, nv12_to_rgb_u8, perturb_u8, png_decode_bank_drawn_u8, png_decode_bank_u8, png_decode_u8,
                     png_decode_bank_window_drawn_u8, png_decode_window_u8, png_encode_u8, relevance_paste_nv12,
                     relevance_paste_u8, warp_similarity_nv12, warp_similarity_u8)
# Every copy derived from a parameter (the compute-dtype operand, its transpose, the stacked operand, the stem's layouts):
# cached, refreshed and released by weights.py; the names below are the live cache's.
from .weights import (_refresh_derived, _refresh_plain_copies, _static_holders, _transposed_operand,  # noqa: F401
                      _versions, derived, invalidate_weight_cache, refresh_stale_operands, set_static_addresses,
                      static_addresses, weight_as, weight_cat_as)


# ------------------------------------------------------------------------------------------
# bench.py sets this to a list to time every GEMM launch with events on the launch stream:
# entries are (start_event, end_event, algorithmic_flops, (a_kc, b_kc), (M, N, K)).
gemm_profile = None
# likewise for the memory-bound / attention kernels: entries are (name, start_event, end_event, algorithmic_bytes,
# algorithmic_flops); bench.py turns them into achieved GB/s and TFLOP/s per kernel class.
kernel_profile = None


class prof:
    """with prof('ln_fwd', nbytes): <launch>  -- records events on the launch stream when bench.py asks for it"""

    def __init__(self, name, nbytes=0, flops=0):
        self.rec = (name, nbytes, flops) if kernel_profile is not None else None

    def __enter__(self):
        if self.rec is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.rec is not None and kernel_profile is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            kernel_profile.append((self.rec[0], self.e0, e1, self.rec[1], self.rec[2]))
        return False


_cus: dict = {}


def _cu_count(device) -> int:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _cus:
        n = torch.cuda.get_device_properties(idx).multi_processor_count
        _cus[idx] = (n if n >= 8 else 256) & ~7
    return _cus[idx]


def gemm_kernel_name(A, lda, a_kc, B, ldb, b_kc, C, ldc, M, N, K, epi=0, residual=None, bias=None, out_mode=0,
                     splitk=1, alpha=1.0, stats=0) -> str:
    """which kernel istvt_gemm launches for these operands (mirrors the dispatch rule in csrc/gemm.hip; the names
    are the ones rocprofv3 prints, so bench.py's per-kernel timings can be checked against profiles/)."""
    big = (A.dtype == torch.bfloat16 and bool(a_kc) == bool(b_kc) and M >= G256_MIN and N >= G256_MIN and N % 8 == 0
           and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0 and (K % 8 == 0 if a_kc else M % 8 == 0))
    if big:
        q_ok = (a_kc and M * lda * 2 < 0x7fffffff and N * ldb * 2 < 0x7fffffff and K >= 32 and out_mode == 0 and splitk == 1
                and (bias is None or alpha == 1.0) and not (epi != 0 and residual is not None))
        if q_ok:
            side = 'true' if (epi == 0 and residual is not None) else 'false'
            # row tile height as gemm.hip picks it: 256 unless ISTVT_GEMM_TM=224 (force) / -1 (rounds x height)
            cus = _cu_count(A.device)
            t256 = -(-M // 256) * -(-N // 256)
            t224 = -(-M // 224) * -(-N // 256)
            tm_env = int(os.environ.get('ISTVT_GEMM_TM', '0'))
            use224 = tm_env == 224 or (tm_env == -1 and -(-t224 // cus) * 224 < -(-t256 // cus) * 256)
            if stats:                   # 1: BatchNorm statistics, 2: column sums in the epilogue (always the 256-row tile)
                use224 = False
            # KHALF: K % 64 in 1..32 -> the last K tile of every output tile runs half its MFMAs (256-row tile only)
            khalf = (not use224) and K > 64 and 0 < (K & 63) <= 32
            return 'gemm256q_kernel<%d, %s, 0, %d, %d, %s>' % (epi, side, 224 if use224 else 256, stats,
                                                               'true' if khalf else 'false')
        t_ok = (not a_kc and out_mode == 3 and bias is None and residual is None and epi == 0 and K * lda * 2 < 0x7fffffff
                and K * ldb * 2 < 0x7fffffff)
        if t_ok:
            return 'gemm256t_kernel'
    t = '__bf16' if A.dtype == torch.bfloat16 else 'float'
    return 'gemm_kernel<%s, %s, %s>' % (t, str(bool(a_kc)).lower(), str(bool(b_kc)).lower())


def gemm_raw(A: Tensor, lda: int, a_kc: bool, B: Tensor, ldb: int, b_kc: bool, C: Tensor, ldc: int, M: int, N: int,
             K: int, *, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None, ldr: int = 0,
             C2: Optional[Tensor] = None, epi: int = 0, out_mode: int = 0, splitk: int = 1, alpha: float = 1.0,
             stats: Optional[Tensor] = None, csum: Optional[Tensor] = None, blocked: bool = True, a_sel_col: int = 0,
             gelu_d: bool = False):
    """stats: double [R][2][N] accumulator (stem.new_stats): the kernel adds the column sums / sums of squares of the
    stored outputs (fused train-mode BatchNorm statistics); only legal where stats_fusable() says so.
    csum=True (with stats, epi 2 only): only the column sums are accumulated (a bias gradient; the caller folds them
    with istvt_stats_reduce_add).
    blocked (float32 only): blocked summation over the reduction dimension (istvt_gemm flags bit 0).  False = one
    sequential fp32 chain, which the Xception stem's forward / input-gradient convolutions keep (it reproduces the
    reference CPU run's ReLU / arg-max decisions).
    a_sel_col > 0 (istvt_gemm flags bit 1): A is two planes of M rows, the second directly behind the first; output
    columns at or past a_sel_col (a multiple of 256) take their rows from the second plane."""
    _req(A); _req(B); _req(C)
    if A.dtype != B.dtype:
        raise TypeError('gemm operands must share a dtype (%s vs %s)' % (A.dtype, B.dtype))
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError('bias must be float32')
    prof = gemm_profile
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    rc = _lib.lib().istvt_gemm(A.data_ptr(), lda, int(a_kc), B.data_ptr(), ldb, int(b_kc), C.data_ptr(), ldc, M, N, K,
                               _ptr(bias), _ptr(residual), ldr, _ptr(C2), epi, out_mode, splitk, alpha,
                               stats[0, 0].data_ptr() if stats is not None else None,
                               stats[0, 1].data_ptr() if (stats is not None and csum is None) else None,
                               int(bool(blocked)) | ((2 | ((a_sel_col // 64) << 16)) if a_sel_col else 0) | (16 if gelu_d else 0)
                               | ((_cu_reserve.get(A.device.index, 0) >> 3) << 8 if _cu_reserve else 0),
                               dtype_code(A), _stream())
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * M * N * K, (bool(a_kc), bool(b_kc)), (M, N, K),
                     gemm_kernel_name(A, lda, a_kc, B, ldb, b_kc, C, ldc, M, N, K, epi, residual, bias, out_mode,
                                      splitk, alpha, 0 if stats is None else (2 if csum else 1))))
    _lib.check(rc, 'istvt_gemm')


# CUs the persistent NT GEMM launches leave free, per device index: an ARGUMENT of every istvt_gemm call (flags bits
# 8..15), not state of the library.  Python-side dict, read and written under the GIL by the main thread (all_reduce) and
# the autograd thread (the early all-reduce hook).
_cu_reserve: dict = {}


def set_cu_reserve(n: int, device=None) -> int:
    """CUs (a multiple of 8, at most 192) that the persistent NT GEMM launches issued on `device` from now on leave free;
    returns the previous value so the caller can restore it.  parallel.GradBucket raises it while its asynchronous
    all-reduce is in flight.  The value travels with each launch (istvt_gemm flags)."""
    n = int(n)
    if n < 0 or n > 192:
        raise RuntimeError('set_cu_reserve: %d is outside 0..192' % n)
    idx = torch._C._cuda_getDevice() if device is None else (device.index if isinstance(device, torch.device) else int(device))
    old = _cu_reserve.get(idx, 0)
    _cu_reserve[idx] = (n + 7) & ~7
    return old


def get_cu_reserve(device=None) -> int:
    idx = torch._C._cuda_getDevice() if device is None else (device.index if isinstance(device, torch.device) else int(device))
    return _cu_reserve.get(idx, 0)


def stats_fusable(x: Tensor, w: Tensor) -> bool:
    """whether linear_fwd(x, w, stats=...) may be used: the problem runs on the persistent bf16 NT kernel (the only one
    whose epilogue accumulates column statistics)"""
    M, K = x.shape
    N = w.shape[0]
    x2, lda = rows(x)
    w2, ldb = rows(w)
    # (with ISTVT_GEMM_TM=224 forced the C side still runs a statistics launch on the 256-row kernel)
    return (x.dtype == torch.bfloat16
            and gemm_kernel_name(x2, lda, True, w2, ldb, True, None, N, M, N, K).startswith('gemm256q_kernel<0, false'))


def linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
               gelu: bool = False, pad: bool = False, stats: Optional[Tensor] = None, blocked: bool = True,
               a_sel_col: int = 0, gelu_d: bool = False):
    """y = x @ w.T (+bias) (+residual); with gelu=True returns (u, gelu(u)) -- (gelu'(u), gelu(u)) with gelu_d=True: the
    derivative is all FeedForward's backward needs of u (istvt_gemm flags bit 4; pass the same flag to linear_dgrad).  x [M,K], w [N,K] (x's dtype); both may
    be row-strided views.  pad=True: the outputs are [M, N] views with line-aligned rows.  stats: see gemm_raw."""
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise RuntimeError('linear: weight %s does not match input width %d' % (tuple(w.shape), K))
    x, lda = rows(x)
    w, ldb = rows(w)
    y = empty_rows(M, N, x.dtype, x.device, pad)
    ldc = y.stride(0) if M > 1 else N
    if gelu:
        g = empty_rows(M, N, x.dtype, x.device, pad)
        gemm_raw(x, lda, True, w, ldb, True, y, ldc, M, N, K, bias=bias, C2=g, epi=1, blocked=blocked, gelu_d=gelu_d)
        return y, g
    ldr = 0
    if residual is not None:
        residual, ldr = rows(residual)
    gemm_raw(x, lda, True, w, ldb, True, y, ldc, M, N, K, bias=bias, residual=residual, ldr=ldr, stats=stats, blocked=blocked,
             a_sel_col=a_sel_col)
    return y


def linear_dgrad(dy: Tensor, w: Tensor, gelu_u: Optional[Tensor] = None, wt: Optional[Tensor] = None,
                 pad: bool = False, csum: Optional[Tensor] = None, blocked: bool = True, gelu_d: bool = False) -> Tensor:
    """dx = dy @ w  (dy [M,N], w [N,K]); with gelu_u: dx *= gelu'(gelu_u) (dx shaped like gelu_u); gelu_d=True: gelu_u IS the
    derivative linear_fwd(gelu=True, gelu_d=True) saved, dx *= gelu_u.
    wt = w^T [K,N] (optional): use the k-contiguous kernel instead of the transposed-operand one.
    csum (with gelu_u): float32 [K] += column sums of dx, taken in the GEMM's epilogue where the kernel supports it
    (else by a colsum pass here): the bias gradient of the Linear whose pre-activation gelu_u is."""
    M, N = dy.shape
    K = w.shape[1]
    dy, lda = rows(dy)
    dx = empty_rows(M, K, dy.dtype, dy.device, pad)
    ldc = dx.stride(0) if M > 1 else K
    epi = 2 if gelu_u is not None else 0
    c2 = None
    if gelu_u is not None:
        c2, ld2 = rows(gelu_u)
        if ld2 != ldc:                    # the kernel reads C2 with C's row stride
            c2 = empty_rows(M, K, dy.dtype, dy.device, pad)
            c2.copy_(gelu_u)
    if wt is None and dy.dtype == torch.bfloat16 and M >= G256_MIN and K >= G256_MIN and N % 8 == 0:
        wt = _transposed_operand(w)
    if wt is not None:
        wt, ldb = rows(wt)
        fuse = (csum is not None and epi == 2 and
                gemm_kernel_name(dy, lda, True, wt, ldb, True, dx, ldc, M, K, N, epi=2).startswith('gemm256q_kernel<2, false'))
        if fuse:
            # replicated double accumulator [R][2][K] (row 0 used): per-tile flushes from 256 workgroups into the 2912
            # addresses of the gradient itself serialise on same-address atomics (+60 us per launch, measured)
            from . import stem as _stem
            acc = _stem.new_stats(K, dy.device)
            gemm_raw(dy, lda, True, wt, ldb, True, dx, ldc, M, K, N, C2=c2, epi=epi, stats=acc, csum=True, gelu_d=gelu_d)
            _lib.check(_lib.lib().istvt_stats_reduce_add(acc.data_ptr(), K, csum.data_ptr(), _stream()), 'istvt_stats_reduce_add')
        else:
            gemm_raw(dy, lda, True, wt, ldb, True, dx, ldc, M, K, N, C2=c2, epi=epi, blocked=blocked, gelu_d=gelu_d)
            if csum is not None:
                colsum(dx, out=csum)
    else:
        w, ldb = rows(w)
        gemm_raw(dy, lda, True, w, ldb, False, dx, ldc, M, K, N, C2=c2, epi=epi, blocked=blocked, gelu_d=gelu_d)
        if csum is not None:
            colsum(dx, out=csum)
    return dx


_WG_TARGET = int(os.environ.get('ISTVT_WGRAD_WGS', '256'))      # workgroups a weight-gradient launch aims for


def _pick_splitk(out_rows: int, out_cols: int, red: int, big_tiles: bool = False) -> int:
    """split of the reduction dim for weight gradients so the grid fills the 256 CUs."""
    if big_tiles:          # 256x256 kernel, one workgroup per CU
        tiles = ((out_rows + 255) // 256) * ((out_cols + 255) // 256)
        s = max(1, _WG_TARGET // tiles)
    else:
        tiles = ((out_rows + 127) // 128) * ((out_cols + 127) // 128)
        s = max(1, 1024 // tiles)
    return min(s, max(1, red // 512))


def linear_wgrad(dy: Tensor, x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """out[N,K] (+)= dy.T @ x   (dy [M,N], x [M,K]); fp32 accumulate; the reduction dimension is split over workgroups
    that write fp32 partial slabs, summed in split order by one reduce pass (no atomics: bit-reproducible)."""
    M, N = dy.shape
    K = x.shape[1]
    (dy, ldy), (x, ldx) = rows(dy), rows(x)
    if out is None:
        out = torch.zeros((N, K), dtype=torch.float32, device=dy.device)
    big = dy.dtype == torch.bfloat16 and N >= G256_MIN and K >= G256_MIN and N % 8 == 0 and K % 8 == 0
    splits = _pick_splitk(N, K, M, big)
    if big:
        # partial slabs + a reduce pass: every split of a tile finishes at the same moment, so
        # atomics into the same 256x256 tile contend (measured 3-8x slower than this)
        splits = min(splits, (M + 63) // 64)
        kper = -(-(-(-M // splits)) // 64) * 64          # what the C side derives: ceil(ceil(M/s)/64)*64
        splits = -(-M // kper)
        ws = torch.empty((splits, N, K), dtype=torch.float32, device=dy.device)
        gemm_raw(dy, ldy, False, x, ldx, False, ws, K, N, K, M, out_mode=3, splitk=splits)
        _lib.check(_lib.lib().istvt_splitk_reduce(ws.data_ptr(), splits, N * K, out.data_ptr(), _stream()),
                   'istvt_splitk_reduce')
    elif splits > 1:
        bk = 64 if dy.dtype == torch.bfloat16 else 32
        kper = -(-(-(-M // splits)) // bk) * bk            # what the C side derives: ceil(ceil(M/s)/bk)*bk
        splits = -(-M // kper)
        ws = torch.empty((splits, N, K), dtype=torch.float32, device=dy.device)
        gemm_raw(dy, ldy, False, x, ldx, False, ws, K, N, K, M, out_mode=3, splitk=splits)
        if (N * K) % 4 == 0:
            _lib.check(_lib.lib().istvt_splitk_reduce(ws.data_ptr(), splits, N * K, out.data_ptr(), _stream()),
                       'istvt_splitk_reduce')
        else:
            _lib.check(_lib.lib().istvt_rows_reduce(ws.data_ptr(), splits, N * K, out.data_ptr(), _stream()), 'istvt_rows_reduce')
    else:
        gemm_raw(dy, ldy, False, x, ldx, False, out, K, N, K, M, out_mode=2, splitk=1)       # one writer per element
    return out


# ------------------------------------------------------------------------------------------
# Fused backward of a separable unit's 1x1 convolution and the BatchNorm behind it (csrc/pw_bwd.hip)
PW_BWD_PAIRS = ((64, 128), (128, 128))          # (Cin, Cout) the kernel is instantiated for


def pw_bwd_geometry(M: int):
    """(G, R): workgroups of a launch over M rows (= fp32 slabs of the workspace; the reduction split linear_wgrad takes
    for the same gradient) and rows per block of istvt_pw_bwd"""
    lib = _lib.lib()
    return int(lib.istvt_pw_bwd_grid(M)), int(lib.istvt_pw_bwd_rows())


def pw_bwd_fusable(dz: Tensor, d: Tensor, w: Tensor) -> bool:
    """whether pw_bwd() takes this unit: bf16, contiguous [M, C] operands, one of the instantiated channel pairs,
    operands below 2 GiB (the kernel addresses them with 32-bit byte offsets)"""
    if dz.dtype != torch.bfloat16 or d.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        return False
    if dz.dim() != 2 or d.dim() != 2 or w.dim() != 2 or not dz.is_contiguous() or not d.is_contiguous():
        return False
    M, cout = dz.shape
    cin = d.shape[1]
    if d.shape[0] != M or tuple(w.shape) != (cout, cin) or (cin, cout) not in PW_BWD_PAIRS or M < 1:
        return False
    return M * cout * 2 < 0x7fffffff and dz.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0


def pw_bwd(dz: Tensor, u: Tensor, bnp: Tensor, gamma: Tensor, stats: Tensor, d: Tensor, w: Tensor, out: Tensor,
           dgamma: Tensor, dbeta: Tensor, training: bool = True) -> Tensor:
    """One launch for du = BatchNorm-backward(dz, u), dd = du @ w and out[Cout, Cin] += du.T @ d (du never reaches memory;
    `out` gets the bits of linear_wgrad(du, d, out=out)).
    bnp: the BatchNorm's [4][Cout] pack; stats: its reduced backward sums (stem.new_stats layout, replica 0); w [Cout, Cin]
    in the compute dtype; out float32 [Cout, Cin] and dgamma / dbeta float32 [Cout] are accumulated into.  Only where
    pw_bwd_fusable() says so: anything else is refused by the library.  -> dd [M, Cin]"""
    for t in (dz, u, d, w, out, dgamma, dbeta):
        _req(t)
    M, cout = dz.shape
    cin = d.shape[1]
    if u.shape != dz.shape or not u.is_contiguous() or u.dtype != dz.dtype:
        raise RuntimeError('pw_bwd: u must match dz (%s %s vs %s %s)' % (tuple(u.shape), u.dtype, tuple(dz.shape), dz.dtype))
    if out.dtype != torch.float32 or out.numel() != cout * cin or not out.is_contiguous():
        raise RuntimeError('pw_bwd: the weight gradient must be contiguous float32 [%d, %d]' % (cout, cin))
    wt, ldwt = rows(_transposed_operand(w))
    lib = _lib.lib()
    G = int(lib.istvt_pw_bwd_grid(M))
    dd = torch.empty((M, cin), dtype=dz.dtype, device=dz.device)
    ws = torch.empty((G, cout * cin), dtype=torch.float32, device=dz.device)
    with prof('pw_bwd_fused', (2 * M * cout + 2 * M * cin) * dz.element_size()):
        _lib.check(lib.istvt_pw_bwd(dz.data_ptr(), u.data_ptr(), bnp.data_ptr(), gamma.data_ptr(), stats[0, 0].data_ptr(),
                                    stats[0, 1].data_ptr(), d.data_ptr(), d.stride(0), wt.data_ptr(), ldwt, dd.data_ptr(),
                                    ws.data_ptr(), out.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), M, cin, cout,
                                    int(training), dtype_code(dz), _stream()), 'istvt_pw_bwd')
    return dd


WGRAD_GROUP_MAX = 8


def wgrad_groupable(dy: Tensor, x: Tensor) -> bool:
    """whether linear_wgrad_group takes this weight gradient (the 256x256 bf16 TN kernel's conditions)"""
    if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or dy.dim() != 2 or x.dim() != 2:
        return False
    M, N = dy.shape
    K = x.shape[1]
    if N < G256_MIN or K < G256_MIN or N % 8 or K % 8 or x.shape[0] != M:
        return False
    for t in (dy, x):
        if t.stride(1) != 1 or (t.stride(0) * 2) % 16 or t.data_ptr() % 16 or M * t.stride(0) * 2 >= 0x7fffffff:
            return False
    return True


def linear_wgrad_group(items) -> None:
    """items: [(dy [M, N_i], x [M, K_i], out float [N_i, K_i])] with one M, each accepted by wgrad_groupable():
    out_i += dy_i.T @ x_i for all of them in one GEMM launch + one reduce launch (istvt_wgrad_group)."""
    import ctypes as C
    n = len(items)
    if not 1 <= n <= WGRAD_GROUP_MAX:
        raise RuntimeError('linear_wgrad_group: %d problems (1..%d)' % (n, WGRAD_GROUP_MAX))
    M = items[0][0].shape[0]
    Ns, Ks = [], []
    for dy, x, out in items:
        _req(dy); _req(x); _req(out)
        if dy.shape[0] != M or not wgrad_groupable(dy, x):
            raise RuntimeError('linear_wgrad_group: problem not groupable: dy %s x %s' % (tuple(dy.shape), tuple(x.shape)))
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != dy.shape[1] * x.shape[1]:
            raise RuntimeError('linear_wgrad_group: out must be a contiguous float [N, K] buffer')
        Ns.append(dy.shape[1]); Ks.append(x.shape[1])
    PA, LA, IA = C.c_void_p * n, C.c_long * n, C.c_int * n
    a_n, a_k = IA(*Ns), IA(*Ks)
    lib = _lib.lib()
    splits = lib.istvt_wgrad_group_splits(n, a_n, a_k, M)
    if splits < 1:
        _lib.check(splits, 'istvt_wgrad_group_splits')
    elems = sum(a * b for a, b in zip(Ns, Ks))
    ws = torch.empty((splits * elems,), dtype=torch.float32, device=items[0][0].device)
    prof = gemm_profile
    if prof is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    rc = lib.istvt_wgrad_group(n, PA(*[it[0].data_ptr() for it in items]), LA(*[it[0].stride(0) for it in items]),
                               PA(*[it[1].data_ptr() for it in items]), LA(*[it[1].stride(0) for it in items]),
                               PA(*[it[2].data_ptr() for it in items]), a_n, a_k, M, splits, ws.data_ptr(),
                               ws.numel(), _stream())
    if prof is not None:
        ev1.record()
        prof.append((ev0, ev1, 2.0 * M * elems, (False, False), (max(Ns), max(Ks), M), 'gemm256t_group_kernel(GemmGroupArgs)'))
    _lib.check(rc, 'istvt_wgrad_group')


def colsum(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    M, N = x.shape
    x, ld = rows(_req(x))
    if out is None:
        out = torch.zeros((N,), dtype=torch.float32, device=x.device)
    if N % 8 == 0:
        lib = _lib.lib()
        ws = torch.empty((lib.istvt_colsum_ws_elems(M, N),), dtype=torch.float32, device=x.device)
        with prof('colsum', M * N * x.element_size()):
            _lib.check(lib.istvt_colsum(x.data_ptr(), out.data_ptr(), M, N, ld, ws.data_ptr(), ws.numel(), dtype_code(x),
                                        _stream()), 'istvt_colsum')
    else:
        x = _c(x)
        # narrow outputs (e.g. the 1-logit head): a [N][1] GEMM against ones keeps it on the HIP path
        ones = torch.ones((M, 8), dtype=x.dtype, device=x.device)
        tmp = torch.zeros((N, 8), dtype=torch.float32, device=x.device)
        gemm_raw(x, N, False, ones, 8, False, tmp, 8, N, 8, M, out_mode=2, splitk=1)
        out += tmp[:, 0]
    return out


# ------------------------------------------------------------------------------------------
def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, pad: bool = False):
    """x [..., D] (row-strided views allowed) -> y [M, D] (pad=True: line-aligned rows), mean [M], rstd [M]."""
    x2, ldx = rows(_req(x))
    M, D = x2.shape
    y = empty_rows(M, D, x.dtype, x.device, pad)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    with prof('ln_fwd', 2 * M * D * x.element_size()):
        _lib.check(_lib.lib().istvt_layernorm_fwd(x2.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                                  y.stride(0) if M > 1 else D, mean.data_ptr(), rstd.data_ptr(), M, D, eps,
                                                  dtype_code(x), _stream()), 'istvt_layernorm_fwd')
    return (y if x.dim() == 2 else y.view(*x.shape)), mean, rstd


def layernorm_fwd_diff(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, B: int, F: int, P: int):
    """LayerNorm of x [B*F*P, D] (rows (b, f, p)) plus the frame difference of module.py:193 taken in fp32 before the
    rounding to x's dtype.  Returns (y, diff, mean, rstd): y and diff are the two [M, D] planes (line-aligned rows) of
    ONE buffer, diff first -- the layout gemm_raw(a_sel_col=...) takes."""
    x2, ldx = rows(_req(x))
    M, D = x2.shape
    if M != B * F * P:
        raise RuntimeError('layernorm_fwd_diff: %d rows are not B=%d x F=%d x P=%d' % (M, B, F, P))
    ld = pad_ld(D)
    planes = torch.empty((2, M, ld), dtype=x.dtype, device=x.device)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    with prof('ln_fwd', 3 * M * D * x.element_size()):
        _lib.check(_lib.lib().istvt_layernorm_fwd_diff(x2.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(),
                                                       planes[1].data_ptr(), ld, planes[0].data_ptr(), ld, mean.data_ptr(),
                                                       rstd.data_ptr(), B, F, P, D, eps, dtype_code(x), _stream()),
                   'istvt_layernorm_fwd_diff')
    return planes[1][:, :D], planes[0][:, :D], mean, rstd


def layernorm_bwd(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, dgamma: Tensor, dbeta: Tensor,
                  dres: Optional[Tensor] = None, pad: bool = False, dcol: Optional[Tensor] = None, defer=None) -> Tensor:
    """dx of LayerNorm (+ dres, the gradient arriving through the residual fork); dgamma / dbeta (float32 [D]) accumulate;
    dcol (float32 [D], optional) accumulates the column sums of dx (the producing Linear's bias gradient).  Row-strided
    views allowed.  Reproducible: the column sums are reduced in a fixed order (per-workgroup partial rows + one
    reduce launch), no atomics.
    defer (callable, optional): only the row kernel is launched here; the fold of the partial rows into dgamma / dbeta /
    dcol is handed to defer(ws, M, D, dgamma, dbeta, dcol), which runs layernorm_bwd_reduce(...) with those arguments
    wherever it likes (functional: on the weight-gradient stream) and keeps `ws` alive until that launch has run."""
    x2, ldx = rows(_req(x))
    M, D = x2.shape
    dy, ld_dy = rows(_req(dy))
    ld_res = 0
    if dres is not None:
        dres, ld_res = rows(dres)
    dx = empty_rows(M, D, x.dtype, x.device, pad)
    lib = _lib.lib()
    ws = torch.empty((lib.istvt_layernorm_bwd_ws_elems(M, D),), dtype=torch.float32, device=x.device)
    ntens = 3 + (dres is not None)          # dy, x, dx (+ dres)
    with prof('ln_bwd', ntens * M * D * x.element_size()):
        if defer is None:
            _lib.check(lib.istvt_layernorm_bwd(dy.data_ptr(), ld_dy, x2.data_ptr(), ldx, mean.data_ptr(), rstd.data_ptr(),
                                               gamma.data_ptr(), _ptr(dres), ld_res, dx.data_ptr(), dx.stride(0) if M > 1 else D,
                                               dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dcol), ws.data_ptr(), ws.numel(), M, D,
                                               dtype_code(x), _stream()), 'istvt_layernorm_bwd')
        else:
            _lib.check(lib.istvt_layernorm_bwd_partial(dy.data_ptr(), ld_dy, x2.data_ptr(), ldx, mean.data_ptr(),
                                                       rstd.data_ptr(), gamma.data_ptr(), _ptr(dres), ld_res, dx.data_ptr(),
                                                       dx.stride(0) if M > 1 else D, int(dcol is not None), ws.data_ptr(),
                                                       ws.numel(), M, D, dtype_code(x), _stream()),
                       'istvt_layernorm_bwd_partial')
    if defer is not None:
        defer(ws, M, D, dgamma, dbeta, dcol)
    return dx if x.dim() == 2 else dx.view(*x.shape)


def layernorm_bwd_reduce(ws: Tensor, M: int, D: int, dgamma: Tensor, dbeta: Tensor, dcol: Optional[Tensor] = None) -> None:
    """the second half of layernorm_bwd(defer=...): folds the partial rows in `ws` into dgamma / dbeta (/ dcol), on the
    current stream, in the same fixed order as the one-call form"""
    _lib.check(_lib.lib().istvt_layernorm_bwd_reduce(ws.data_ptr(), ws.numel(), M, D, dgamma.data_ptr(), dbeta.data_ptr(),
                                                     _ptr(dcol), _stream()), 'istvt_layernorm_bwd_reduce')


def _same_rows(like: Tensor, ld: int, M: int, D: int) -> Tensor:
    """an uninitialised [M, D] tensor with row stride ld (the layout of a saved operand: its gradient shares it)"""
    buf = torch.empty((M, ld), dtype=like.dtype, device=like.device)
    return buf if ld == D else buf[:, :D]


def attn_spatial_fwd(qkv: Tensor, BF: int, P: int, heads: int, dh: int, fp8: bool = False):
    """qkv [BF*P, 3*heads*dh] (row-strided views allowed) -> out [BF*P, heads*dh] with line-aligned rows, lse"""
    inner = heads * dh
    qkv, ldq = rows(_req(qkv))
    if tuple(qkv.shape) != (BF * P, 3 * inner):
        raise RuntimeError('attn_spatial: qkv %s is not (%d*%d, 3*%d)' % (tuple(qkv.shape), BF, P, inner))
    out = empty_rows(BF * P, inner, qkv.dtype, qkv.device)
    lse = torch.empty((BF * P, heads, 2), dtype=torch.float32, device=qkv.device)   # (row max [log2], 1/rowsum)
    if fp8 and qkv.dtype != torch.bfloat16:
        raise TypeError('the fp8 attention path needs bfloat16 activations')
    fn = _lib.lib().istvt_attn_spatial_fwd_fp8 if fp8 else _lib.lib().istvt_attn_spatial_fwd
    with prof('attn_spatial_fwd', 4 * BF * P * inner * qkv.element_size(), 4.0 * BF * heads * P * P * dh):
        _lib.check(fn(qkv.data_ptr(), ldq, out.data_ptr(), out.stride(0), lse.data_ptr(), BF, P, heads, dh, dh ** -0.5,
                      dtype_code(qkv), _stream()), 'istvt_attn_spatial_fwd')
    return out, lse


def attn_spatial_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, BF: int, P: int, heads: int, dh: int,
                     fp8: bool = False) -> Tensor:
    inner = heads * dh
    qkv, ldq = rows(_req(qkv))
    out, ldo = rows(_req(out))
    dout, ldd = rows(_req(dout))
    if ldd != ldo:                       # the kernels take one stride for out and dout
        d2 = _same_rows(out, ldo, BF * P, inner)
        d2.copy_(dout)
        dout = d2
    dqkv = _same_rows(qkv, ldq, BF * P, 3 * inner)
    delta = torch.empty((BF * P, heads), dtype=torch.float32, device=qkv.device)
    fn = _lib.lib().istvt_attn_spatial_bwd_fp8 if fp8 else _lib.lib().istvt_attn_spatial_bwd
    with prof('attn_spatial_bwd', 8 * BF * P * inner * qkv.element_size(), 10.0 * BF * heads * P * P * dh):
        _lib.check(fn(qkv.data_ptr(), ldq, out.data_ptr(), dout.data_ptr(), ldo, lse.data_ptr(), delta.data_ptr(),
                      dqkv.data_ptr(), BF, P, heads, dh, dh ** -0.5, dtype_code(qkv), _stream()), 'istvt_attn_spatial_bwd')
    return dqkv


def attn_temporal_fwd(qk: Tensor, v: Tensor, B: int, F: int, P: int, heads: int, dh: int, diff: bool = False):
    """qk [B*F*P, 2*heads*dh], v [B*F*P, heads*dh] (row-strided views allowed: e.g. the two column ranges of one packed
    q|k|v projection) -> out [B*F*P, heads*dh] with line-aligned rows.  diff = 1: frame difference on q, k in the kernel
    (TemporalResidualAttention, module.py:193); diff = 2 (bfloat16): q, k arrive differenced (layernorm_fwd_diff), the
    backward still returns gradients w.r.t. the un-differenced projections."""
    inner = heads * dh
    (qk, ldqk), (v, ldv) = rows(_req(qk)), rows(_req(v))
    if F > 17:
        raise RuntimeError('attn_temporal: at most 17 frames (T <= 16) are supported, got F=%d' % F)
    if tuple(qk.shape) != (B * F * P, 2 * inner) or tuple(v.shape) != (B * F * P, inner):
        raise RuntimeError('attn_temporal: shapes %s / %s do not match B=%d F=%d P=%d' % (tuple(qk.shape), tuple(v.shape), B, F, P))
    out = empty_rows(B * F * P, inner, v.dtype, v.device)
    ldo = out.stride(0)
    with prof('attn_temporal_fwd', 4 * B * F * P * inner * qk.element_size(), 4.0 * B * P * heads * F * F * dh):
        _lib.check(_lib.lib().istvt_attn_temporal_fwd(qk.data_ptr(), ldqk, v.data_ptr(), ldv, out.data_ptr(), ldo, B, F, P,
                                                      heads, dh, dh ** -0.5, int(diff), dtype_code(qk), _stream()),
                   'istvt_attn_temporal_fwd')
    return out


def attn_temporal_bwd(qk: Tensor, v: Tensor, dout: Tensor, B: int, F: int, P: int, heads: int, dh: int, diff: bool = False,
                      packed: bool = False):
    """-> (dqk, dv) laid out like qk and v.  packed=True (qk and v are the column ranges [0, 2*inner) and [2*inner,
    3*inner) of one projection buffer): the two gradients are the same column ranges of ONE [B*F*P, 3*inner] buffer,
    returned as (dqkv, None) -- the operand of a single input-gradient GEMM."""
    inner = heads * dh
    (qk, ldqk), (v, ldv) = rows(_req(qk)), rows(_req(v))
    dout, ldo = rows(_req(dout))
    M = B * F * P
    if packed:
        if ldqk != ldv or v.data_ptr() != qk.data_ptr() + 2 * inner * qk.element_size():
            raise RuntimeError('attn_temporal_bwd(packed=True): v is not the third column range of the qk buffer')
        dqkv = _same_rows(qk, ldqk, M, 3 * inner)
        dqk, dv = dqkv[:, :2 * inner], dqkv[:, 2 * inner:]
    else:
        dqkv = None
        dqk = _same_rows(qk, ldqk, M, 2 * inner)
        dv = _same_rows(v, ldv, M, inner)
    with prof('attn_temporal_bwd', 7 * M * inner * qk.element_size(), 10.0 * B * P * heads * F * F * dh):
        _lib.check(_lib.lib().istvt_attn_temporal_bwd(qk.data_ptr(), ldqk, v.data_ptr(), ldv, dout.data_ptr(), ldo,
                                                      dqk.data_ptr(), dv.data_ptr(), B, F, P, heads, dh, dh ** -0.5,
                                                      int(diff), dtype_code(qk), _stream()), 'istvt_attn_temporal_bwd')
    return (dqkv, None) if packed else (dqk, dv)


# ------------------------------------------------------------------------------------------
# Relevance maps (gradient-weighted attention rollout, DESIGN.md "Relevance maps"): one rollout step per attention call,
# r_out = r + (1/H) sum_h r E_h, E_h = max(0, A_h * dA_h).  r / r_out fp32, a new r_out per call.
def _rollout_vec(r: Tensor, rows_: int, n: int, what: str) -> Tensor:
    _req(r, what)
    if r.dtype != torch.float32 or r.numel() != rows_ * n:
        raise RuntimeError('%s: r must be float32 with %d x %d elements, got %s %s' % (what, rows_, n, r.dtype, tuple(r.shape)))
    return _c(r)


def attn_spatial_relevance(qkv: Tensor, dout: Tensor, lse: Tensor, r: Tensor, BF: int, P: int, heads: int, dh: int) -> Tensor:
    """qkv / lse as attn_spatial_fwd used and returned them, dout [BF*P, heads*dh], r [BF, P] fp32 -> r_out [BF, P]"""
    inner = heads * dh
    qkv, ldq = rows(_req(qkv))
    dout, ldd = rows(_req(dout))
    if tuple(qkv.shape) != (BF * P, 3 * inner) or tuple(dout.shape) != (BF * P, inner):
        raise RuntimeError('attn_spatial_relevance: qkv %s / dout %s do not match BF=%d P=%d heads=%d dh=%d'
                           % (tuple(qkv.shape), tuple(dout.shape), BF, P, heads, dh))
    if dout.dtype != qkv.dtype:
        raise TypeError('attn_spatial_relevance: dout is %s, qkv %s' % (dout.dtype, qkv.dtype))
    if lse.dtype != torch.float32 or lse.numel() != BF * P * heads * 2 or not lse.is_contiguous():
        raise RuntimeError('attn_spatial_relevance: lse must be the forward\'s contiguous float32 (BF*P, heads, 2) statistics')
    if dh not in (32, 64):
        raise RuntimeError('attn_spatial_relevance: dim_head must be 32 or 64, got %d' % dh)
    r = _rollout_vec(r, BF, P, 'attn_spatial_relevance')
    out = torch.empty((BF, P), dtype=torch.float32, device=qkv.device)
    # q, k, v and dO once per key tile (ceil(P / 64) tiles); two P x P x dh products per (frame, head)
    ntile = (P + 63) // 64
    with prof('attn_spatial_relevance', (3 * ntile + 1) * BF * P * inner * qkv.element_size(), 4.0 * BF * heads * P * P * dh):
        _lib.check(_lib.lib().istvt_attn_spatial_relevance(qkv.data_ptr(), ldq, dout.data_ptr(), ldd, lse.data_ptr(),
                                                           r.data_ptr(), out.data_ptr(), BF, P, heads, dh, dh ** -0.5,
                                                           dtype_code(qkv), _stream()), 'istvt_attn_spatial_relevance')
    return out


def attn_temporal_relevance(qkv: Tensor, dout: Tensor, r: Tensor, B: int, F: int, P: int, heads: int, dh: int,
                            diff: int = 0) -> Tensor:
    """qkv [B*F*P, 3*heads*dh] (the packed q|k|v TemporalAttnFn saved), dout [B*F*P, heads*dh], r [B*P, F] fp32 ->
    r_out [B*P, F]; diff: the forward's code (0 plain, 1 q / k differenced in the kernel, 2 q / k arrived differenced)"""
    inner = heads * dh
    qkv, ldq = rows(_req(qkv))
    dout, ldd = rows(_req(dout))
    if F > 17:
        raise RuntimeError('attn_temporal_relevance: at most 17 frames are supported, got F=%d' % F)
    if tuple(qkv.shape) != (B * F * P, 3 * inner) or tuple(dout.shape) != (B * F * P, inner):
        raise RuntimeError('attn_temporal_relevance: qkv %s / dout %s do not match B=%d F=%d P=%d heads=%d dh=%d'
                           % (tuple(qkv.shape), tuple(dout.shape), B, F, P, heads, dh))
    if dout.dtype != qkv.dtype:
        raise TypeError('attn_temporal_relevance: dout is %s, qkv %s' % (dout.dtype, qkv.dtype))
    if dh not in (32, 64) or int(diff) not in (0, 1, 2):
        raise RuntimeError('attn_temporal_relevance: dim_head must be 32 or 64 and diff 0, 1 or 2 (got %d, %r)' % (dh, diff))
    r = _rollout_vec(r, B * P, F, 'attn_temporal_relevance')
    out = torch.empty((B * P, F), dtype=torch.float32, device=qkv.device)
    M = B * F * P
    with prof('attn_temporal_relevance', (4 + (int(diff) == 1)) * M * inner * qkv.element_size(), 4.0 * B * P * heads * F * F * dh):
        _lib.check(_lib.lib().istvt_attn_temporal_relevance(qkv.data_ptr(), ldq, dout.data_ptr(), ldd, r.data_ptr(),
                                                            out.data_ptr(), B, F, P, heads, dh, dh ** -0.5, int(diff),
                                                            dtype_code(qkv), _stream()), 'istvt_attn_temporal_relevance')
    return out


def relevance_heatmap(cam: Tensor, scale: int = 16) -> Tensor:
    """cam (..., g, g) fp32 -> (..., g*scale, g*scale): bilinear upsampling (align_corners=False) and per-map min-max"""
    cam = _c(_req(cam, 'cam'))
    if cam.dtype != torch.float32 or cam.dim() < 2 or cam.shape[-1] != cam.shape[-2]:
        raise RuntimeError('relevance_heatmap: cam must be float32 (..., g, g), got %s %s' % (cam.dtype, tuple(cam.shape)))
    g, s = cam.shape[-1], int(scale)
    if not 1 <= g <= 64 or s < 1 or g * s > 8192:
        raise RuntimeError('relevance_heatmap: need 1 <= g <= 64 and 1 <= g*scale <= 8192 (g=%d, scale=%d)' % (g, s))
    maps = cam.numel() // (g * g)
    out = torch.empty((*cam.shape[:-2], g * s, g * s), dtype=torch.float32, device=cam.device)
    if maps == 0:
        return out
    with prof('relevance_heatmap', 4 * maps * (g * g + g * s * g * s)):
        _lib.check(_lib.lib().istvt_relevance_heatmap(cam.data_ptr(), out.data_ptr(), maps, g, s, _stream()),
                   'istvt_relevance_heatmap')
    return out


def check_window_starts(starts, n: int, T: int):
    """The window starts of an n-frame video as a list of ints: ascending and 0 <= s <= n - T, ValueError otherwise."""
    starts = [int(v) for v in (starts.tolist() if torch.is_tensor(starts) else starts)]
    if not starts:
        raise ValueError('window starts: no windows')
    if any(b < a for a, b in zip(starts, starts[1:])):
        raise ValueError('window starts must ascend, got %s' % (starts,))
    if starts[0] < 0 or starts[-1] > n - T:
        raise ValueError('window starts span [%d, %d]: %d-frame windows of a %d-frame video start in [0, %d]'
                         % (starts[0], starts[-1], T, n, n - T))
    return starts


def relevance_fuse_windows(r_s: Tensor, r_t: Tensor, logits: Tensor, starts, n: int, index: int = 0):
    """The rollouts of W sliding windows fused per frame.  r_s (W, T+1, P), r_t (W, P, T+1), logits (W, nc) fp32; starts:
    the W first frames (a host tensor or a list, validated here and uploaded on the current stream) -> frame_s, frame_t
    (n, P-1), frame_weight, frame_logit (n,) fp32 and count (n,) int32: plain means over the windows that cover a frame,
    in window order; zeros where none does."""
    for t, what in ((r_s, 'r_s'), (r_t, 'r_t'), (logits, 'logits')):
        _req(t, what)
        if t.dtype != torch.float32:
            raise TypeError('relevance_fuse_windows: %s must be float32, got %s' % (what, t.dtype))
    if r_s.dim() != 3 or r_t.dim() != 3 or logits.dim() != 2:
        raise RuntimeError('relevance_fuse_windows: r_s (W, T+1, P), r_t (W, P, T+1) and logits (W, nc) expected, got %s %s %s'
                           % (tuple(r_s.shape), tuple(r_t.shape), tuple(logits.shape)))
    W, F, P = r_s.shape
    T, nc = F - 1, logits.shape[1]
    if tuple(r_t.shape) != (W, P, F) or logits.shape[0] != W or T < 1 or P < 2:
        raise RuntimeError('relevance_fuse_windows: r_s %s, r_t %s and logits %s do not describe the same windows'
                           % (tuple(r_s.shape), tuple(r_t.shape), tuple(logits.shape)))
    if not 0 <= index < nc:
        raise IndexError('relevance_fuse_windows: index %d out of range for %d outputs' % (index, nc))
    starts = check_window_starts(starts, n, T)
    if len(starts) != W:
        raise RuntimeError('relevance_fuse_windows: %d starts for %d windows' % (len(starts), W))
    dev = r_s.device
    st = torch.tensor(starts, dtype=torch.int32).to(dev, non_blocking=True)
    r_s, r_t, logits = _c(r_s), _c(r_t), _c(logits)
    frame_s = torch.empty((n, P - 1), dtype=torch.float32, device=dev)
    frame_t = torch.empty((n, P - 1), dtype=torch.float32, device=dev)
    weight = torch.empty((n,), dtype=torch.float32, device=dev)
    logit = torch.empty((n,), dtype=torch.float32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    with prof('relevance_fuse_windows', 4 * (2 * W * F * P + 2 * n * (P - 1))):
        _lib.check(_lib.lib().istvt_relevance_fuse_windows(r_s.data_ptr(), r_t.data_ptr(), logits.data_ptr(), st.data_ptr(),
                                                           frame_s.data_ptr(), frame_t.data_ptr(), weight.data_ptr(),
                                                           logit.data_ptr(), count.data_ptr(), W, T, P, nc, int(index), int(n),
                                                           _stream()), 'istvt_relevance_fuse_windows')
    return frame_s, frame_t, weight, logit, count


def check_window_offsets(offsets, W: int):
    """The window ranges of V videos as a list of V + 1 ints: 0 = o[0] < o[1] < ... < o[V] = W (every video has a window),
    ValueError otherwise."""
    off = [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
    if len(off) < 2:
        raise ValueError('window offsets: no videos')
    if off[0] != 0 or off[-1] != W:
        raise ValueError('window offsets span [%d, %d], the %d windows [0, %d]' % (off[0], off[-1], W, W))
    if any(b <= a for a, b in zip(off, off[1:])):
        raise ValueError('window offsets must ascend strictly (a video without a window cannot be scored), got %s'
                         % (off if len(off) <= 16 else off[:16] + ['...'],))
    return off


def windows_reduce(logits: Tensor, offsets, checked: bool = False):
    """The windows of V videos reduced per video.  logits (W, nc) fp32, video v owns the rows [offsets[v], offsets[v+1]);
    offsets: V + 1 ints as a host tensor or a list, validated here (check_window_offsets) and uploaded on the current stream;
    checked=True takes an int32 device table the caller has validated already -> logit_mean, prob_mean (V, nc) fp32: the mean
    logit and the mean of 1 / (1 + exp(-logit)), each an fp64 sum in a fixed order rounded once."""
    _req(logits, 'logits')
    if logits.dtype != torch.float32:
        raise TypeError('windows_reduce: logits must be float32, got %s' % logits.dtype)
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise RuntimeError('windows_reduce: logits (W, nc) with W, nc >= 1 expected, got %s' % (tuple(logits.shape),))
    W, nc = logits.shape
    if checked:
        if (not torch.is_tensor(offsets) or offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2
                or offsets.device != logits.device):
            raise RuntimeError('windows_reduce: a checked offset table is int32 (V + 1,) on %s' % logits.device)
        off = _c(offsets)
        V = off.shape[0] - 1
    else:
        if torch.is_tensor(offsets) and offsets.dim() != 1:
            raise RuntimeError('windows_reduce: offsets must be (V + 1,), got %s' % (tuple(offsets.shape),))
        host = check_window_offsets(offsets, W)
        V = len(host) - 1
        off = torch.tensor(host, dtype=torch.int32).to(logits.device, non_blocking=True)
    if V > W:
        raise ValueError('windows_reduce: %d videos for %d windows' % (V, W))
    logits = _c(logits)
    logit_mean = torch.empty((V, nc), dtype=torch.float32, device=logits.device)
    prob_mean = torch.empty((V, nc), dtype=torch.float32, device=logits.device)
    with prof('windows_reduce', 4 * (W * nc + 2 * V * nc + V + 1)):
        _lib.check(_lib.lib().istvt_windows_reduce(logits.data_ptr(), off.data_ptr(), logit_mean.data_ptr(), prob_mean.data_ptr(),
                                                   W, V, nc, _stream()), 'istvt_windows_reduce')
    return logit_mean, prob_mean


AUC_COUNTS = ('greater', 'equal', 'positives', 'negatives', 'nonfinite', 'correct')


def auc_pairs(scores: Tensor, labels: Tensor, threshold: float = 0.0):
    """scores fp32 (V,), labels int32 (V,) of 0 / 1, both on the device -> counts int64 (6,) in the order of AUC_COUNTS and auc
    float64 (1,) = (greater + equal / 2) / (positives * negatives) over the (positive, negative) pairs, NaN when a class is
    empty.  A non-finite score is in no pair, never correct, and counted in nonfinite.  Nothing here synchronises."""
    _req(scores, 'scores')
    _req(labels, 'labels')
    if scores.dtype != torch.float32:
        raise TypeError('auc_pairs: scores must be float32, got %s' % scores.dtype)
    if labels.dtype != torch.int32:
        raise TypeError('auc_pairs: labels must be int32, got %s' % labels.dtype)
    if scores.dim() != 1 or scores.shape[0] < 1 or tuple(labels.shape) != tuple(scores.shape):
        raise RuntimeError('auc_pairs: scores (V,) and labels (V,) with V >= 1 expected, got %s and %s'
                           % (tuple(scores.shape), tuple(labels.shape)))
    if labels.device != scores.device:
        raise RuntimeError('auc_pairs: scores are on %s, labels on %s' % (scores.device, labels.device))
    V = scores.shape[0]
    scores, labels = _c(scores), _c(labels)
    ws = torch.empty((-(-V // 256), len(AUC_COUNTS)), dtype=torch.int64, device=scores.device)
    counts = torch.empty((len(AUC_COUNTS),), dtype=torch.int64, device=scores.device)
    auc = torch.empty((1,), dtype=torch.float64, device=scores.device)
    with prof('auc_pairs', 8 * V):
        _lib.check(_lib.lib().istvt_auc_pairs(scores.data_ptr(), labels.data_ptr(), float(threshold), ws.data_ptr(), ws.numel(),
                                              counts.data_ptr(), auc.data_ptr(), V, _stream()), 'istvt_auc_pairs')
    return counts, auc


def relevance_overlay_u8(frames: Tensor, maps: Tensor, lut: Tensor, scale: int = 16) -> Tensor:
    """frames uint8 (N, S, S, 3) (any view: a non-contiguous one is copied), maps fp32 (N, g, g), lut uint8 (256, 3) ->
    uint8 (N, g*scale, g*scale, 3): the colour-mapped, min-max normalised heat map added to the frame and the sum scaled
    to the frame's maximum (the reference's show_cam_on_image)."""
    _req(frames, 'frames')
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[1] != frames.shape[2]:
        raise RuntimeError('relevance_overlay_u8: frames must be channels-last uint8 (N, S, S, 3), got %s %s'
                           % (frames.dtype, tuple(frames.shape)))
    if maps.dtype != torch.float32 or maps.dim() != 3 or maps.shape[1] != maps.shape[2]:
        raise RuntimeError('relevance_overlay_u8: maps must be float32 (N, g, g), got %s %s' % (maps.dtype, tuple(maps.shape)))
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise RuntimeError('relevance_overlay_u8: lut must be uint8 (256, 3), got %s %s' % (lut.dtype, tuple(lut.shape)))
    if maps.shape[0] != frames.shape[0]:
        raise RuntimeError('relevance_overlay_u8: %d maps for %d frames' % (maps.shape[0], frames.shape[0]))
    if maps.device != frames.device or lut.device != frames.device:
        raise RuntimeError('relevance_overlay_u8: frames, maps and lut must share one device')
    N, S, g, s = frames.shape[0], frames.shape[1], maps.shape[1], int(scale)
    if not 1 <= g <= 64 or s < 1 or g * s > 8192 or not 1 <= N <= 65535 or S < 1:
        raise RuntimeError('relevance_overlay_u8: need 1 <= g <= 64, 1 <= g*scale <= 8192 and 1 <= N <= 65535 '
                           '(g=%d, scale=%d, N=%d)' % (g, s, N))
    frames, maps, lut = _c(frames), _c(maps), _c(lut)
    So = g * s
    out = torch.empty((N, So, So, 3), dtype=torch.uint8, device=frames.device)
    ws = torch.empty((N, 4), dtype=torch.float32, device=frames.device)
    with prof('relevance_overlay_u8', N * S * S * 3 + N * So * So * 3):
        _lib.check(_lib.lib().istvt_relevance_overlay_u8(frames.data_ptr(), maps.data_ptr(), lut.data_ptr(), ws.data_ptr(),
                                                         out.data_ptr(), N, S, g, s, _stream()), 'istvt_relevance_overlay_u8')
    return out


# ------------------------------------------------------------------------------------------
def tokens_fwd(feats: Tensor, space: Tensor, temporal: Tensor, pos: Tensor, pad: bool = False) -> Tensor:
    """feats [B,T,hw,D] -> x [B,(T+1)*(hw+1),D]; pos is the full (1,T,P_decl,D) parameter."""
    feats = _c(_req(feats))
    B, T, hw, D = feats.shape
    F, P = T + 1, hw + 1
    if pos.shape[1] != T:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (T, pos.shape[1]))          # same failure the reference hits at vivit.py:138
    if pos.shape[2] < P:
        raise RuntimeError('pos_embedding has %d tokens per frame, input needs %d' % (pos.shape[2], P))
    x = empty_rows(B * F * P, D, feats.dtype, feats.device, pad)
    with prof('tokens_fwd', (B * T * hw + B * F * P) * D * feats.element_size()):
        _lib.check(_lib.lib().istvt_tokens_fwd(feats.data_ptr(), space.data_ptr(), temporal.data_ptr(), pos.data_ptr(),
                                               x.data_ptr(), x.stride(0), B, F, P, D, pos.shape[2], dtype_code(feats),
                                               _stream()), 'istvt_tokens_fwd')
    return x.view(B, F * P, D)


def tokens_gather_fwd(bank: Tensor, idx: Tensor, space: Tensor, temporal: Tensor, pos: Tensor, pad: bool = False,
                      checked: bool = False) -> Tensor:
    """Token assembly for sliding windows: bank [cap,hw,D] per-frame features, idx int32 [W,T] bank slots of every window's
    frames -> x [W,(T+1)*(hw+1),D], bit-identical to tokens_fwd(bank[idx]).  The table is validated here, on the host: pass
    it as a host tensor (it is uploaded on the current stream); a device table costs one synchronisation to check.
    checked=True takes a device table whose range the caller has validated on the host already (video.SetPlan's tables,
    uploaded once per call): no synchronisation."""
    bank = _c(_req(bank, 'feature bank'))
    if bank.dim() != 3:
        raise RuntimeError('tokens_gather_fwd: bank must be (cap, h*w, D), got %s' % (tuple(bank.shape),))
    if idx.dim() != 2 or idx.dtype != torch.int32:
        raise RuntimeError('tokens_gather_fwd: idx must be an int32 (windows, frames) table, got %s %s'
                           % (idx.dtype, tuple(idx.shape)))
    cap, hw, D = bank.shape
    W, T = idx.shape
    if W == 0:
        raise RuntimeError('tokens_gather_fwd: no windows')
    if checked:
        if not idx.is_cuda:
            raise RuntimeError('tokens_gather_fwd: a checked table is on the device already')
    else:
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= cap:
            raise IndexError('tokens_gather_fwd: slots span [%d, %d], the bank has %d' % (lo, hi, cap))
    idx = _c(idx)
    if not idx.is_cuda:
        idx = idx.to(bank.device, non_blocking=True)
    elif idx.device != bank.device:
        raise RuntimeError('tokens_gather_fwd: idx is on %s, the bank on %s' % (idx.device, bank.device))
    F, P = T + 1, hw + 1
    if pos.shape[1] != T:
        raise RuntimeError('The size of tensor a (%d) must match the size of tensor b (%d) at non-singleton dimension 1'
                           % (T, pos.shape[1]))          # as tokens_fwd
    if pos.shape[2] < P:
        raise RuntimeError('pos_embedding has %d tokens per frame, input needs %d' % (pos.shape[2], P))
    if pos.shape[-1] != D or space.shape[-1] != D or temporal.shape[-1] != D:
        raise RuntimeError('tokens_gather_fwd: bank has %d channels, the tokens %d' % (D, pos.shape[-1]))
    x = empty_rows(W * F * P, D, bank.dtype, bank.device, pad)
    with prof('tokens_gather_fwd', (W * T * hw + W * F * P) * D * bank.element_size() + W * T * 4):
        _lib.check(_lib.lib().istvt_tokens_gather_fwd(bank.data_ptr(), idx.data_ptr(), space.data_ptr(), temporal.data_ptr(),
                                                      pos.data_ptr(), x.data_ptr(), x.stride(0), W, F, P, D, pos.shape[2],
                                                      cap, dtype_code(bank), _stream()), 'istvt_tokens_gather_fwd')
    return x.view(W, F * P, D)


# ---- conv1 of the Xception stem (3 -> 32, 3x3, stride 2, no padding) from its two kinds of input: the float32 NCHW clip, or
# decoded frames (uint8, channels last) read through a view and normalised in the kernel.  Every byte routine gives the bits of
# its float twin on clips.to_float(src, mean, std, view, S) made on the host.
def _float_clip(what: str, x: Tensor):
    _req(x, 'input clip')
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.shape[0] == 0:
        raise RuntimeError('%s expects a float32 (frames, 3, S, S) clip, got %s %s' % (what, x.dtype, tuple(x.shape)))
    return _c(x), x.shape[0], x.shape[2]


def _conv1_out(Fr: int, S: int, dtype, device) -> Tensor:
    if dtype not in _DT:
        raise TypeError('istvt_amd supports float32 and bfloat16 activations, got %s' % dtype)
    Ho = (S - 3) // 2 + 1
    return torch.empty((Fr * Ho * Ho, 32), dtype=dtype, device=device)


def _conv1_w(what: str, weight: Tensor, device) -> Tensor:
    if weight.dtype != torch.float32 or tuple(weight.shape) != (32, 3, 3, 3) or weight.device != device:
        raise RuntimeError('%s: weight must be conv1.weight, float32 (32, 3, 3, 3) on %s' % (what, device))
    return _c(weight.detach())


def _conv1_du1(what: str, du1: Tensor, Fr: int, S: int, device) -> Tensor:
    Ho = (S - 3) // 2 + 1
    if du1.device != device or du1.dim() != 2 or tuple(du1.shape) != (Fr * Ho * Ho, 32):
        raise RuntimeError('%s: du1 must be (%d, 32) on %s, got %s' % (what, Fr * Ho * Ho, device, tuple(du1.shape)))
    return _c(du1)


def _conv1_wgrad_ws(device):
    """(dW float32 [32, 32] zeroed, the kernel's slab workspace)"""
    return (torch.zeros((32, 32), dtype=torch.float32, device=device),
            torch.empty((_lib.lib().istvt_conv1_wgrad_slabs(), 1024), dtype=torch.float32, device=device))


def conv1_fwd(x: Tensor, weight: Tensor, dtype: torch.dtype) -> Tensor:
    """x float32 [Fr,3,S,S], weight conv1.weight (32,3,3,3) float32 -> u1 [Fr*Ho*Ho, 32] in `dtype` (the direct kernel)."""
    x, Fr, S = _float_clip('conv1_fwd', x)
    w = _conv1_w('conv1_fwd', weight, x.device)
    u1 = _conv1_out(Fr, S, dtype, x.device)
    _lib.check(_lib.lib().istvt_conv1_fwd(x.data_ptr(), w.data_ptr(), u1.data_ptr(), Fr, S, _DT[dtype], _stream()),
               'istvt_conv1_fwd')
    return u1


def conv1_wgrad(du1: Tensor, x: Tensor) -> Tensor:
    """du1 [Fr*Ho*Ho, 32] (float32 or bfloat16), x float32 [Fr,3,S,S] -> dW float32 [32, 32], column k = ci*9 + dy*3 + dx
    (27..31 zero).  Needs Ho <= 128 (S <= 258)."""
    x, Fr, S = _float_clip('conv1_wgrad', x)
    du1 = _conv1_du1('conv1_wgrad', du1, Fr, S, x.device)
    dW, slabs = _conv1_wgrad_ws(x.device)
    _lib.check(_lib.lib().istvt_conv1_wgrad(du1.data_ptr(), x.data_ptr(), slabs.data_ptr(), dW.data_ptr(), Fr, S,
                                            dtype_code(du1), _stream()), 'istvt_conv1_wgrad')
    return dW


def im2col_conv1(x: Tensor, dtype: torch.dtype) -> Tensor:
    """x float32 [Fr,3,S,S] -> col [Fr*Ho*Ho, 32] in `dtype`: columns (dy,dx,ci) + 5 zero columns."""
    x, Fr, S = _float_clip('im2col_conv1', x)
    col = _conv1_out(Fr, S, dtype, x.device)
    _lib.check(_lib.lib().istvt_im2col_conv1(x.data_ptr(), col.data_ptr(), Fr, S, _DT[dtype], _stream()), 'istvt_im2col_conv1')
    return col


def _u8_source(what: str, src: Tensor, view, S: Optional[int], mean: Tensor, std: Tensor, dtype, checked: bool):
    """Arguments common to the kernels that read a view of decoded frames: src uint8 [Fr,Hs,Ws,3], view int32 [Fr,3] =
    (y0, x0, flip) or None, crop side S (None: the frames' own side).  A view is validated on the host (clips.check_views)
    before any launch and then uploaded; checked=True takes a device table the caller has validated already (the stem:
    one table, checked once, read by the forward and the backward).  -> (src, Fr, Hs, Ws, S, device table or None)"""
    from . import clips
    _req(src, 'frames')
    if src.dtype != torch.uint8:
        raise TypeError('%s: frames must be uint8, got %s' % (what, src.dtype))
    if src.dim() != 4 or src.shape[3] != 3:
        raise RuntimeError('%s expects channels-last (frames, Hs, Ws, 3) uint8 input, got %s' % (what, tuple(src.shape)))
    if dtype not in _DT:
        raise TypeError('istvt_amd supports float32 and bfloat16 activations, got %s' % dtype)
    for t, n in ((mean, 'mean'), (std, 'std')):
        if t.dtype != torch.float32 or t.numel() != 3 or t.device != src.device:
            raise RuntimeError('%s: %s must be 3 float32 values on %s' % (what, n, src.device))
    Fr, Hs, Ws = src.shape[0], src.shape[1], src.shape[2]
    if Fr == 0:
        raise RuntimeError('%s: empty input %s' % (what, tuple(src.shape)))
    if checked:
        if S is None or S < 3 or S > min(Hs, Ws) or (view is None and (Hs != S or Ws != S)):
            raise ValueError('%s: crop side %r does not fit %d x %d frames' % (what, S, Hs, Ws))
        if view is not None and (view.dtype != torch.int32 or tuple(view.shape) != (Fr, 3) or view.device != src.device):
            raise RuntimeError('%s: a checked view table is int32 (%d, 3) on %s' % (what, Fr, src.device))
        vdev = None if view is None else _c(view)
    else:
        v = clips.check_views(view, Fr, Hs, Ws, S)
        S = Hs if S is None else S
        vdev = None if v is None else v.contiguous().to(src.device)
    return _c(src), Fr, Hs, Ws, S, vdev


def conv1_fwd_u8(frames: Tensor, mean: Tensor, std: Tensor, weight: Tensor, dtype: torch.dtype) -> Tensor:
    """conv1 straight from decoded frames, the inference entry: frames uint8 [Fr,S,S,3] whole (the identity view), mean / std
    float32 [3] on the device -> u1 [Fr*Ho*Ho, 32] in `dtype`, bit-identical to conv1_fwd on
    ((frames.float() / 255 - mean) / std).permute(0, 3, 1, 2)."""
    # (the one refusal kept here: _u8_source's check_views answers a non-square frame with ValueError, this entry always
    # answered RuntimeError; a wrong dtype stays _u8_source's TypeError)
    if frames.dtype == torch.uint8 and frames.dim() == 4 and (frames.shape[1] != frames.shape[2] or frames.shape[1] < 3):
        raise RuntimeError('conv1_fwd_u8 expects channels-last (frames, S, S, 3) uint8 input, got %s' % (tuple(frames.shape),))
    frames, Fr, _, _, S, _ = _u8_source('conv1_fwd_u8', frames, None, None, mean, std, dtype, False)
    w = _conv1_w('conv1_fwd_u8', weight, frames.device)
    u1 = _conv1_out(Fr, S, dtype, frames.device)
    with prof('conv1_fwd_u8', Fr * S * S * 3 + u1.numel() * u1.element_size(), 2.0 * 27 * u1.numel()):
        _lib.check(_lib.lib().istvt_conv1_fwd_u8(frames.data_ptr(), _c(mean).data_ptr(), _c(std).data_ptr(), w.data_ptr(),
                                                 u1.data_ptr(), Fr, S, _DT[dtype], _stream()), 'istvt_conv1_fwd_u8')
    return u1


def conv1_fwd_u8_view(src: Tensor, view, S: Optional[int], mean: Tensor, std: Tensor, weight: Tensor, dtype: torch.dtype,
                      checked: bool = False) -> Tensor:
    """conv1 from a view of decoded frames (clips.py): src uint8 [Fr,Hs,Ws,3], view int32 [Fr,3] or None, crop side S ->
    u1 [Fr*Ho*Ho, 32] in `dtype`, bit-identical to conv1_fwd on clips.to_float(src, mean, std, view, S) made on the host."""
    src, Fr, Hs, Ws, S, vdev = _u8_source('conv1_fwd_u8_view', src, view, S, mean, std, dtype, checked)
    w = _conv1_w('conv1_fwd_u8_view', weight, src.device)
    u1 = _conv1_out(Fr, S, dtype, src.device)
    with prof('conv1_fwd_u8_view', Fr * S * S * 3 + u1.numel() * u1.element_size(), 2.0 * 27 * u1.numel()):
        _lib.check(_lib.lib().istvt_conv1_fwd_u8_view(src.data_ptr(), src.numel(), Hs, Ws, _ptr(vdev), _c(mean).data_ptr(),
                                                      _c(std).data_ptr(), w.data_ptr(), u1.data_ptr(), Fr, S, _DT[dtype],
                                                      _stream()), 'istvt_conv1_fwd_u8_view')
    return u1


def conv1_wgrad_u8(du1: Tensor, src: Tensor, view, S: Optional[int], mean: Tensor, std: Tensor,
                   checked: bool = False) -> Tensor:
    """conv1's weight gradient from a view of decoded frames: du1 as conv1_wgrad takes it, source and view as
    conv1_fwd_u8_view -> dW float32 [32, 32], bit-identical to conv1_wgrad on clips.to_float(...); the same limit."""
    src, Fr, Hs, Ws, S, vdev = _u8_source('conv1_wgrad_u8', src, view, S, mean, std, du1.dtype, checked)
    du1 = _conv1_du1('conv1_wgrad_u8', du1, Fr, S, src.device)
    dW, slabs = _conv1_wgrad_ws(src.device)
    with prof('conv1_wgrad_u8', du1.numel() * du1.element_size() + Fr * S * S * 3, 2.0 * 32 * du1.numel()):
        _lib.check(_lib.lib().istvt_conv1_wgrad_u8(du1.data_ptr(), src.data_ptr(), src.numel(), Hs, Ws, _ptr(vdev),
                                                   _c(mean).data_ptr(), _c(std).data_ptr(), slabs.data_ptr(), dW.data_ptr(),
                                                   Fr, S, _DT[du1.dtype], _stream()), 'istvt_conv1_wgrad_u8')
    return dW


def im2col_conv1_u8(src: Tensor, view, S: Optional[int], mean: Tensor, std: Tensor, dtype: torch.dtype,
                    checked: bool = False) -> Tensor:
    """conv1's im2col from a view of decoded frames -> col [Fr*Ho*Ho, 32] in `dtype`, bit-identical to im2col_conv1 on
    clips.to_float(...)."""
    src, Fr, Hs, Ws, S, vdev = _u8_source('im2col_conv1_u8', src, view, S, mean, std, dtype, checked)
    col = _conv1_out(Fr, S, dtype, src.device)
    with prof('im2col_conv1_u8', Fr * S * S * 3 + col.numel() * col.element_size()):
        _lib.check(_lib.lib().istvt_im2col_conv1_u8(src.data_ptr(), src.numel(), Hs, Ws, _ptr(vdev), _c(mean).data_ptr(),
                                                    _c(std).data_ptr(), col.data_ptr(), Fr, S, _DT[dtype], _stream()),
                   'istvt_im2col_conv1_u8')
    return col


def tokens_bwd(dx: Tensor, B: int, T: int, hw: int, D: int, dspace: Tensor, dtemporal: Tensor, dpos: Tensor,
               need_dfeats: bool) -> Optional[Tensor]:
    dx, lddx = rows(_req(dx))
    F, P = T + 1, hw + 1
    dfeats = torch.empty((B, T, hw, D), dtype=dx.dtype, device=dx.device) if need_dfeats else None
    ws = torch.empty(((P + F - 1) * D,), dtype=torch.float32, device=dx.device)       # partial rows of the two token gradients
    with prof('tokens_bwd', (B * F * P + (B * T * hw if need_dfeats else 0)) * D * dx.element_size()):
        _lib.check(_lib.lib().istvt_tokens_bwd(dx.data_ptr(), lddx, _ptr(dfeats), dspace.data_ptr(), dtemporal.data_ptr(),
                                               dpos.data_ptr(), ws.data_ptr(), B, F, P, D, dpos.shape[2], dtype_code(dx),
                                               _stream()), 'istvt_tokens_bwd')
    return dfeats


def frame_diff(x: Tensor, B: int, F: int, P: int, adjoint: bool = False) -> Tensor:
    x = _c(_req(x))
    D = x.shape[-1]
    if x.numel() != B * F * P * D:
        raise RuntimeError('frame_diff: %s is not (B=%d, F=%d, P=%d, D)' % (tuple(x.shape), B, F, P))
    out = torch.empty_like(x)
    _lib.check(_lib.lib().istvt_frame_diff(x.data_ptr(), out.data_ptr(), B, F, P, D, int(adjoint), dtype_code(x),
                                           _stream()), 'istvt_frame_diff')
    return out


# ---- the criterion (include/istvt_hip.h istvt_bce_logits) ------------------------------------------
BCE_TARGET_KINDS = {torch.float32: 0, torch.int64: 1, torch.int32: 2, torch.uint8: 3}
BCE_REDUCTIONS = {'none': 0, 'mean': 1, 'sum': 2}
METER_WORDS = 10                   # istvt_loss_meter: two float64 sums and eight int64 words


def check_meter_block(meter: Tensor, device) -> Tensor:
    if (not torch.is_tensor(meter) or meter.dtype != torch.int64 or tuple(meter.shape) != (METER_WORDS,)
            or not meter.is_contiguous() or meter.device != device):
        raise RuntimeError('bce_logits: a meter block is a contiguous int64 (%d,) tensor on %s' % (METER_WORDS, device))
    return meter


def bce_logits(z: Tensor, y: Tensor, weight: Optional[Tensor] = None, pos_weight: float = 1.0, label_smoothing: float = 0.0,
               reduction: str = 'mean', threshold: float = 0.0, want_loss: bool = False, want_reduced: bool = True,
               want_grad: bool = True, meter: Optional[Tensor] = None):
    """BCE with logits on z (n,) float32 (any positive stride) against y (n,) float32 / int64 / int32 / uint8 / bool, in one
    launch -> (loss (n,) or None, reduced (1,) or None, d (n,) or None): the per-sample losses, their sum or mean (the sum with
    reduction 'none') and the unscaled logit gradient of the reduced value; `meter` (a raw block, TrainMeter.tensor) is added
    to.  Shapes and dtypes are checked before the device is, so a host tensor of the wrong kind says what is wrong with it."""
    if z.dtype != torch.float32:
        raise TypeError('bce_logits: logits must be float32, got %s' % z.dtype)
    if y.dtype == torch.bool:
        y = y.view(torch.uint8)
    if y.dtype not in BCE_TARGET_KINDS:
        raise TypeError('bce_logits: targets must be float32, int64, int32, uint8 or bool, got %s' % y.dtype)
    if z.dim() != 1 or z.shape[0] < 1:
        raise RuntimeError('bce_logits: logits (n,) with n >= 1 expected, got %s (pass outputs.view(-1))' % (tuple(z.shape),))
    n = z.shape[0]
    if tuple(y.shape) != (n,):
        raise RuntimeError('bce_logits: %d logits, targets %s' % (n, tuple(y.shape)))
    if weight is not None:
        if weight.dtype != torch.float32:
            raise TypeError('bce_logits: weight must be float32, got %s' % weight.dtype)
        if tuple(weight.shape) != (n,):
            raise RuntimeError('bce_logits: %d logits, per-sample weight %s' % (n, tuple(weight.shape)))
    if reduction not in BCE_REDUCTIONS:
        raise ValueError("bce_logits: reduction must be 'none', 'mean' or 'sum', got %r" % (reduction,))
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError('bce_logits: label_smoothing must be in [0, 1), got %r' % (label_smoothing,))
    if n > 1 << 30:
        raise RuntimeError('bce_logits: at most 2^30 logits per call, got %d' % n)
    _req(z, 'logits')
    for t, name in ((y, 'targets'), (weight, 'weight')):
        if t is not None and t.device != z.device:
            raise RuntimeError('bce_logits: logits are on %s, %s on %s' % (z.device, name, t.device))
    if meter is not None:
        check_meter_block(meter, z.device)
    stride = z.stride(0) if n > 1 else 1
    if stride < 1:
        z, stride = z.contiguous(), 1
    y = _c(y)
    weight = None if weight is None else _c(weight)
    loss = torch.empty((n,), dtype=torch.float32, device=z.device) if want_loss else None
    reduced = torch.empty((1,), dtype=torch.float32, device=z.device) if want_reduced else None
    d = torch.empty((n,), dtype=torch.float32, device=z.device) if want_grad else None
    with prof('bce_logits', 4 * n * (2 + (weight is not None) + want_loss + want_grad)):
        _lib.check(_lib.lib().istvt_bce_logits(z.data_ptr(), stride, y.data_ptr(), BCE_TARGET_KINDS[y.dtype], _ptr(weight),
                                               float(pos_weight), float(label_smoothing), BCE_REDUCTIONS[reduction],
                                               float(threshold), n, _ptr(loss), _ptr(reduced), _ptr(d), _ptr(meter), _stream()),
                   'istvt_bce_logits')
    return loss, reduced, d


def bce_logits_bwd(d: Tensor, g: Tensor) -> Tensor:
    """d (n,) from bce_logits times the incoming gradient g -- one element (mean / sum) or (n,) ('none'), read on the device"""
    _req(d, 'd')
    _req(g, 'grad_output')
    if d.dtype != torch.float32 or g.dtype != torch.float32:
        raise TypeError('bce_logits_bwd: float32 expected, got %s and %s' % (d.dtype, g.dtype))
    n = d.shape[0]
    if d.dim() != 1 or g.numel() not in (1, n) or g.device != d.device:
        raise RuntimeError('bce_logits_bwd: d %s, grad_output %s on %s / %s' % (tuple(d.shape), tuple(g.shape), d.device, g.device))
    per_sample = n > 1 and g.numel() == n
    d, g = _c(d), _c(g)
    grad = torch.empty_like(d)
    with prof('bce_logits_bwd', 12 * n):
        _lib.check(_lib.lib().istvt_bce_logits_bwd(d.data_ptr(), g.data_ptr(), int(per_sample), grad.data_ptr(), n, _stream()),
                   'istvt_bce_logits_bwd')
    return grad
