"""The routines on decoded uint8 frames (clips.py holds their definitions on the host): crops, similarity warps, the NV12
readers, the JPEG round trip, the perturbations and the relevance paste, in packed RGB and in NV12; and the JPEG decoder
that makes such frames from files (jpeg_decode_u8, decode_frames) and the encoder that makes files from them (jpeg_encode_u8,
encode_frames); and the batch draw, which makes the index and the tables of a training batch on the device (batch_draw,
jpeg_decode_drawn_u8, draw_clips); and the PNG decoder (png_decode_u8), which decode_frames takes packed files of too, and
the PNG writer (png_encode_u8), which encode_frames(format='png') ends in.

One argument front end serves them all: _rgb_source / _nv12_source (the frames), _side, _frame_table (a per-frame table:
checked as it is, or validated on the host, spread over a clip's frames and uploaded), _u8_out and _no_overlap (the result),
_nv12_launches (the launches of an NV12 batch with the per-frame tensors sliced alongside) and _paste_target (in place, `out`
or a copy); for the file decoders _packed (files or a packed batch), _canvas, _decode_buffers ((scratch, sizes, status) made
or checked), _decode_args (their argument block) and _call (the entry called, recorded and its return code read).  crop_frames and paste_maps pick the entry for a pixel format.  ops re-exports the public entries, and ops.prof
records them: ops.kernel_profile stays the one switch.  Nothing here synchronises; with checked=True nothing is read back.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib, clips
from ._common import Tensor, _c, _req, _stream


def prof(name, nbytes):
    """ops.prof (ops imports this module, so the name is looked up at the call)"""
    from . import ops
    return ops.prof(name, nbytes)


# ---- the argument front end ------------------------------------------------------------------------------------------------
def _rgb_source(what: str, frames: Tensor, clips_too: bool = True, contiguous: bool = False, on_device: bool = True,
                channels=(3,)):
    """Packed RGB frames: uint8, channels last, (n, Hs, Ws, 3) or (clips_too) (B, T, Hs, Ws, 3) on the device, not empty, at
    most 16384 x 16384; contiguous=True refuses what would have to be copied.  -> (n frames, T or None, Hs, Ws); the kernels
    take a pointer and n, so the flat source is _c(frames).  on_device=False leaves the device to the caller, who asks for it
    (_req) behind the argument errors that need none.  channels: the channel counts taken in the place of 3 (the PNG writer:
    1, 3 or 4); the caller reads the count from the shape."""
    if on_device:
        _req(frames, 'frames')
    elif not torch.is_tensor(frames):
        raise TypeError('%s: frames must be a uint8 tensor, got %s' % (what, type(frames).__name__))
    if frames.dtype != torch.uint8:
        raise TypeError('%s: frames must be uint8, got %s' % (what, frames.dtype))
    if tuple(channels) != (3,) and (frames.dim() not in (4, 5) or frames.shape[-1] not in channels):
        raise RuntimeError('%s expects channels-last (n, H, W, C) or (B, T, H, W, C) uint8 input with C in %s (grey also as (n, H, W)), '
                           'got %s' % (what, tuple(channels), tuple(frames.shape)))
    if frames.dim() not in ((4, 5) if clips_too else (4,)) or frames.shape[-1] not in channels:
        hw = 'H, W' if contiguous else 'Hs, Ws'
        raise RuntimeError('%s expects channels-last (n, %s, 3)%s uint8 input, got %s'
                           % (what, hw, ' or (B, T, %s, 3)' % hw if clips_too else '', tuple(frames.shape)))
    if frames.numel() == 0:
        raise RuntimeError('%s: empty input %s' % (what, tuple(frames.shape)))
    if contiguous and not frames.is_contiguous():
        raise RuntimeError('%s: frames must be contiguous, got strides %s for %s'
                           % (what, tuple(frames.stride()), tuple(frames.shape)))
    Hs, Ws = int(frames.shape[-3]), int(frames.shape[-2])
    if Hs > 16384 or Ws > 16384:
        raise ValueError('%s: frames of at most 16384 x 16384, got %d x %d' % (what, Hs, Ws))
    T = int(frames.shape[1]) if frames.dim() == 5 else None
    return frames.numel() // (Hs * Ws * int(frames.shape[-1])), T, Hs, Ws


def _nv12_launch(t: Tensor, first: int, Hs: int, Ws: int):
    """t uint8 [n, 3 Hs / 2, Ws] with contiguous rows -> (t, data_ptr, readable bytes, pitch, frame stride, first, n)"""
    n, pitch, fs = int(t.shape[0]), int(t.stride(1)), int(t.stride(0)) if t.shape[0] > 1 else 0
    return (t, t.data_ptr(), (n - 1) * fs + (Hs + Hs // 2 - 1) * pitch + Ws, pitch, fs, first, n)


def _nv12_source(what: str, frames: Tensor, matrix: str):
    """Arguments common to the kernels that read NV12 frames (clips.py): frames uint8 [n, 3 Hs / 2, Ws] or [B, T, 3 Hs / 2, Ws]
    on the device.  The row pitch and the frame stride are the tensor's strides; only a non-contiguous last dimension is
    copied.  -> (n frames, T or None, Hs, Ws, coefficients as a C array, launches), launches = [(tensor that keeps the memory
    alive, data_ptr, readable bytes, pitch, frame stride, first frame, frames)]: one launch, or one per clip when the clip
    stride of a 4-D batch is not T frame strides."""
    if torch.is_tensor(frames) and frames.dtype != torch.uint8:
        raise TypeError('%s: frames must be uint8, got %s' % (what, frames.dtype))
    if not torch.is_tensor(frames) or frames.dim() not in (3, 4):
        raise RuntimeError('%s expects NV12 (n, 3 * Hs / 2, Ws) or (B, T, 3 * Hs / 2, Ws) uint8 input, got %s'
                           % (what, tuple(frames.shape) if torch.is_tensor(frames) else type(frames).__name__))
    if frames.numel() == 0:
        raise RuntimeError('%s: empty input %s' % (what, tuple(frames.shape)))
    if frames.stride(-1) != 1:
        frames = frames.contiguous()
    Hs, Ws = clips.check_nv12(frames)
    if Hs > 16384 or Ws > 16384:
        raise ValueError('%s: frames of at most 16384 x 16384, got %d x %d' % (what, Hs, Ws))
    coef = (ctypes.c_int * 6)(*clips.nv12_coefficients(matrix))
    _req(frames, 'frames')             # after the argument errors, which need no device
    rows, pitch = Hs + Hs // 2, int(frames.stride(-2))
    if pitch > (1 << 20):
        raise ValueError('%s: a row pitch of at most 2^20 bytes, got %d' % (what, pitch))
    n = frames.numel() // (rows * Ws)
    if frames.dim() == 3:
        return n, None, Hs, Ws, coef, [_nv12_launch(frames, 0, Hs, Ws)]
    B, T = int(frames.shape[0]), int(frames.shape[1])
    if B == 1 or T == 1 or frames.stride(0) == T * frames.stride(1):
        flat = frames[0] if B == 1 else frames[:, 0] if T == 1 else frames.as_strided((B * T, rows, Ws), (frames.stride(1), pitch, 1))
        return n, T, Hs, Ws, coef, [_nv12_launch(flat, 0, Hs, Ws)]
    return n, T, Hs, Ws, coef, [_nv12_launch(frames[b], b * T, Hs, Ws) for b in range(B)]


def _nv12_launches(launches, *per_frame):
    """every launch of _nv12_source -> (data_ptr, readable bytes, pitch, frame stride, frames k, the k rows of each per-frame
    tensor that belong to it)"""
    for _, ptr, total, pitch, fs, first, k in launches:
        yield (ptr, total, pitch, fs, k) + tuple(t[first:first + k] for t in per_frame)


def _side(what: str, S, noun: str = 'output side') -> int:
    S = int(S)
    if S < 1 or S > 480:
        raise ValueError('%s: the %s must lie in [1, 480], got %d' % (what, noun, S))
    return S


# the per-frame tables: (what a refusal calls it, dtype, shape of a row)
_BOXES = ('box table', torch.int32, (4,))
_SIMILARITIES = ('table of similarities', torch.float32, (2, 3))
_QUALITIES = ('quality table', torch.int32, ())
_PERTURBATIONS = ('table', torch.int32, (4,))
_PASTE_A = ('A', torch.float64, (2, 3))
_PASTE_RECT = ('rect', torch.int32, (4,))


def _frame_table(what: str, kind, table, n: int, T: Optional[int], device, checked: bool, check, host_only: Optional[str] = None):
    """The device table of a routine, one row for each of the n frames.  checked=True: the caller's device table as it is
    (dtype, shape and device looked at, nothing read back).  Otherwise check(table, rows) validates the host table
    (clips.check_*) of n rows or, for clips (T not None), n / T rows spread over the T frames of each clip, and the result is
    uploaded.  host_only: the refusal of an unchecked device table, whose validation would wait for the device; such a table
    is uploaded without blocking."""
    noun, dtype, row = kind
    if checked:
        if not torch.is_tensor(table) or table.dtype != dtype or tuple(table.shape) != (n,) + row or table.device != device:
            raise RuntimeError('%s: a checked %s is %s %s on %s' % (what, noun, str(dtype)[6:], (n,) + row, device))
        return _c(table)
    if host_only is not None and torch.is_tensor(table) and table.is_cuda:
        raise RuntimeError(host_only)
    t = check(table, n if T is None else n // T)
    if T is not None:
        t = t.repeat_interleave(T, dim=0)
    return t.contiguous().to(device, non_blocking=host_only is not None)


def _u8_out(what: str, frames: Tensor, shape, out: Optional[Tensor]) -> Tensor:
    """the uint8 result of the byte-image routines: a new tensor of `shape` on the frames' device, or the caller's `out`"""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=frames.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != frames.device or not out.is_contiguous():
        raise RuntimeError('%s: out must be contiguous uint8 %s on %s' % (what, tuple(shape), frames.device))
    return out


def _no_overlap(what: str, out: Tensor, ptr: int, nbytes: int, source: str) -> None:
    """`out` may not share memory with the nbytes the kernel reads at ptr"""
    if out.data_ptr() < ptr + nbytes and ptr < out.data_ptr() + out.numel():
        raise RuntimeError('%s: out may not share memory with the %s' % (what, source))


# the file decoders' share of the front end (jpeg_decode_u8, png_decode_u8, jpeg_decode_indexed_u8, jpeg_decode_drawn_u8)
def _packed(what: str, batch, checked: bool, cls, pack, *how):
    """The `batch` of a file decoder -> a packed batch: a `cls` as it is; with checked=True nothing else is taken; a sequence
    of files (bytes), not empty, is packed here by pack(files, *how)."""
    if isinstance(batch, cls):
        return batch
    if checked:
        raise RuntimeError('%s: checked=True takes a clips.%s (clips.%s packs and validates the files)' % (what, cls.__name__, pack.__name__))
    if isinstance(batch, (bytes, bytearray)) or not hasattr(batch, '__len__'):
        raise TypeError('%s expects a sequence of files (bytes) or a clips.%s, got %s' % (what, cls.__name__, type(batch).__name__))
    if len(batch) == 0:
        raise RuntimeError('%s: empty input (no files)' % what)
    return pack(batch, *how)


def _decode_device(what: str, out: Optional[Tensor]):
    """where a batch of files is decoded: on the device of a given `out`, else on the current one"""
    if not torch.cuda.is_available():
        raise RuntimeError('istvt_amd: %s needs a ROCm device (no CPU fallback exists for the ISTVT hot path)' % what)
    return out.device if out is not None and out.is_cuda else torch.device('cuda', torch.cuda.current_device())


def _canvas(what: str, Hmax: int, Wmax: int, canvas, whose: str = ''):
    """canvas = (Hc, Wc), by default Hmax x Wmax: it holds every image (`whose`: ' of the bank') and is at most 16384 x 16384"""
    Hc, Wc = (Hmax, Wmax) if canvas is None else (int(canvas[0]), int(canvas[1]))
    if Hc < Hmax or Wc < Wmax or Hc > 16384 or Wc > 16384:
        raise ValueError('%s: the canvas must hold every image%s (%d x %d at least, 16384 x 16384 at most), got %d x %d'
                         % (what, whose, Hmax, Wmax, Hc, Wc))
    return Hc, Wc


def _decode_buffers(what: str, device, n: int, need: int, buffers, hint: str = '', short=None):
    """(scratch, sizes, status) of a decode of n images: made here, or the caller's `buffers` checked -- contiguous on
    `device`, a uint8 scratch of `need` bytes (`hint` says more about them) at a multiple of 16, int32 sizes (n, 2) and status
    (n,).  short = (bytes, message with a %d): what a refused scratch of at least that many bytes is told instead."""
    if buffers is None:
        return (torch.empty((need,), dtype=torch.uint8, device=device), torch.empty((n, 2), dtype=torch.int32, device=device),
                torch.empty((n,), dtype=torch.int32, device=device))
    scratch, sizes, status = buffers
    ok = (t.device == device and t.is_contiguous() for t in buffers)
    if (not all(ok) or scratch.dtype != torch.uint8 or scratch.numel() < need or scratch.data_ptr() % 16
            or sizes.dtype != torch.int32 or tuple(sizes.shape) != (n, 2)
            or status.dtype != torch.int32 or tuple(status.shape) != (n,)):
        if short is not None and torch.is_tensor(scratch) and short[0] <= scratch.numel() < need:
            raise RuntimeError(short[1] % scratch.numel())
        raise RuntimeError('%s: buffers = (uint8 scratch of %d bytes%s, 16-byte aligned; int32 sizes (%d, 2); int32 '
                           'status (%d,)), contiguous on %s' % (what, need, hint, n, n, device))
    return scratch, sizes, status


def _decode_args(dev, host_or_index: Tensor, scratch: Tensor, out: Tensor, sizes: Tensor, status: Tensor, n: int, nseg: int,
                 nq: int, nh: int, nbytes: int, Hc: int, Wc: int, segments_host: Optional[Tensor] = None):
    """The argument block of a decode.  dev: the uploaded tensors, .data and whichever of .images .segments .qtabs .htabs the
    entry reads; host_or_index: what the entry reads through images_host (include/istvt_hip.h)."""
    at = lambda name: getattr(dev, name).data_ptr() if hasattr(dev, name) else None
    return _lib.JpegDecodeArgs(bytes=dev.data.data_ptr(), nbytes=nbytes, images=at('images'), images_host=host_or_index.data_ptr(),
                               segments=at('segments'), segments_host=None if segments_host is None else segments_host.data_ptr(),
                               qtabs=at('qtabs'), htabs=at('htabs'), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(),
                               out=out.data_ptr(), sizes=sizes.data_ptr(), status=status.data_ptr(), stream=_stream(), n=n,
                               nseg=nseg, nq=nq, nh=nh, Hc=Hc, Wc=Wc)


def _call(name: str, nbytes: int, *cargs) -> None:
    """one call of the library's entry `name` (istvt_...), recorded under its name without the prefix"""
    with prof(name[6:], nbytes):
        _lib.check(getattr(_lib.lib(), name)(*cargs), name)


# ---- crops and warps ---------------------------------------------------------------------------------------------------------
def crop_resize_u8(frames: Tensor, boxes: Tensor, S: int, out: Optional[Tensor] = None, checked: bool = False) -> Tensor:
    """Frames and boxes (clips.py): frames uint8 [n,Hs,Ws,3] or [B,T,Hs,Ws,3] on the device, boxes int32 [n,4] = (y0, x0, h,
    w) per frame or, for clips, [B,4] spread over the T frames of a clip -> uint8 [n,S,S,3] / [B,T,S,S,3]: every box cut out
    and resized with the antialiased bilinear filter of clips.crop_resize_host.  Boxes are validated on the host
    (clips.check_boxes) before any launch and then uploaded; checked=True takes a per-frame device table the caller has
    validated already.  `out` (uint8, contiguous, of the result's shape) is written when given."""
    n, T, Hs, Ws = _rgb_source('crop_resize_u8', frames)
    S = _side('crop_resize_u8', S)
    src = _c(frames)
    bdev = _frame_table('crop_resize_u8', _BOXES, boxes, n, T, frames.device, checked,
                        lambda b, rows: clips.check_boxes(b, rows, Hs, Ws, S))
    out = _u8_out('crop_resize_u8', frames, tuple(frames.shape[:-3]) + (S, S, 3), out)
    with prof('crop_resize_u8', n * S * S * 3):        # + the boxes' areas * 3, which live on the device
        _lib.check(_lib.lib().istvt_crop_resize_u8(src.data_ptr(), src.numel(), Hs, Ws, bdev.data_ptr(), out.data_ptr(), n, S,
                                                   _stream()), 'istvt_crop_resize_u8')
    return out


def nv12_to_rgb_u8(frames: Tensor, matrix: str = 'bt709', out: Optional[Tensor] = None) -> Tensor:
    """NV12 frames (clips.py) -> packed RGB: frames uint8 [n, 3 Hs / 2, Ws] or [B, T, 3 Hs / 2, Ws] on the device, the row
    pitch and the frame stride taken from the tensor's strides (a decoder surface wrapped with as_strided is read where it
    lies) -> uint8 [n, Hs, Ws, 3] / [B, T, Hs, Ws, 3], the bits of clips.nv12_to_rgb_host.  matrix: 'bt601', 'bt709' (limited
    range) or 'jfif' (full range).  `out` (uint8, contiguous, of the result's shape, no overlap with the frames) is written
    when given."""
    n, _, Hs, Ws, coef, launches = _nv12_source('nv12_to_rgb_u8', frames, matrix)
    out = _u8_out('nv12_to_rgb_u8', frames, tuple(frames.shape[:-2]) + (Hs, Ws, 3), out)
    for ptr, total, pitch, fs, k, rgb in _nv12_launches(launches, out.view((n, Hs, Ws, 3))):
        _no_overlap('nv12_to_rgb_u8', out, ptr, total, 'frames')
        with prof('nv12_to_rgb_u8', k * Hs * Ws * 9 // 2):
            _lib.check(_lib.lib().istvt_nv12_to_rgb_u8(ptr, total, Hs, Ws, pitch, fs, coef, rgb.data_ptr(), k, _stream()),
                       'istvt_nv12_to_rgb_u8')
    return out


def crop_resize_nv12(frames: Tensor, boxes: Tensor, S: int, matrix: str = 'bt709', out: Optional[Tensor] = None,
                     checked: bool = False) -> Tensor:
    """crop_resize_u8 from NV12 frames (clips.py): frames uint8 [n, 3 Hs / 2, Ws] or [B, T, 3 Hs / 2, Ws] on the device (pitch
    and frame stride from the tensor's strides, nothing copied unless the last dimension is not contiguous), boxes, S, `out`
    and `checked` as crop_resize_u8 takes them, the boxes in pixels of the Hs x Ws picture -> uint8 [n, S, S, 3] /
    [B, T, S, S, 3]: the bits of crop_resize_u8(nv12_to_rgb_u8(frames, matrix), boxes, S) without the RGB frames -- the colour
    conversion runs on the rows of the box only, inside the crop kernel."""
    n, T, Hs, Ws, coef, launches = _nv12_source('crop_resize_nv12', frames, matrix)
    S = _side('crop_resize_nv12', S)
    bdev = _frame_table('crop_resize_nv12', _BOXES, boxes, n, T, frames.device, checked,
                        lambda b, rows: clips.check_boxes(b, rows, Hs, Ws, S))
    out = _u8_out('crop_resize_nv12', frames, tuple(frames.shape[:-2]) + (S, S, 3), out)
    for ptr, total, pitch, fs, k, b, crops in _nv12_launches(launches, bdev, out.view((n, S, S, 3))):
        with prof('crop_resize_nv12', k * S * S * 3):  # + the boxes' areas * 3 / 2, which live on the device
            _lib.check(_lib.lib().istvt_crop_resize_nv12(ptr, total, Hs, Ws, pitch, fs, coef, b.data_ptr(), crops.data_ptr(), k, S,
                                                         _stream()), 'istvt_crop_resize_nv12')
    return out


def warp_similarity_u8(frames: Tensor, M: Tensor, S: int, out: Optional[Tensor] = None, checked: bool = False) -> Tensor:
    """Aligned crops (clips.py): frames uint8 [n,Hs,Ws,3] or [B,T,Hs,Ws,3] on the device, M float32 [n,2,3] per frame or, for
    clips, [B,2,3] spread over the T frames of a clip: the similarity that takes the centre of an output pixel to source
    coordinates (pixel j covers [j, j + 1)) -> uint8 [n,S,S,3] / [B,T,S,S,3], every frame resampled through its map with the
    antialiased triangle of clips.warp_similarity_host, the border replicated.  The table is validated on the host
    (clips.check_similarities) before any launch and then uploaded; checked=True takes a per-frame device table the caller
    has validated already (an entry the kernel itself refuses gives a frame of zeros).  `out` (uint8, contiguous, of the
    result's shape) is written when given."""
    n, T, Hs, Ws = _rgb_source('warp_similarity_u8', frames)
    S = _side('warp_similarity_u8', S)
    src = _c(frames)
    mdev = _frame_table('warp_similarity_u8', _SIMILARITIES, M, n, T, frames.device, checked,
                        lambda m, rows: clips.check_similarities(m, rows, Hs, Ws, S))
    out = _u8_out('warp_similarity_u8', frames, tuple(frames.shape[:-3]) + (S, S, 3), out)
    with prof('warp_similarity_u8', n * S * S * 3):    # + the footprints' areas * 3, which live on the device
        _lib.check(_lib.lib().istvt_warp_similarity_u8(src.data_ptr(), src.numel(), Hs, Ws, mdev.data_ptr(), out.data_ptr(), n,
                                                       S, _stream()), 'istvt_warp_similarity_u8')
    return out


def warp_similarity_nv12(frames: Tensor, M: Tensor, S: int, matrix: str = 'bt709', out: Optional[Tensor] = None,
                         checked: bool = False) -> Tensor:
    """warp_similarity_u8 from NV12 frames (clips.py): frames uint8 [n, 3 Hs / 2, Ws] or [B, T, 3 Hs / 2, Ws] on the device
    (pitch and frame stride from the tensor's strides, as crop_resize_nv12 takes them), M, S, `out` and `checked` as
    warp_similarity_u8 takes them, the maps in pixels of the Hs x Ws picture -> uint8 [n, S, S, 3] / [B, T, S, S, 3]: the bits of
    warp_similarity_u8(nv12_to_rgb_u8(frames, matrix), M, S) without the RGB frames -- a source pixel is converted once per
    output tile, inside the warp kernel."""
    n, T, Hs, Ws, coef, launches = _nv12_source('warp_similarity_nv12', frames, matrix)
    S = _side('warp_similarity_nv12', S)
    mdev = _frame_table('warp_similarity_nv12', _SIMILARITIES, M, n, T, frames.device, checked,
                        lambda m, rows: clips.check_similarities(m, rows, Hs, Ws, S))
    out = _u8_out('warp_similarity_nv12', frames, tuple(frames.shape[:-2]) + (S, S, 3), out)
    for ptr, total, pitch, fs, k, m, crops in _nv12_launches(launches, mdev, out.view((n, S, S, 3))):
        with prof('warp_similarity_nv12', k * S * S * 3):
            _lib.check(_lib.lib().istvt_warp_similarity_nv12(ptr, total, Hs, Ws, pitch, fs, coef, m.data_ptr(), crops.data_ptr(),
                                                             k, S, _stream()), 'istvt_warp_similarity_nv12')
    return out


def crop_frames(pixel_format: str, aligned: bool, frames: Tensor, table: Tensor, S: int, matrix: str = 'bt709',
                out: Optional[Tensor] = None, checked: bool = False) -> Tensor:
    """the crop of frames in `pixel_format` ('nv12', or packed RGB): a warp through similarities when `aligned`, boxes cut
    out and resized otherwise; `matrix` is read for NV12 frames only"""
    if pixel_format == 'nv12':
        return (warp_similarity_nv12 if aligned else crop_resize_nv12)(frames, table, S, matrix, out=out, checked=checked)
    return (warp_similarity_u8 if aligned else crop_resize_u8)(frames, table, S, out=out, checked=checked)


# ---- the relevance paste -----------------------------------------------------------------------------------------------------
def _paste_geometry(what: str, A, rect, n: int):
    """host A and rect as clips.paste_geometry makes them, validated: dtypes, shapes, every number of A finite, no negative
    extent -> (A, rect) on the host"""
    if not torch.is_tensor(A) or A.dtype != torch.float64:
        raise TypeError('%s: A must be a float64 tensor (n, 2, 3) as clips.paste_geometry makes it' % what)
    if not torch.is_tensor(rect) or rect.dtype != torch.int32:
        raise TypeError('%s: rect must be an int32 tensor (n, 4) as clips.paste_geometry makes it' % what)
    if tuple(A.shape) != (n, 2, 3) or tuple(rect.shape) != (n, 4):
        raise ValueError('%s: A (%d, 2, 3) and rect (%d, 4) expected, got %s and %s'
                         % (what, n, n, tuple(A.shape), tuple(rect.shape)))
    A, rect = A.detach().cpu(), rect.detach().cpu()
    if not bool(torch.isfinite(A).all()):
        raise ValueError('%s: every entry of A must be finite' % what)
    if bool((rect[:, 2:] < 0).any()):
        raise ValueError('%s: rect = (y0, x0, h, w) with h, w >= 0' % what)
    return A, rect


def _paste_tables(what: str, frames: Tensor, n: int, maps: Tensor, A: Tensor, rect: Tensor, lut: Tensor, alpha, S: int,
                  checked: bool):
    """the device tables of the two pastes -> (maps (n, g * g), g, A, rect, lut, alpha (n,), S).  A and rect: checked tables as
    they are, or host tables validated (_paste_geometry) and uploaded."""
    S = _side(what, S, 'crop side')
    if not torch.is_tensor(maps) or maps.dtype != torch.float32 or maps.dim() not in (2, 3) or maps.shape[0] != n:
        raise RuntimeError('%s: maps must be float32 (%d, g, g) or (%d, g * g), got %s'
                           % (what, n, n, (maps.dtype, tuple(maps.shape)) if torch.is_tensor(maps) else type(maps).__name__))
    g = int(maps.shape[1]) if maps.dim() == 3 else int(round(maps.shape[1] ** 0.5))
    if not 1 <= g <= 19 or maps.numel() != n * g * g:
        raise RuntimeError('%s: a square grid of at most 19 x 19 cells per map expected, got %s' % (what, tuple(maps.shape)))
    if not torch.is_tensor(lut) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise RuntimeError('%s: the colour table must be uint8 (256, 3)' % what)
    if maps.device != frames.device or lut.device != frames.device:
        raise RuntimeError('%s: frames, maps and the colour table must share one device' % what)
    if not checked:
        A, rect = _paste_geometry(what, A, rect, n)
    A = _frame_table(what, _PASTE_A, A, n, None, frames.device, checked, lambda t, rows: t)
    rect = _frame_table(what, _PASTE_RECT, rect, n, None, frames.device, checked, lambda t, rows: t)
    if torch.is_tensor(alpha):
        if alpha.dtype != torch.float32 or tuple(alpha.shape) != (n,):
            raise RuntimeError('%s: alpha is a float or a float32 tensor (%d,), got %s %s'
                               % (what, n, alpha.dtype, tuple(alpha.shape)))
        alpha = alpha.to(frames.device, non_blocking=True)
    else:
        alpha = float(alpha)
        if alpha != alpha or alpha in (float('inf'), float('-inf')):
            raise ValueError('%s: alpha must be finite, got %r' % (what, alpha))
        alpha = torch.full((n,), alpha, dtype=torch.float32, device=frames.device)
    return _c(maps).view(n, g * g), g, A, rect, _c(lut), _c(alpha), S


def _paste_target(what: str, frames: Tensor, out: Optional[Tensor], inplace: bool) -> Tensor:
    """what a paste writes: the frames themselves (inplace), or a copy of them in `out` or in a new tensor"""
    if inplace:
        return frames
    out = _u8_out(what, frames, tuple(frames.shape), out)
    out.copy_(frames)
    return out


def relevance_paste_u8(frames: Tensor, maps: Tensor, A: Tensor, rect: Tensor, lut: Tensor, alpha, S: int,
                       out: Optional[Tensor] = None, inplace: bool = False, checked: bool = False) -> Tensor:
    """Relevance maps pasted onto whole frames (clips.paste_maps_host is the definition): frames uint8 [n,Hs,Ws,3] on the
    device, maps float32 [n,g,g] or [n,g*g] (g <= 19, crop coordinates), A float64 [n,2,3] and rect int32 [n,4] as
    clips.paste_geometry makes them for crops of side S, lut uint8 [256,3], alpha a float or float32 [n] -> the frames with
    every map coloured through the table and blended over its face.  A and rect are host tables, validated here and
    uploaded; checked=True takes device tables as they are (the kernel clamps a rectangle into its frame and leaves a frame
    with a non-finite A, alpha or map untouched).  inplace=True writes into `frames` (contiguous) and costs the rectangles'
    area; otherwise the frames are copied once, into `out` when given, and the same launch runs on the copy."""
    n, _, Hs, Ws = _rgb_source('relevance_paste_u8', frames, clips_too=False)
    maps, g, A, rect, lut, alpha, S = _paste_tables('relevance_paste_u8', frames, n, maps, A, rect, lut, alpha, S, checked)
    if inplace and (out is not None or not frames.is_contiguous()):
        raise RuntimeError('relevance_paste_u8: inplace=True writes into contiguous frames and takes no out')
    out = _paste_target('relevance_paste_u8', frames, out, inplace)
    with prof('relevance_paste_u8', n * g * g * 4):    # + twice the rectangles' areas * 3, which live on the device
        _lib.check(_lib.lib().istvt_relevance_paste_u8(out.data_ptr(), out.numel(), Hs, Ws, maps.data_ptr(), g, A.data_ptr(),
                                                       rect.data_ptr(), lut.data_ptr(), alpha.data_ptr(), n, S, _stream()),
                   'istvt_relevance_paste_u8')
    return out


def relevance_paste_nv12(frames: Tensor, maps: Tensor, A: Tensor, rect: Tensor, lut_ycc: Tensor, alpha, S: int,
                         out: Optional[Tensor] = None, inplace: bool = False, checked: bool = False) -> Tensor:
    """relevance_paste_u8 on NV12 frames (clips.py): frames uint8 [n, 3 Hs / 2, Ws] on the device, the pitch and the frame
    stride taken from the tensor's strides; lut_ycc uint8 [256,3] holds (Y, Cb, Cr) per entry (clips.lut_to_ycc of the RGB
    table in the frames' matrix); A and rect in pixels of the Hs x Ws picture, rect from paste_geometry(even=True).  The blend
    runs in the frame's own colour space: no pixel is converted.  inplace=True writes the surface where it lies (frames that
    do not overlap); otherwise -> a contiguous copy with the maps pasted on."""
    if inplace and (not torch.is_tensor(frames) or frames.dim() != 3 or frames.stride(-1) != 1):
        raise RuntimeError('relevance_paste_nv12: inplace=True takes (n, 3 * Hs / 2, Ws) frames with contiguous rows')
    if torch.is_tensor(frames) and frames.dim() != 3:
        raise RuntimeError('relevance_paste_nv12 expects NV12 (n, 3 * Hs / 2, Ws) uint8 input, got %s' % (tuple(frames.shape),))
    n, _, Hs, Ws, _, _ = _nv12_source('relevance_paste_nv12', frames, 'bt709')
    maps, g, A, rect, lut, alpha, S = _paste_tables('relevance_paste_nv12', frames, n, maps, A, rect, lut_ycc, alpha, S, checked)
    if inplace and out is not None:
        raise RuntimeError('relevance_paste_nv12: inplace=True takes no out')
    out = _paste_target('relevance_paste_nv12', frames, out, inplace)
    _, ptr, total, pitch, fs, _, _ = _nv12_launch(out, 0, Hs, Ws)
    if n > 1 and fs < total - (n - 1) * fs:            # a frame's own bytes reach into the next frame
        raise RuntimeError('relevance_paste_nv12: the frames of a batch written in place may not overlap')
    with prof('relevance_paste_nv12', n * g * g * 4):  # + twice the rectangles' areas * 3 / 2, which live on the device
        _lib.check(_lib.lib().istvt_relevance_paste_nv12(ptr, total, Hs, Ws, pitch, fs, maps.data_ptr(), g, A.data_ptr(),
                                                         rect.data_ptr(), lut.data_ptr(), alpha.data_ptr(), n, S, _stream()),
                   'istvt_relevance_paste_nv12')
    return out


def paste_maps(pixel_format: str, frames: Tensor, maps: Tensor, A: Tensor, rect: Tensor, lut: Tensor, alpha, S: int,
               **kw) -> Tensor:
    """the paste onto frames in `pixel_format` ('nv12', or packed RGB); lut in the frames' colour space"""
    return (relevance_paste_nv12 if pixel_format == 'nv12' else relevance_paste_u8)(frames, maps, A, rect, lut, alpha, S, **kw)


# ---- degradations ------------------------------------------------------------------------------------------------------------
def jpeg_roundtrip_u8(frames: Tensor, quality, subsampling: str = '420', out: Optional[Tensor] = None,
                      checked: bool = False) -> Tensor:
    """JPEG round trip (clips.py): frames uint8 [n,H,W,3] or [B,T,H,W,3] on the device, quality int32 [n] per frame or, for
    clips, [B] shared by the T frames of a clip (or an int for all) -> uint8 of the same shape: what a baseline JPEG encoder
    and decoder hand back at that quality ('420' or '444' chroma), the bits of clips.jpeg_roundtrip_host.  Entries 1..100
    compress, an entry <= 0 copies its frame.  A host table is validated (clips.check_qualities) before any launch and
    uploaded without blocking; checked=True takes a per-frame device table the caller has validated already and reads nothing
    back.  A device table without checked=True is refused: validating it would copy it back and wait for the device.  `out`
    (uint8, contiguous, of the input's shape) is written when given; it may not share memory with the input, whose
    neighbouring blocks the chroma upsample reads."""
    n, T, H, W = _rgb_source('jpeg_roundtrip_u8', frames, contiguous=True)
    sub = clips._jpeg_sub(subsampling)
    qdev = _frame_table('jpeg_roundtrip_u8', _QUALITIES, quality, n, T, frames.device, checked, clips.check_qualities,
                        'jpeg_roundtrip_u8: a device quality table is taken with checked=True only (int32, one entry per '
                        'frame, validated by the caller); hand over the host table otherwise')
    out = _u8_out('jpeg_roundtrip_u8', frames, frames.shape, out)
    nbytes = frames.numel()
    _no_overlap('jpeg_roundtrip_u8', out, frames.data_ptr(), nbytes, 'input (the round trip is not done in place)')
    mcu = 8 * sub
    Hp, Wp = -(-H // mcu) * mcu, -(-W // mcu) * mcu
    planes = torch.empty((n * Hp * Wp * 3 // (2 if sub == 2 else 1),), dtype=torch.uint8, device=frames.device)
    with prof('jpeg_roundtrip_u8', 2 * nbytes + 2 * planes.numel()):
        _lib.check(_lib.lib().istvt_jpeg_roundtrip_u8(frames.data_ptr(), nbytes, n, H, W, qdev.data_ptr(), 2 if sub == 2 else 0,
                                                      planes.data_ptr(), planes.numel(), out.data_ptr(), _stream()),
                   'istvt_jpeg_roundtrip_u8')
    return out


def _jpeg_split(batch, split):
    """the `split` argument of jpeg_decode_u8 -> the chunk size of the split entropy kernel, or None for the one lane per
    restart interval"""
    if split is None:
        return None
    if split == 'auto':
        longest = int((batch.segments[:, 2] - batch.segments[:, 1]).max())
        return clips.JPEG_SPLIT_DEFAULT if longest > clips.JPEG_SPLIT_AUTO_BYTES else None
    if isinstance(split, bool) or not isinstance(split, int) or split < clips.JPEG_SPLIT_MIN:
        raise ValueError("jpeg_decode_u8: split is None, 'auto' or a chunk size in bytes (an int of at least %d), got %r"
                         % (clips.JPEG_SPLIT_MIN, split))
    return split


def jpeg_decode_u8(batch, canvas=None, out: Optional[Tensor] = None, checked: bool = False, buffers=None, split=None,
                   layouts=clips.JPEG_LAYOUTS_DEFAULT):
    """JPEG files (clips.py): a batch of baseline JPEG files goes to the device as compressed bytes -> (frames, sizes,
    status): frames uint8 [n, Hc, Wc, 3], image i in the top left H_i x W_i of its canvas and 0 elsewhere, the bits of
    clips.jpeg_decode_host; sizes int32 [n, 2] = (H, W) and status int32 [n] (0: fine; clips.jpeg_decode_host lists the
    rest) on the device.  Nothing is decoded on the host and nothing synchronises: clips.check_jpeg_status(status) reads
    back and raises, for callers who want that.  batch: a sequence of bytes, parsed and packed here (clips.jpeg_batch, which
    refuses what the decoder does not take), or with checked=True a clips.JpegBatch the caller has packed already (the
    loader's worker); its tables are uploaded once per device and kept on it.  canvas = (Hc, Wc) defaults to the largest
    H and W of the batch.  `out` (uint8, contiguous, of the result's shape, no overlap with the uploaded bytes) is written
    when given.  buffers = (scratch uint8 of at least batch.scratch_bytes bytes and 16-byte aligned, sizes, status): the
    caller's, to decode step after step without an allocation.  split: how a restart interval is decoded.  None: by one
    lane, which suits files with a restart marker per MCU row.  A chunk size in bytes (an int of at least 16): by one lane
    per chunk, which start from guessed decoder states and relax them to the sequential decoder's (clips.jpeg_split_host) --
    for files without restart markers, as cameras and most encoders write them; the same bytes come out.  'auto': chunks
    of clips.JPEG_SPLIT_DEFAULT bytes where some interval of the batch is longer than clips.JPEG_SPLIT_AUTO_BYTES (the
    split has a cost: on intervals of one MCU row of a 224-pixel frame it is the slower of the two), else None.  With a split the
    scratch holds clips.jpeg_split_plan(batch, chunk).scratch_bytes.  layouts: what clips.jpeg_batch accepts when files are
    handed over, a tuple of names from clips.JPEG_LAYOUTS or 'all' (4:2:0, 4:4:4, 4:2:2 and greyscale files, mixed as they
    come); by default 4:2:0 and 4:4:4 alone.  A JpegBatch has been parsed already: the argument is not consulted for it."""
    if isinstance(batch, clips.JpegFiles):                        # the encoder's result: read back, then parsed like any files
        batch = batch.files()
    what = 'jpeg_decode_u8'
    batch = _packed(what, batch, checked, clips.JpegBatch, clips.jpeg_batch, layouts)
    chunk = _jpeg_split(batch, split)
    need = batch.scratch_bytes if chunk is None else clips.jpeg_split_plan(batch, chunk).scratch_bytes
    device = _decode_device(what, out)
    n = batch.n
    Hc, Wc = _canvas(what, max(h for h, _ in batch.sizes), max(w for _, w in batch.sizes), canvas)
    dev = batch.on(device)
    out = _u8_out(what, dev.data, (n, Hc, Wc, 3), out)
    _no_overlap(what, out, dev.data.data_ptr(), dev.data.numel(), 'uploaded files')
    scratch, sizes, status = _decode_buffers(what, device, n, need, buffers)
    args = _decode_args(dev, batch.images, scratch, out, sizes, status, n, int(batch.segments.shape[0]), int(batch.qtabs.shape[0]),
                        int(batch.htabs.shape[0]), batch.nbytes, Hc, Wc, segments_host=batch.segments)
    name, extra = ('istvt_jpeg_decode_u8', ()) if chunk is None else ('istvt_jpeg_decode_split_u8', (chunk,))
    _call(name, batch.nbytes + 2 * 192 * batch.blocks + out.numel(), ctypes.byref(args), *extra)
    return out, sizes, status


def png_decode_u8(batch, canvas=None, out: Optional[Tensor] = None, checked: bool = False, buffers=None, bands=None):
    """PNG files (clips.py): a batch of 8-bit grey, RGB or RGBA PNG files goes to the device as its DEFLATE streams ->
    (frames, sizes, status): frames uint8 [n, Hc, Wc, 3], image i in the top left H_i x W_i of its canvas and 0 elsewhere
    (grey replicated, alpha dropped), the bytes of clips.png_decode_host; sizes int32 [n, 2] = (H, W) and status int32 [n]
    (0: fine; clips.PNG_STATUS lists the rest, and such a file's canvas is all zeros) on the device.  Nothing is inflated on the
    host and nothing synchronises: clips.check_png_status(status) reads back and raises, for callers who want that.  batch: a
    sequence of bytes, parsed and packed here (clips.png_batch, which refuses what the decoder does not take), or with
    checked=True a clips.PngBatch the caller has packed already; its tensors are uploaded once per device and kept on it.
    canvas = (Hc, Wc) defaults to the largest H and W of the batch.  `out` (uint8, contiguous, of the result's shape, no
    overlap with the uploaded bytes) is written when given.  buffers = (scratch uint8 of at least batch.scratch_bytes bytes
    and 16-byte aligned, sizes, status): the caller's, to decode step after step without an allocation.
    bands='index' with a sequence of bytes packs it with clips.png_batch(bands='index'); a batch that carries bands, packed
    here or by the caller, is decoded one wave per band of the files' baND chunks (istvt_png_decode_bands_u8, the bytes and
    statuses of clips.png_decode_bands_host; status 7 is clips.PNG_BAND_STATUS's) and its scratch holds a status word per band
    behind the filtered rows.  A PngBatch is decoded as it was packed: bands= given with one must agree with it.
    A batch packed with clips.png_batch(bands='index', alone=True) (batch.alone is not None) goes to
    istvt_png_decode_alone_u8: the files whose index says their bands stand alone are unfiltered one wave per band too, the
    bytes and statuses of clips.png_decode_alone_host (status 10 is clips.PNG_ALONE_STATUS's); its flags are uploaded with the
    other tables, and the promises about `out` and `buffers` hold as before."""
    what = 'png_decode_u8'
    clips.check_png_bands(bands, what)
    if isinstance(batch, clips.PngBatch) and bands is not None and batch.bands is None:
        raise ValueError("png_decode_u8: bands='index' with a clips.PngBatch that was packed without bands "
                         "(clips.png_batch(files, bands='index') packs them)")
    batch = _packed(what, batch, checked, clips.PngBatch, clips.png_batch, bands)
    need = batch.scratch_bytes
    device = _decode_device(what, out)
    n = batch.n
    Hc, Wc = _canvas(what, max(h for h, _ in batch.sizes), max(w for _, w in batch.sizes), canvas)
    dev = batch.on(device)
    out = _u8_out(what, dev.data, (n, Hc, Wc, 3), out)
    _no_overlap(what, out, dev.data.data_ptr(), dev.data.numel(), 'uploaded files')
    name, nband, short = 'istvt_png_decode_u8', 0, None
    if batch.bands is not None:
        name, nband = 'istvt_png_decode_bands_u8', int(batch.bands.shape[0])
        extra = {}
        if batch.alone is not None:                               # the flags go where qtabs do, their host copy where htabs do
            name, extra = 'istvt_png_decode_alone_u8', dict(qtabs=dev.alone, htabs=batch.alone)
        dev = SimpleNamespace(data=dev.data, images=dev.images, segments=dev.bands, **extra)   # the band table goes where segments do
        # said to a scratch that holds the rows but not the band status words
        short = (n * batch.raw_stride, 'png_decode_u8: a batch with bands needs a scratch of %d bytes: %d of filtered rows and a '
                 'status word for each of its %d bands, got %%d' % (need, n * batch.raw_stride, nband))
    scratch, sizes, status = _decode_buffers(what, device, n, need, buffers, short=short)
    nflags = 0 if batch.alone is None else n
    args = _decode_args(dev, batch.images, scratch, out, sizes, status, n, nband, nflags, nflags, batch.nbytes, Hc, Wc,
                        segments_host=batch.bands)
    _call(name, batch.nbytes + 2 * batch.raw_bytes + out.numel(), ctypes.byref(args), batch.raw_stride)
    return out, sizes, status


def _bank_call(what: str, bank, m: int, device, canvas, out: Optional[Tensor], buffers, rows: Optional[int] = None):
    """What a decode of m places of a bank needs beside the index: the canvas, the uploaded bank, `out` and `buffers` checked
    or made -> (the bank on its device, Hc, Wc, out, scratch, sizes, status).  rows: the window height of a windowed decode of a
    clips.PngBank, whose canvas is rows x Wc and whose scratch is the window's (clips.png_window_scratch_bytes)."""
    Hc, Wc = _canvas(what, bank.Hmax, bank.Wmax, canvas, ' of the bank')
    if rows is not None:
        Hc = rows
    dev = bank.on(device)
    out = _u8_out(what, dev.data, (m, Hc, Wc, 3), out)
    _no_overlap(what, out, dev.data.data_ptr(), dev.data.numel(), "bank's files")
    if rows is not None:
        need = clips.png_window_scratch_bytes(bank, m, rows)
        layout = ' (clips.png_window_scratch_bytes: filtered rows, a status word per slot, moved boxes and origins)'
    elif isinstance(bank, clips.PngBank):
        need, layout = clips.png_bank_scratch_bytes(bank, m), ' (clips.png_bank_scratch_bytes: filtered rows and a status word per band)'
    else:
        need = clips.jpeg_bank_scratch_bytes(bank, m)
        layout = '' if bank.split is None else ' for the split layout (bank.split = %d: %d state rows per segment)' \
            % (bank.split, bank.chunk_rows)
    scratch, sizes, status = _decode_buffers(what, dev.data.device, m, need, buffers, layout)
    return dev, Hc, Wc, out, scratch, sizes, status


def _bank_decode(name: str, bank, index: Tensor, head, dev, Hc: int, Wc: int, out: Tensor, scratch: Tensor, sizes: Tensor,
                 status: Tensor):
    """The call behind _bank_call: the bank's entry istvt_jpeg_decode_<name>_u8, which reads the index at `index` and takes the
    scalars `head` in front of the bank's, or for a bank with a split its _split sibling, which takes chunk_bytes,
    chunk_rows and seg_bytes_max (-1: no limit on a segment's length) behind them -> (out, sizes, status)"""
    args = _decode_args(dev, index, scratch, out, sizes, status, bank.n, bank.nseg, bank.nq, bank.nh, bank.nbytes, Hc, Wc)
    tail = (bank.seg_max, bank.block_stride, bank.Hmax, bank.Wmax)
    if bank.split is not None:
        name += '_split'
        tail += (bank.split, bank.chunk_rows, -1 if bank.seg_bytes_max is None else min(int(bank.seg_bytes_max), 2 ** 31 - 1))
    # the bytes: + those drawn, known on the device
    _call('istvt_jpeg_decode_%s_u8' % name, 2 * 192 * out.shape[0] * bank.block_stride + out.numel(), ctypes.byref(args), *head, *tail)
    return out, sizes, status


def jpeg_decode_indexed_u8(bank, index, canvas=None, out: Optional[Tensor] = None, buffers=None, split=None):
    """JPEG bank (clips.py): the files of a clips.JpegBank stay on the device, and the m of them that `index` names are
    decoded, in that order and with repeats -> (frames, sizes, status) as jpeg_decode_u8 hands them back, the bits of
    clips.jpeg_bank_decode_host: frames uint8 [m, Hc, Wc, 3], sizes int32 [m, 2], status int32 [m]; a place whose index is
    outside the bank has status 4, one whose file the device ingest could not read status 5, both with size (0, 0) and a
    frame of zeros.  index: int32 or int64, one dimension, contiguous, on the device (torch.randint there) -- then no host
    data is part of the call, nothing synchronises, and the call can be captured in a graph with `out` and `buffers` -- or
    a host tensor or list, which is uploaded.  int64 is narrowed on the device.  The bank is uploaded at the first call
    (bank.on).  canvas = (Hc, Wc) defaults to the bank's largest H and W, whatever is drawn.  buffers = (scratch uint8 of
    clips.jpeg_bank_scratch_bytes(bank, m) bytes and 16-byte aligned, sizes, status).  How the intervals are decoded is the
    bank's property: with bank.split set (clips.jpeg_bank(files, split=), bank.with_split) the split entropy kernel runs, one
    lane per chunk with its state rows at a stride per drawn segment, for files without restart markers; the same bytes come
    out, and the scratch is larger.  The call's own split= is refused: the chunk size fixes the scratch layout and the
    workgroup size, which must not change from call to call."""
    if not isinstance(bank, clips.JpegBank):
        raise TypeError('jpeg_decode_indexed_u8 expects a clips.JpegBank (clips.jpeg_bank, clips.JpegBank.from_encoded), got %s'
                        % type(bank).__name__)
    if split is not None:
        raise ValueError('jpeg_decode_indexed_u8: split= is not available for a bank (the state rows of the split kernel are '
                         'addressed over the whole byte range, which here is the whole set): the split is a property of the '
                         'bank, clips.jpeg_bank(files, split=) or bank.with_split(split)')
    index = clips.check_bank_index(index, 'jpeg_decode_indexed_u8')
    if not torch.cuda.is_available():
        raise RuntimeError('istvt_amd: jpeg_decode_indexed_u8 needs a ROCm device (no CPU fallback exists for the ISTVT hot path)')
    device = torch.device(bank.device) if bank.device is not None else index.device if index.is_cuda else \
        out.device if out is not None and out.is_cuda else torch.device('cuda', torch.cuda.current_device())
    m = int(index.numel())
    front = _bank_call('jpeg_decode_indexed_u8', bank, m, device, canvas, out, buffers)
    on = front[0].data.device
    if index.device != on:
        index = index.to(on, non_blocking=True)
    if index.dtype != torch.int32:                                # -1 and n are outside the bank as everything beyond them is
        index = index.clamp(-1, bank.n).to(torch.int32)
    return _bank_decode('indexed', bank, index, (m,), *front)


# ---- batch draw ----------------------------------------------------------------------------------------------------------------
def _drawn_plan(what: str, plan) -> 'clips.BatchPlan':
    if not isinstance(plan, clips.BatchPlan):
        raise TypeError('%s expects a clips.BatchPlan, got %s' % (what, type(plan).__name__))
    if plan.block is None or not plan.block.is_cuda:
        raise RuntimeError('%s: the plan is drawn from where its draw block lives: upload it first, plan.on(device)' % what)
    return plan


def batch_draw(plan):
    """Batch draw (clips.py): the tables of the batch of the plan's current step, drawn on the device into the plan's draw
    block, and the step advanced there -> plan.draw, the namespace of int32 device views index (B*T,), boxes (B*T, 4), quality
    (B*T,), view (B, 3), perturb (B, 4), label (B,), status (1,) (0: drawn; clips.DRAW_STATUS names the refusals, which leave
    tables and step as they were) and drawn (2,), the step as two words.  The bits of clips.batch_draw_host(plan, step).  One
    launch of one workgroup; no synchronisation, no allocation and no host read, so the call can be captured in a graph, and
    every replay draws the next step.  The views are the same tensors at every call: crop_resize_u8, jpeg_roundtrip_u8 and
    perturb_u8 take them with checked=True, jpeg_decode_indexed_u8 takes the index, and a source of raw uint8 clips can be
    gathered through it just as well."""
    plan = _drawn_plan('batch_draw', plan)
    args = _lib.JpegDecodeArgs(images_host=plan.block.data_ptr(), stream=_stream())
    with prof('batch_draw', 4 * plan.block.numel()):
        _lib.check(_lib.lib().istvt_batch_draw(ctypes.byref(args), plan.B, plan.T, plan.block.numel()), 'istvt_batch_draw')
    return plan.draw


def jpeg_decode_drawn_u8(bank, plan, canvas=None, out: Optional[Tensor] = None, buffers=None):
    """batch_draw(plan) and jpeg_decode_indexed_u8(bank, the index just drawn) as one call of five launches -> (frames, sizes,
    status, draw): frames uint8 [B*T, Hc, Wc, 3], sizes and status as the indexed decode hands them back, draw as batch_draw
    does.  The plan was built for this bank (as many places) and lives on its device.  canvas, out and buffers are
    jpeg_decode_indexed_u8's, for m = B * T; with out and buffers the call can be captured in a graph.  A bank with a split
    decodes through the split entropy kernel, as there."""
    if not isinstance(bank, clips.JpegBank):
        raise TypeError('jpeg_decode_drawn_u8 expects a clips.JpegBank, got %s' % type(bank).__name__)
    plan = _drawn_plan('jpeg_decode_drawn_u8', plan)
    if plan.N != bank.n:
        raise ValueError('jpeg_decode_drawn_u8: the plan was built for a bank of %d places, this one has %d' % (plan.N, bank.n))
    front = _bank_call('jpeg_decode_drawn_u8', bank, plan.B * plan.T, plan.block.device, canvas, out, buffers)
    if front[0].data.device != plan.block.device:
        raise RuntimeError('jpeg_decode_drawn_u8: the bank lives on %s, the plan on %s' % (front[0].data.device, plan.block.device))
    return _bank_decode('drawn', bank, plan.block, (plan.B, plan.T, plan.block.numel()), *front) + (plan.draw,)


def _png_bank_decode(name: str, bank, index: Tensor, head, dev, Hc: int, Wc: int, out: Tensor, scratch: Tensor, sizes: Tensor,
                     status: Tensor):
    """The call behind _bank_call for a clips.PngBank: the entry istvt_png_decode_<name>_u8, which reads the index at `index` and
    takes the scalars `head` in front of the bank's band_max and raw_stride -> (out, sizes, status).  A bank packed with
    clips.png_bank(alone=True) goes to the entry's _alone sibling (istvt_png_decode_bank_alone_u8, ..._bank_alone_drawn_u8)."""
    if bank.alone:
        name = name.replace('bank', 'bank_alone')
    args = _decode_args(dev, index, scratch, out, sizes, status, bank.n, bank.nband, 0, 0, bank.first_byte + bank.nbytes, Hc, Wc)
    # the bytes: + the streams drawn, known on the device
    _call('istvt_png_decode_%s_u8' % name, 2 * out.shape[0] * bank.raw_stride + out.numel(), ctypes.byref(args), *head, bank.band_max,
          bank.raw_stride)
    return out, sizes, status


def png_decode_bank_u8(bank, index, canvas=None, out: Optional[Tensor] = None, buffers=None):
    """PNG bank (clips.py): the files of a clips.PngBank stay on the device, and the m of them that `index` names are decoded
    by their bands, in that order and with repeats -> (frames, sizes, status) as png_decode_u8 hands them back, the bytes of
    clips.png_bank_decode_host: frames uint8 [m, Hc, Wc, 3], sizes int32 [m, 2], status int32 [m]; a place whose index is
    outside the bank has status 8, one whose rows on the device do not fit the call status 9 (clips.PNG_BANK_STATUS), both
    with size (0, 0) and a frame of zeros.  index: int32 or int64, one dimension, contiguous, on the device -- then no host
    data is part of the call, nothing synchronises, and the call can be captured in a graph with `out` and `buffers` -- or a
    host tensor or list, which is uploaded.  int64 is clamped to [-1, n] and narrowed on the device.  The bank is uploaded at
    the first call (bank.on); it may hold more than 2^31 bytes.  canvas = (Hc, Wc) defaults to the bank's largest H and W,
    whatever is drawn.  buffers = (scratch uint8 of clips.png_bank_scratch_bytes(bank, m) bytes and 16-byte aligned, sizes,
    status).  Two launches.  A bank packed with clips.png_bank(alone=True) is decoded by istvt_png_decode_bank_alone_u8: its
    flagged files are unfiltered one wave per band too (status 10 is clips.PNG_ALONE_STATUS's)."""
    what = 'png_decode_bank_u8'
    if not isinstance(bank, clips.PngBank):
        raise TypeError('%s expects a clips.PngBank (clips.png_bank), got %s' % (what, type(bank).__name__))
    index = clips.check_bank_index(index, what)
    if not torch.cuda.is_available():
        raise RuntimeError('istvt_amd: %s needs a ROCm device (no CPU fallback exists for the ISTVT hot path)' % what)
    device = index.device if index.is_cuda else out.device if out is not None and out.is_cuda else \
        torch.device('cuda', torch.cuda.current_device())
    m = int(index.numel())
    front = _bank_call(what, bank, m, device, canvas, out, buffers)
    on = front[0].data.device
    if index.device != on:
        index = index.to(on, non_blocking=True)
    if index.dtype != torch.int32:                                # -1 and n are outside the bank as everything beyond them is
        index = index.clamp(-1, bank.n).to(torch.int32)
    return _png_bank_decode('bank', bank, index, (m,), *front)


def png_decode_bank_drawn_u8(bank, plan, canvas=None, out: Optional[Tensor] = None, buffers=None):
    """batch_draw(plan) and png_decode_bank_u8(bank, the index just drawn) as one call of three launches -> (frames, sizes,
    status, draw): frames uint8 [B*T, Hc, Wc, 3], sizes and status as the bank decode hands them back, draw as batch_draw
    does.  The plan was built for this bank (as many places) and lives on its device.  canvas, out and buffers are
    png_decode_bank_u8's, for m = B * T; with out and buffers the call can be captured in a graph."""
    what = 'png_decode_bank_drawn_u8'
    if not isinstance(bank, clips.PngBank):
        raise TypeError('%s expects a clips.PngBank, got %s' % (what, type(bank).__name__))
    plan = _drawn_plan(what, plan)
    if plan.N != bank.n:
        raise ValueError('%s: the plan was built for a bank of %d places, this one has %d' % (what, plan.N, bank.n))
    front = _bank_call(what, bank, plan.B * plan.T, plan.block.device, canvas, out, buffers)
    return _png_bank_decode('bank_drawn', bank, plan.block, (plan.B, plan.T, plan.block.numel()), *front) + (plan.draw,)


# ---- PNG windows ---------------------------------------------------------------------------------------------------------------
def _png_window_call(name: str, src, reads, head, boxes: Tensor, m: int, rows: int, dev, Hc: int, Wc: int, out: Tensor, scratch: Tensor,
                     sizes: Tensor, status: Tensor):
    """The call of a windowed decode of m places behind the front end: the entry istvt_png_decode_<name>_u8 with the boxes where
    qtabs go and `reads` (a batch's image table, a bank's index, a plan's draw block) where images_host goes -> (out, moved boxes,
    sizes, status, origin), the boxes and origins being views of the scratch"""
    win_bands, win_stride = clips.png_window_bands(src, rows), clips.png_window_stride(src, rows)
    if isinstance(src, clips.PngBank):
        tabs = SimpleNamespace(data=dev.data, images=dev.images, segments=dev.segments, qtabs=boxes)
        args = _decode_args(tabs, reads, scratch, out, sizes, status, src.n, src.nband, m, 0, src.first_byte + src.nbytes, Hc, Wc)
        tail = (src.band_max, src.raw_stride, win_bands, win_stride)
    else:                                                         # the flags' host copy goes where htabs do
        tabs = SimpleNamespace(data=dev.data, images=dev.images, segments=dev.bands, qtabs=boxes, htabs=src.alone)
        args = _decode_args(tabs, reads, scratch, out, sizes, status, m, int(src.bands.shape[0]), m, m, src.nbytes, Hc, Wc,
                            segments_host=src.bands)
        tail = (win_bands, win_stride)
    # the bytes: + the streams of the touched bands, known on the device
    _call('istvt_png_decode_%s_u8' % name, 2 * m * win_stride + out.numel(), ctypes.byref(args), *head, *tail)
    at = clips.png_window_boxes_at(src, m, rows)
    words = scratch[at:at + 20 * m].view(torch.int32)
    return out, words[:4 * m].view(m, 4), sizes, status, words[4 * m:]


def png_decode_window_u8(batch_or_bank, boxes, index=None, rows: Optional[int] = None, canvas_w: Optional[int] = None,
                         out: Optional[Tensor] = None, buffers=None):
    """PNG windows (clips.py): files whose bands stand alone are decoded through one box (y0, x0, h, w) per place, and only the
    bands a box touches are inflated and unfiltered -> (windows uint8 [m, rows, Wc, 3], moved_boxes int32 [m, 4], sizes int32
    [m, 2], status int32 [m], origin int32 [m]), the bytes of clips.png_bank_window_host: place j holds rows [origin, origin +
    the window's rows) of its image at its top, 0 elsewhere, and moved_boxes[j] is the box within it, so that
    crop_resize_u8(windows, moved_boxes, S, checked=True) is the crop of the whole frame through the box.  A place with a status
    (clips.PNG_STATUS and its siblings; 11 and 12 are clips.PNG_WINDOW_STATUS's) has a window of zeros and the box (0, 0, 1, 1):
    a black crop.  Damage in a band the box does not touch is not seen.  moved_boxes and origin are views of the scratch.
    batch_or_bank: a clips.PngBatch packed with clips.png_batch(files, bands='index', alone=True) whose files all carry the
    flag -- place j is file j, and boxes int32 [n, 4] live on the host or on the device -- or a clips.PngBank packed with
    clips.png_bank(files, alone=True) with `index` as png_decode_bank_u8 takes it; index and boxes may both live on the device,
    and `rows` is then required.  Host boxes (with a host index) are checked by name first (clips.check_png_window) and
    uploaded; rows=None then takes the smallest window that fits them.  canvas_w defaults to the widest image.  buffers =
    (scratch uint8 of clips.png_window_scratch_bytes(batch_or_bank, m, rows) bytes and 16-byte aligned, sizes, status): with
    `out`, `buffers`, and boxes and index on the device, nothing is allocated and nothing synchronises, and the call can be
    captured in a graph.  Two launches (istvt_png_decode_window_u8, istvt_png_decode_bank_window_u8)."""
    what = 'png_decode_window_u8'
    src = batch_or_bank
    boxes, rows, Wc = clips.check_png_window(src, boxes, index, rows, canvas_w, what)
    if isinstance(src, clips.PngBank):
        index = clips.check_bank_index(index, what)
        if not torch.cuda.is_available():
            raise RuntimeError('istvt_amd: %s needs a ROCm device (no CPU fallback exists for the ISTVT hot path)' % what)
        device = index.device if index.is_cuda else boxes.device if boxes.is_cuda else out.device if out is not None and out.is_cuda \
            else torch.device('cuda', torch.cuda.current_device())
        m = int(index.numel())
        front = _bank_call(what, src, m, device, (src.Hmax, Wc), out, buffers, rows=rows)
        on = front[0].data.device
        if index.device != on:
            index = index.to(on, non_blocking=True)
        if index.dtype != torch.int32:                            # -1 and n are outside the bank as everything beyond them is
            index = index.clamp(-1, src.n).to(torch.int32)
        boxes = _frame_table(what, _BOXES, boxes, m, None, on, boxes.is_cuda, lambda b, k: b)
        return _png_window_call('bank_window', src, index, (m,), boxes, m, rows, *front)
    device = boxes.device if boxes.is_cuda else _decode_device(what, out)
    n = src.n
    dev = src.on(device)
    out = _u8_out(what, dev.data, (n, rows, Wc, 3), out)
    _no_overlap(what, out, dev.data.data_ptr(), dev.data.numel(), 'uploaded files')
    scratch, sizes, status = _decode_buffers(what, device, n, clips.png_window_scratch_bytes(src, n, rows), buffers,
                                             ' (clips.png_window_scratch_bytes: filtered rows, a status word per slot, moved boxes '
                                             'and origins)')
    boxes = _frame_table(what, _BOXES, boxes, n, None, device, boxes.is_cuda, lambda b, k: b)
    return _png_window_call('window', src, src.images, (), boxes, n, rows, dev, rows, Wc, out, scratch, sizes, status)


def png_decode_bank_window_drawn_u8(bank, plan, rows: Optional[int] = None, canvas_w: Optional[int] = None,
                                    out: Optional[Tensor] = None, buffers=None):
    """batch_draw(plan) and png_decode_window_u8(bank, the boxes just drawn, the index just drawn) as one call of three launches
    -> (windows, moved_boxes, sizes, status, origin, draw): the first five as png_decode_window_u8 hands them back for m = B *
    T, draw as batch_draw does.  The bank was packed with clips.png_bank(files, alone=True); the plan was built for it and lives
    on its device.  rows defaults to clips.png_window_rows(bank, plan.max_side), which fits every box the plan draws; canvas_w,
    out and buffers are png_decode_window_u8's.  With out and buffers the call can be captured in a graph."""
    what = 'png_decode_bank_window_drawn_u8'
    if not isinstance(bank, clips.PngBank):
        raise TypeError('%s expects a clips.PngBank, got %s' % (what, type(bank).__name__))
    plan = _drawn_plan(what, plan)
    if plan.N != bank.n:
        raise ValueError('%s: the plan was built for a bank of %d places, this one has %d' % (what, plan.N, bank.n))
    if rows is None and bank.alone:
        rows = clips.png_window_rows(bank, plan.max_side)
    boxes, rows, Wc = clips.check_png_window(bank, plan.draw.boxes, plan.draw.index, rows, canvas_w, what)
    m = plan.B * plan.T
    front = _bank_call(what, bank, m, plan.block.device, (bank.Hmax, Wc), out, buffers, rows=rows)
    return _png_window_call('bank_window_drawn', bank, plan.block, (plan.B, plan.T, plan.block.numel()), boxes, m, rows, *front) \
        + (plan.draw,)


def draw_clips(bank, plan, S: int, out: Optional[Tensor] = None, window: bool = False):
    """The whole input side of a training step on the device: the batch of the plan's current step is drawn and decoded
    (jpeg_decode_drawn_u8; png_decode_bank_drawn_u8 for a clips.PngBank), every frame cut and resized through its drawn box (crop_resize_u8), recompressed at its clip's
    drawn quality (jpeg_roundtrip_u8; left out when the plan's jpeg is off) and perturbed by its clip's drawn row (perturb_u8
    with the plan's taps and its seed as the noise key; left out when the plan's perturb is off) -> (u8 [B, T, S, S, 3], view
    int32 [B, 3], label int32 [B], status int32 [B*T]), all on the device: the bytes of the same calls on the host tables of
    clips.batch_draw_host(plan, step).  The step is model(u8, view=view, view_checked=True, crop=S).  No host table, no
    upload, no synchronisation: with `out` (uint8, contiguous, of the result's shape) the call can be captured in a graph,
    and every replay gives the next batch.  view, label and the draw behind them are views of the plan's draw block, which
    the next draw overwrites.  window=True (a clips.PngBank packed with alone=True): the decode is
    png_decode_bank_window_drawn_u8, which inflates and unfilters only the bands each drawn box touches into a window of
    clips.png_window_rows(bank, plan.max_side) rows, and the crop reads the windows through the boxes moved into them: the
    same bytes, from a fraction of the canvas and of the scratch."""
    if not isinstance(window, bool):
        raise ValueError('draw_clips: window is True or False, got %r' % (window,))
    if window and not isinstance(bank, clips.PngBank):
        raise ValueError('draw_clips: window=True goes with a clips.PngBank packed with alone=True, got %s' % type(bank).__name__)
    if window and not bank.alone:
        raise ValueError('draw_clips: the bank was not packed with alone=True (clips.png_bank(files, alone=True)): only bands that '
                         'stand alone are decoded by a box')
    plan = _drawn_plan('draw_clips', plan)
    S = _side('draw_clips', S)
    if plan.max_side > clips.MAX_BOX_SCALE * S:
        raise ValueError('draw_clips: the largest base box of the plan has a side of %d; boxes of at most %d (8 x the output side '
                         '%d) are resized' % (plan.max_side, clips.MAX_BOX_SCALE * S, S))
    B, T = plan.B, plan.T
    out = _u8_out('draw_clips', plan.block, (B, T, S, S, 3), out)
    if window:
        frames, boxes, _, status, _, draw = png_decode_bank_window_drawn_u8(bank, plan)
    else:
        frames, _, status, draw = (png_decode_bank_drawn_u8 if isinstance(bank, clips.PngBank) else jpeg_decode_drawn_u8)(bank, plan)
        boxes = draw.boxes
    stages = ['crop'] + ['jpeg'] * (plan.thr_jpeg > 0) + ['perturb'] * (plan.thr_perturb > 0)
    flat = lambda stage: out.view(B * T, S, S, 3) if stages[-1] == stage else None      # the last stage writes `out`
    u8 = crop_resize_u8(frames, boxes, S, out=flat('crop'), checked=True)
    if 'jpeg' in stages:
        u8 = jpeg_roundtrip_u8(u8, draw.quality, out=flat('jpeg'), checked=True)
    if 'perturb' in stages:
        u8 = perturb_u8(u8.view(B, T, S, S, 3), draw.perturb, plan.taps_dev, plan.seed, out=out, checked=True)
    return u8.view(B, T, S, S, 3), draw.view, draw.label, status


_JPEG_STD_HTABS: dict = {}        # (device, tables) -> the Annex K.3 Huffman tables in decode form on the device


def jpeg_bank_ingest(jf, H=None, W=None, layout=None, restart_interval=None, seg_bytes_max=None) -> 'clips.JpegBank':
    """clips.JpegBank.from_encoded: the encoder's result -> a bank over the same bytes, where they lie.  What the host knows
    without waiting -- the number of files, the geometry they share, the header's length, seg_max = ceil(MCUs / restart
    interval), the Annex K.3 Huffman tables -- it fills in; istvt_jpeg_bank_ingest reads the rest on the device: every
    file's two quantisation tables and where its restart intervals lie.  A file the encoder did not finish (a status that is
    not 0) becomes an empty place.  Two launches; no files(), no readback, no synchronisation.  seg_bytes_max: the caller's
    bound on a restart interval's bytes, kept as bank.seg_bytes_max (the lengths are not read here)."""
    if not isinstance(jf, clips.JpegFiles):
        raise TypeError('JpegBank.from_encoded expects a clips.JpegFiles, got %s' % type(jf).__name__)
    if seg_bytes_max is not None and (isinstance(seg_bytes_max, bool) or not isinstance(seg_bytes_max, int) or seg_bytes_max < 1):
        raise ValueError('JpegBank.from_encoded: seg_bytes_max is None or a positive int (bytes of the longest restart interval), '
                         'got %r' % (seg_bytes_max,))
    g = jf.geometry
    if g is not None and g.optimize:
        raise ValueError('JpegBank.from_encoded: files with optimised Huffman tables (optimize=True) carry their own tables behind a '
                         'header of their own length, which the device ingest does not read: encode with optimize=False, or '
                         'hand files() to clips.jpeg_bank')
    if g is None and (H is None or W is None or layout is None or restart_interval is None):
        raise ValueError('JpegBank.from_encoded: a JpegFiles that no encoder call made needs H, W, layout and restart_interval')
    H, W = int(g.H if H is None else H), int(g.W if W is None else W)
    layout = g.layout if layout is None else layout
    if layout not in clips.JPEG_LAYOUTS:
        raise ValueError("JpegBank.from_encoded: layout must be one of '420', '444', '422', 'grey', got %r" % (layout,))
    if not (1 <= H <= clips.JPEG_MAX_SIDE and 1 <= W <= clips.JPEG_MAX_SIDE):
        raise ValueError('JpegBank.from_encoded: frames of 1 x 1 to 16384 x 16384, got %d x %d' % (H, W))
    ri = clips.jpeg_restart_interval(g.restart_interval if restart_interval is None else restart_interval, W, layout=layout)
    if not jf.data.is_cuda or jf.offsets.device != jf.data.device or jf.status.device != jf.data.device \
            or not (jf.data.is_contiguous() and jf.offsets.is_contiguous() and jf.status.is_contiguous()):
        raise RuntimeError('JpegBank.from_encoded: data, offsets and status of the JpegFiles are contiguous on one ROCm device')
    device, n = jf.data.device, len(jf)
    capacity = clips._bank_bytes(int(jf.data.numel()), 'JpegBank.from_encoded')
    hlen = len(clips.jpeg_header(H, W, 50, restart_interval=ri, layout=layout))
    fac = clips.JPEG_LAYOUT_FACTORS[layout]
    (mh, mv), grey = fac[0], len(fac) == 1
    mcus = (-(-H // (8 * mv))) * (-(-W // (8 * mh)))
    seg_max = -(-mcus // min(ri, mcus)) if ri else 1
    nb = mcus * (mh * mv + len(fac) - 1)
    key = (str(device), grey)
    if key not in _JPEG_STD_HTABS:
        order = ((0, 0), (1, 0)) if grey else ((0, 0), (1, 0), (0, 1), (1, 1))
        tabs = [clips.jpeg_huffman_table(*clips.JPEG_STD_HUFFMAN[k]) for k in order]
        _JPEG_STD_HTABS[key] = torch.tensor(tabs, dtype=torch.int32).to(device)
    tables = torch.empty((n * (5 * seg_max + 128 + clips.JPEG_IMAGE_INTS),), dtype=torch.int32, device=device)
    args = _lib.JpegEncodeArgs(
        frames=None, total=0, quality=None, header=None, header_bytes=hlen, scratch=tables.data_ptr(),
        scratch_bytes=4 * tables.numel(), data=jf.data.data_ptr(), capacity=capacity, offsets=jf.offsets.data_ptr(),
        status=jf.status.data_ptr(), stream=_stream(), n=n, H=H, W=W, subsampling=2 if layout == '420' else 0,
        restart_interval=ri, dqt0=clips.JPEG_HEADER_DQT[0], dqt1=clips.JPEG_HEADER_DQT[1])
    with prof('jpeg_bank_ingest', capacity + 4 * tables.numel()):
        _lib.check(_lib.lib().istvt_jpeg_bank_ingest(ctypes.byref(args), clips.JPEG_LAYOUT_CODES[layout]), 'istvt_jpeg_bank_ingest')
    at = 5 * n * seg_max
    bank = clips.JpegBank(data=None, images=None, segments=None, qtabs=None, htabs=None, nbytes=capacity, sizes=[(H, W)] * n, n=n,
                          nseg=n * seg_max, nq=2 * n, nh=2 if grey else 4, blocks=n * nb,
                          groups=n * -(-nb // clips.JPEG_IDCT_BLOCKS), seg_max=seg_max,
                          block_stride=-(-nb // clips.JPEG_IDCT_BLOCKS) * clips.JPEG_IDCT_BLOCKS, Hmax=H, Wmax=W, device=device,
                          seg_bytes_max=seg_bytes_max)
    bank._on[str(device)] = SimpleNamespace(data=jf.data, images=tables[at + 128 * n:].view(n, clips.JPEG_IMAGE_INTS),
                                            segments=tables[:at].view(n * seg_max, 5),
                                            qtabs=tables[at:at + 128 * n].view(2 * n, 64), htabs=_JPEG_STD_HTABS[key])
    return bank


def decode_frames(files, S: int, boxes: Optional[Tensor] = None, split=None, layouts=clips.JPEG_LAYOUTS_DEFAULT,
                  index=None, window: bool = False) -> Tensor:
    """Face crops from JPEG files: files (a sequence of bytes, a clips.JpegBatch or a clips.JpegFiles) are decoded on the device
    (jpeg_decode_u8) and every frame is cut and resized to S x S through `boxes` (int32 [n, 4], crop_resize_u8), or as a
    whole (clips.whole_boxes) where none are given -> uint8 [n, S, S, 3], ready for model(u8.view(B, T, S, S, 3), view=...)
    and the scorers.  split: jpeg_decode_u8's, for files without restart markers.  layouts: jpeg_decode_u8's, for files that are
    not all 4:2:0 or 4:4:4.  files may be a clips.JpegBank with `index` (jpeg_decode_indexed_u8): the places the index names
    are decoded and cut; without `boxes` each is cut whole through boxes made from the decoder's sizes on the device, and a
    place with status 4 or 5 comes out black.  A bank brings its own split (bank.split); split= is refused for it.  A
    clips.PngBatch (clips.png_batch) is decoded by png_decode_u8 and cut the same way, by its bands where it carries them;
    split= and layouts= are refused for it.  A clips.PngBank (clips.png_bank) with `index` goes through png_decode_bank_u8 as a
    JpegBank goes through its decoder: whole-image boxes from the decoder's sizes, a place with status 8 or 9 black; split= and
    layouts= are refused for it too.  window=True (a clips.PngBatch or clips.PngBank packed with alone=True, and `boxes`): only
    the bands each box touches are decoded (png_decode_window_u8) and the crop reads the windows through the moved boxes -- the
    same bytes; host boxes are checked as crop_resize_u8 checks them, boxes on the device are the caller's, with h and w of at
    most 8 S, and for a bank with boxes or an index on the device the window fits any such box."""
    if not isinstance(window, bool):
        raise ValueError('decode_frames: window is True or False, got %r' % (window,))
    if window:
        if not isinstance(files, (clips.PngBatch, clips.PngBank)):
            raise ValueError('decode_frames: window=True goes with a clips.PngBatch or a clips.PngBank packed with alone=True; JPEG '
                             'files are decoded whole')
        if boxes is None:
            raise ValueError('decode_frames: window=True decodes through boxes=, one per frame')
        if split is not None or layouts is not clips.JPEG_LAYOUTS_DEFAULT:
            raise ValueError('decode_frames: split= and layouts= go with JPEG files; a clips.%s takes neither' % type(files).__name__)
        S = _side('crop_resize_u8', S)
        rows = None
        if not torch.is_tensor(boxes):                            # a list is a host table like any other
            boxes = torch.tensor(boxes, dtype=torch.int32).reshape(-1, 4)
        if not boxes.is_cuda:
            clips.check_boxes(boxes, int(boxes.shape[0]) if boxes.dim() else 0, clips.PNG_MAX_SIDE, clips.PNG_MAX_SIDE, S)
        if isinstance(files, clips.PngBank) and files.alone and (boxes.is_cuda or (torch.is_tensor(index) and index.is_cuda)):
            rows = clips.png_window_rows(files, clips.MAX_BOX_SCALE * S)
        windows, moved, _, _, _ = png_decode_window_u8(files, boxes, index=index, rows=rows)
        return crop_resize_u8(windows, moved, S, checked=True)
    if isinstance(files, (clips.JpegBank, clips.PngBank)):
        if index is None:
            raise ValueError('decode_frames: a clips.%s is decoded through index=' % type(files).__name__)
        if isinstance(files, clips.JpegBank):
            frames, sizes, _ = jpeg_decode_indexed_u8(files, index, split=split)
        elif split is not None or layouts is not clips.JPEG_LAYOUTS_DEFAULT:
            raise ValueError('decode_frames: split= and layouts= go with JPEG files; a clips.PngBank takes neither')
        else:
            frames, sizes, _ = png_decode_bank_u8(files, index)
        if boxes is not None:
            return crop_resize_u8(frames, boxes, S)
        S = _side('crop_resize_u8', S)
        clips.check_boxes(clips.whole_boxes([(files.Hmax, files.Wmax)]), 1, files.Hmax, files.Wmax, S)   # the largest there is
        whole = torch.cat([torch.zeros_like(sizes), sizes.clamp(min=1)], dim=1)        # (0, 0, H, W); (0, 0, 1, 1) of a black place
        return crop_resize_u8(frames, whole, S, checked=True)
    if index is not None:
        raise ValueError('decode_frames: index= goes with a clips.JpegBank')
    if isinstance(files, clips.PngBatch):                         # PNG files come packed: a sequence of bytes stays JPEG
        if split is not None or layouts is not clips.JPEG_LAYOUTS_DEFAULT:
            raise ValueError('decode_frames: split= and layouts= go with JPEG files; a clips.PngBatch takes neither')
        frames, _, _ = png_decode_u8(files, checked=True)
        return crop_resize_u8(frames, clips.whole_boxes(files.sizes) if boxes is None else boxes, S)
    batch = files if isinstance(files, clips.JpegBatch) else clips.jpeg_batch(files, layouts)
    frames, _, _ = jpeg_decode_u8(batch, checked=True, split=split)
    return crop_resize_u8(frames, clips.whole_boxes(batch.sizes) if boxes is None else boxes, S)


# ---- JPEG files out ----------------------------------------------------------------------------------------------------------
_JPEG_HEADERS: dict = {}          # (H, W, subsampling, restart interval, device, layout) -> (header on the device, its length)


def _jpeg_header_on(device, H: int, W: int, subsampling: str, ri: int, layout=None):
    """the header every file of a call starts with, uploaded once per geometry and device; its table bytes are placeholders"""
    key = (H, W, subsampling, ri, str(device), layout)
    if key not in _JPEG_HEADERS:
        head = clips.jpeg_header(H, W, 50, subsampling, ri, layout)
        _JPEG_HEADERS[key] = (torch.frombuffer(bytearray(head), dtype=torch.uint8).to(device), len(head))
    return _JPEG_HEADERS[key]


def jpeg_encode_u8(frames: Tensor, quality, subsampling: str = '420', restart_interval='row', capacity: Optional[int] = None,
                   out: Optional[Tensor] = None, checked: bool = False, optimize: bool = False, layout=None) -> 'clips.JpegFiles':
    """JPEG files out (clips.py): frames uint8 [n,H,W,3] or [B,T,H,W,3], contiguous, on the device, quality int32 [n] per
    frame or, for clips, [B] shared by the T frames of a clip (or an int for all), every entry in 1..100 -> a clips.JpegFiles
    on the device: the baseline JFIF files of clips.jpeg_encode_files_host end to end in `data`, byte for byte, with `offsets`
    and a `status` per file.  subsampling '420' or '444'; restart_interval in MCUs (0: none, and one lane per image, slow)
    or 'row': a restart marker every MCU row, the files ops.jpeg_decode_u8 decodes one lane per row.  A host quality table is
    validated before any launch and uploaded without blocking; checked=True takes a per-frame device table as it is, and an
    entry <= 0 then gives an empty file with status 2.  capacity: the bytes of `data`, by default n * (H * W * 3 + header); a
    file that does not fit (noise at quality 100; a frame of a few pixels, whose file still codes a whole MCU) gets status 1,
    nothing of it is written, and offsets[n] still says what a retry needs.  `out` (uint8, one dimension, contiguous, no
    overlap with the frames) is used as `data`.  Nothing synchronises.
    optimize=True (PIL's word for it): every file is coded with its own four Huffman tables, the bytes of
    clips.jpeg_encode_files_host(optimize=True): fewer scan bytes for every later decode, for one more launch now.  Its header
    is at most the standard one's (clips.jpeg_header_bound), so the default capacity is the same.  The scratch of that entry
    is 128 bytes per block + 16 per restart interval + 3344 per frame.
    layout: one of clips.JPEG_LAYOUTS in the place of subsampling, which then keeps its default: the bytes of
    clips.jpeg_encode_files_host(layout=).  '420' and '444' are the subsampling of that name, by the same entry.  '422' (MCUs
    of 16 x 8 pixels, 4 blocks) and 'grey' (8 x 8, one block: Y of the colour transform, the frames stay RGB) go through
    istvt_jpeg_encode_layout_u8, standard or optimised; restart_interval counts those MCUs."""
    if not isinstance(optimize, bool):
        raise ValueError('jpeg_encode_u8: optimize is True or False, got %r' % (optimize,))
    n, T, H, W = _rgb_source('jpeg_encode_u8', frames, contiguous=True, on_device=False)
    word = clips._jpeg_encode_layout(subsampling, layout, 'jpeg_encode_u8')
    if word in clips.JPEG_SUBSAMPLINGS:    # the subsampling of that name: the same header, entry and profile record
        subsampling, layout = word, None
    mh, mv = clips.JPEG_LAYOUT_FACTORS[word][0]
    ri = clips.jpeg_restart_interval(restart_interval, W, subsampling, layout)
    host_only = ('jpeg_encode_u8: a device quality table is taken with checked=True only (int32, one entry per frame, validated '
                 'by the caller); hand over the host table otherwise')
    if not checked:                        # the argument errors that need no device, before the one that asks for it
        if torch.is_tensor(quality) and quality.device.type != 'cpu':
            raise RuntimeError(host_only)
        clips.check_encode_qualities(quality, n if T is None else n // T)
    _req(frames, 'frames')
    qdev = _frame_table('jpeg_encode_u8', _QUALITIES, quality, n, T, frames.device, checked, clips.check_encode_qualities, host_only)
    header, hlen = _jpeg_header_on(frames.device, H, W, subsampling, ri, layout)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or out.device != frames.device \
                or not out.is_contiguous() or out.numel() == 0:
            raise RuntimeError('jpeg_encode_u8: out must be contiguous uint8 (capacity,) on %s' % frames.device)
        if capacity is not None and int(capacity) != out.numel():
            raise ValueError('jpeg_encode_u8: capacity %d and out of %d bytes disagree' % (int(capacity), out.numel()))
        data = out
    else:
        # (hlen is clips.jpeg_header_bound(H, W, subsampling, ri): no optimised header is longer than the standard one)
        capacity = n * (H * W * 3 + hlen) if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError('jpeg_encode_u8: the capacity must be positive, got %d' % capacity)
        data = torch.empty((capacity,), dtype=torch.uint8, device=frames.device)
    nbytes = frames.numel()
    _no_overlap('jpeg_encode_u8', data, frames.data_ptr(), nbytes, 'frames')
    mcus = (-(-H // (8 * mv))) * (-(-W // (8 * mh)))
    blocks = n * mcus * (mh * mv + len(clips.JPEG_LAYOUT_FACTORS[word]) - 1)
    segments = n * (-(-mcus // min(ri, mcus)) if ri else 1)
    scratch = torch.empty((jpeg_encode_scratch_bytes(blocks, segments, n, optimize),), dtype=torch.uint8, device=frames.device)
    offsets = torch.empty((n + 1,), dtype=torch.int64, device=frames.device)
    status = torch.empty((n,), dtype=torch.int32, device=frames.device)
    _jpeg_encode_launch(frames, nbytes, qdev, header, hlen, scratch, data, offsets, status, n, H, W, mh, ri, optimize, layout)
    files = clips.JpegFiles(data, offsets, status)
    # what all files of the call share, for clips.JpegBank.from_encoded: known here, and nowhere else without a parse
    files.geometry = SimpleNamespace(H=H, W=W, layout=word, restart_interval=ri, optimize=optimize)
    return files


JPEG_OPT_ROW_BYTES = 3344                   # ISTVT_JPEG_OPT_ROW_BYTES of include/istvt_hip.h: an image's tables in the scratch


def jpeg_encode_scratch_bytes(blocks: int, segments: int, n: int, optimize: bool = False) -> int:
    """the scratch of istvt_jpeg_encode_u8: 128 bytes per 8 x 8 block of the batch + 16 per restart interval; of
    istvt_jpeg_encode_opt_u8 (optimize=True): + JPEG_OPT_ROW_BYTES per frame"""
    return 128 * blocks + 16 * segments + (JPEG_OPT_ROW_BYTES * n if optimize else 0)


def _jpeg_encode_launch(frames, nbytes, qdev, header, hlen, scratch, data, offsets, status, n, H, W, sub, ri, optimize=False,
                        layout=None) -> None:
    """the entry on buffers that are all the caller's (tests put sentinels around them); layout: None, '422' or 'grey'"""
    args = _lib.JpegEncodeArgs(
        frames=frames.data_ptr(), total=nbytes, quality=qdev.data_ptr(), header=header.data_ptr(), header_bytes=hlen,
        scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), data=data.data_ptr(), capacity=data.numel(),
        offsets=offsets.data_ptr(), status=status.data_ptr(), stream=_stream(), n=n, H=H, W=W,
        subsampling=2 if sub == 2 and layout is None else 0,
        restart_interval=ri, dqt0=clips.JPEG_HEADER_DQT[0], dqt1=clips.JPEG_HEADER_DQT[1])
    if layout is not None:
        dht = clips.jpeg_header_dht(layout) if optimize else (0, 0)
        with prof('jpeg_encode_layout_u8', nbytes + (4 if optimize else 3) * scratch.numel()):
            _lib.check(_lib.lib().istvt_jpeg_encode_layout_u8(ctypes.byref(args), clips.JPEG_LAYOUT_CODES[layout], *dht),
                       'istvt_jpeg_encode_layout_u8')
        return
    if optimize:
        with prof('jpeg_encode_opt_u8', nbytes + 4 * scratch.numel()):
            _lib.check(_lib.lib().istvt_jpeg_encode_opt_u8(ctypes.byref(args), *clips.JPEG_HEADER_DHT), 'istvt_jpeg_encode_opt_u8')
        return
    with prof('jpeg_encode_u8', nbytes + 3 * scratch.numel()):   # + the files' bytes, which live on the device
        _lib.check(_lib.lib().istvt_jpeg_encode_u8(ctypes.byref(args)), 'istvt_jpeg_encode_u8')


class _NotGiven:
    """the default of encode_frames' JPEG-only arguments: tells `not given` from a value that happens to be the default"""

    def __init__(self, value):
        self.value = value

    def __repr__(self):
        return repr(self.value)


_JPEG_ONLY = dict(quality=_NotGiven(90), subsampling=_NotGiven('420'), restart_interval=_NotGiven('row'), optimize=_NotGiven(False),
                  layout=None)       # layout's own word for `not given` is None, as in every other signature that has it


def encode_frames(frames: Tensor, S: int, boxes: Optional[Tensor] = None, transforms: Optional[Tensor] = None,
                  quality=_JPEG_ONLY['quality'], subsampling=_JPEG_ONLY['subsampling'],
                  restart_interval=_JPEG_ONLY['restart_interval'], optimize=_JPEG_ONLY['optimize'], layout=_JPEG_ONLY['layout'],
                  format: str = 'jpeg', band_rows=None, filters=None, index=None, alone=None):
    """Dataset preparation, the mirror of decode_frames: whole frames uint8 [n,Hs,Ws,3] or [B,T,Hs,Ws,3] on the device are
    cut to S x S through `boxes` (crop_resize_u8) or `transforms` (warp_similarity_u8) and the crops leave as JPEG files
    (jpeg_encode_u8; optimize=True: with their own Huffman tables; layout: one of clips.JPEG_LAYOUTS in the place of
    subsampling) -> a clips.JpegFiles, whose files() ops.decode_frames and clips.jpeg_batch take (with layouts='all' for '422'
    and 'grey').  format='png': the crops leave lossless, as PNG files (png_encode_u8 with band_rows and filters, 16 and
    'adaptive' where not given) -> a clips.PngFiles; the JPEG-only arguments (quality 90, subsampling '420', restart_interval
    'row' and optimize False where not given) are then refused if given, whatever their value, and so is a layout.
    index=True (format='png' only): the files carry their band index (png_encode_u8(index=True)); alone=True with it: the
    bands stand alone (png_encode_u8(alone=True))."""
    if format not in ('jpeg', 'png'):
        raise ValueError("encode_frames: format is 'jpeg' or 'png', got %r" % (format,))
    if index is not None and format != 'png':
        raise ValueError("encode_frames: index= goes with format='png' (the band index of a PNG file); JPEG files have none")
    if alone is not None and format != 'png':
        raise ValueError("encode_frames: alone= goes with format='png' (bands of a PNG file that stand alone); JPEG files have none")
    if format == 'png':
        given = dict(quality=quality, subsampling=subsampling, restart_interval=restart_interval, optimize=optimize, layout=layout)
        for name, default in _JPEG_ONLY.items():
            if given[name] is not default:
                raise ValueError("encode_frames: %s= goes with format='jpeg'; format='png' takes band_rows= and filters=" % name)
    elif band_rows is not None or filters is not None:
        raise ValueError("encode_frames: band_rows= and filters= go with format='png'")
    quality, subsampling, restart_interval, optimize, layout = (v.value if isinstance(v, _NotGiven) else v for v in
                                                                (quality, subsampling, restart_interval, optimize, layout))
    if (boxes is None) == (transforms is None):
        raise ValueError('encode_frames: boxes and transforms are two ways to cut the same crop: pass one of them')
    if format == 'png':
        band_rows = clips.check_png_band_rows(16 if band_rows is None else band_rows, 'png_encode_u8')
        filters = 'adaptive' if filters is None else filters
        clips.check_png_filters(filters, 'png_encode_u8')
        if index is not None and not isinstance(index, bool):
            raise ValueError('png_encode_u8: index is True or False, got %r' % (index,))
        index, alone = False if index is None else index, False if alone is None else alone
        clips._check_png_alone(alone, index, 'png_encode_u8')
        crops = crop_resize_u8(frames, boxes, S) if boxes is not None else warp_similarity_u8(frames, transforms, S)
        return png_encode_u8(crops, band_rows, filters, index=index, alone=alone)
    if not isinstance(optimize, bool):
        raise ValueError('jpeg_encode_u8: optimize is True or False, got %r' % (optimize,))
    clips._jpeg_encode_layout(subsampling, layout, 'jpeg_encode_u8')
    crops = crop_resize_u8(frames, boxes, S) if boxes is not None else warp_similarity_u8(frames, transforms, S)
    return jpeg_encode_u8(crops, quality, subsampling, restart_interval, optimize=optimize, layout=layout)


# ---- PNG files out -----------------------------------------------------------------------------------------------------------
PNG_BAND_ROW_BYTES = 1728                   # ISTVT_PNG_BAND_ROW_BYTES of include/istvt_hip.h: a band's tables in the scratch


def png_encode_scratch(n: int, H: int, W: int, bpp: int, band_rows: int):
    """-> (raw_stride, scratch bytes) of istvt_png_encode_u8: a file's filtered rows, rounded up to 16 bytes, and
    PNG_BAND_ROW_BYTES per band"""
    R = min(band_rows, H)
    raw_stride = -(-(H * (1 + W * bpp)) // 16) * 16
    return raw_stride, n * raw_stride + n * (-(-H // R)) * PNG_BAND_ROW_BYTES


def png_encode_u8(frames: Tensor, band_rows: int = 16, filters='adaptive', capacity: Optional[int] = None,
                  buffers=None, index: bool = False, alone: bool = False) -> 'clips.PngFiles':
    """PNG files out (clips.py): frames uint8 [n,H,W] or [n,H,W,1] (grey), [n,H,W,3] (RGB), [n,H,W,4] (RGBA) or clips
    [B,T,H,W,C], contiguous, on the device -> a clips.PngFiles on the device: the files of clips.png_encode_files_host end to
    end in `data`, byte for byte, with `offsets` and a `status` per file.  Lossless, for frame sets whose compression traces a
    JPEG re-encode would overwrite.  band_rows: the rows that are coded together; every band is a DEFLATE block of its own
    that starts and ends on a byte and refers to nothing outside itself.  filters: 'adaptive' (per row the type with the
    smallest sum of absolute residuals) or one type 0..4 for every row.  capacity: the bytes of `data`, by default n *
    clips.png_encoded_bound(H, W, bpp, band_rows); a file that does not fit gets status 1, nothing of it is written, and
    offsets[n] says what a retry needs.  buffers = (data uint8 (capacity,), scratch uint8 of at least png_encode_scratch(...)[1]
    bytes and 16-byte aligned, offsets int64 (n + 1,), status int32 (n,)): the caller's, to encode step after step without an
    allocation; data may not overlap the frames.  Four launches, nothing synchronises.
    index=True: every file carries its bands' offsets in a baND chunk between IHDR and IDAT, the bytes of
    clips.png_encode_files_host(index=True), which ops.png_decode_u8(files, bands='index') decodes one wave per band; the
    default capacity grows by the chunks (clips.png_encoded_bound(index=True)).
    alone=True (needs index=True): every band's first row is filtered without the row above and the index says so, the bytes
    of clips.png_encode_files_host(index=True, alone=True) (istvt_png_encode_alone_u8); a batch or bank packed with alone=True
    then unfilters such files one wave per band."""
    what = 'png_encode_u8'
    if not isinstance(index, bool):
        raise ValueError('%s: index is True or False, got %r' % (what, index))
    clips._check_png_alone(alone, index, what)
    if torch.is_tensor(frames) and frames.dim() == 3:
        frames = frames.unsqueeze(-1)
    n, T, H, W = _rgb_source(what, frames, contiguous=True, on_device=False, channels=(1, 3, 4))
    bpp = int(frames.shape[-1])
    R = clips.check_png_band_rows(band_rows, what)
    mode = clips.check_png_filters(filters, what)
    bound = n * clips.png_encoded_bound(H, W, bpp, R, index)
    if bound > clips.PNG_MAX_BYTES:
        raise ValueError('%s: the files of a batch hold at most %d bytes, %d frames of %d x %d x %d can need %d'
                         % (what, clips.PNG_MAX_BYTES, n, H, W, bpp, bound))
    _req(frames, 'frames')
    device = frames.device
    raw_stride, need = png_encode_scratch(n, H, W, bpp, R)
    if buffers is None:
        capacity = bound if capacity is None else int(capacity)
        if capacity < 1:
            raise ValueError('%s: the capacity must be positive, got %d' % (what, capacity))
        data = torch.empty((capacity,), dtype=torch.uint8, device=device)
        scratch = torch.empty((need,), dtype=torch.uint8, device=device)
        offsets = torch.empty((n + 1,), dtype=torch.int64, device=device)
        status = torch.empty((n,), dtype=torch.int32, device=device)
    else:
        data, scratch, offsets, status = buffers
        ok = (torch.is_tensor(t) and t.device == device and t.is_contiguous() for t in buffers)
        if (not all(ok) or data.dtype != torch.uint8 or data.dim() != 1 or data.numel() < 1 or scratch.dtype != torch.uint8
                or scratch.numel() < need or scratch.data_ptr() % 16 or offsets.dtype != torch.int64
                or tuple(offsets.shape) != (n + 1,) or status.dtype != torch.int32 or tuple(status.shape) != (n,)):
            raise RuntimeError('%s: buffers = (uint8 data (capacity,); uint8 scratch of %d bytes, 16-byte aligned; int64 offsets '
                               '(%d,); int32 status (%d,)), contiguous on %s' % (what, need, n + 1, n, device))
        if capacity is not None and int(capacity) != data.numel():
            raise ValueError('%s: capacity %d and data of %d bytes disagree' % (what, int(capacity), data.numel()))
    nbytes = frames.numel()
    _no_overlap(what, data, frames.data_ptr(), nbytes, 'frames')
    args = _lib.JpegEncodeArgs(
        frames=frames.data_ptr(), total=nbytes, scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), data=data.data_ptr(),
        capacity=data.numel(), offsets=offsets.data_ptr(), status=status.data_ptr(), stream=_stream(), n=n, H=H, W=W)
    name = 'png_encode_alone_u8' if alone else 'png_encode_indexed_u8' if index else what
    with prof(name, nbytes + 3 * n * H * (1 + W * bpp)):          # the pixels; the filtered rows written once and read twice
        _lib.check(getattr(_lib.lib(), 'istvt_' + name)(ctypes.byref(args), bpp, R, mode, raw_stride), 'istvt_' + name)
    files = clips.PngFiles(data, offsets, status)
    files.geometry = SimpleNamespace(H=H, W=W, bpp=bpp, band_rows=R, filters=filters, index=index, alone=alone)
    return files


def perturb_u8(frames: Tensor, table: Tensor, taps: Optional[Tensor] = None, seed: int = 0, out: Optional[Tensor] = None,
               checked: bool = False) -> Tensor:
    """Perturbations (clips.py): frames uint8 [n,H,W,3] or [B,T,H,W,3] on the device, table int32 [n,4] = (kind, param,
    frame_id, stream) per frame or, for clips, [B,4] per clip (frame t of a clip takes its clip's kind, param and stream and
    frame_id + t), taps int32 [K,21] (clips.gaussian_taps; needed where a row blurs), seed the 64-bit key of the noise -> uint8
    of the same shape: brightness, contrast, saturation, Gaussian noise, Gaussian blur or pixelation per frame, the bits of
    clips.perturb_host.  A host table (and host taps) is validated (clips.check_perturbations) before any launch and uploaded
    without blocking; checked=True takes a device table, and device taps, that the caller has validated already and reads
    nothing back.  A device table without checked=True is refused: validating it would copy it back and wait for the device.
    `out` (uint8, contiguous, of the input's shape) is written when given; it may not share memory with the input, whose
    neighbours blur and pixelation read."""
    n, T, H, W = _rgb_source('perturb_u8', frames, contiguous=True)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError('perturb_u8: the seed must lie in [0, 2^64), got %d' % seed)
    dev = frames.device
    host_only = ('perturb_u8: a device table or device taps are taken with checked=True only (validated by the caller); hand '
                 'over the host tensors otherwise')
    if checked:
        if taps is not None and (not torch.is_tensor(taps) or taps.dtype != torch.int32 or taps.dim() != 2
                                 or taps.shape[1] != clips.PERTURB_TAPS
                                 or not 1 <= taps.shape[0] <= clips.PERTURB_MAX_TAPS_ROWS or taps.device != dev):
            raise RuntimeError('perturb_u8: checked taps are int32 (K, 21), K <= %d, on %s' % (clips.PERTURB_MAX_TAPS_ROWS, dev))
    elif torch.is_tensor(taps) and taps.is_cuda:
        raise RuntimeError(host_only)
    # the table keeps one row per clip: the kernel spreads it, frame t of a clip takes frame_id + t
    tdev = _frame_table('perturb_u8', _PERTURBATIONS, table, frames.shape[0], None, dev, checked,
                        lambda t, rows: clips.check_perturbations(t, rows, taps), host_only)
    pdev = None if taps is None else _c(taps) if checked else taps.detach().contiguous().to(dev, non_blocking=True)
    out = _u8_out('perturb_u8', frames, frames.shape, out)
    nbytes = frames.numel()
    _no_overlap('perturb_u8', out, frames.data_ptr(), nbytes, 'input (blur and pixelation read their neighbours)')
    strips = min(32, -(-(H * W) // 2048))                         # partial sums of Y per frame, for the contrast mean
    scratch = torch.empty((n * strips,), dtype=torch.int64, device=dev)
    with prof('perturb_u8', 2 * nbytes):
        _lib.check(_lib.lib().istvt_perturb_u8(frames.data_ptr(), nbytes, n, H, W, tdev.data_ptr(), 0 if T is None else T,
                                               0 if pdev is None else pdev.data_ptr(), 0 if pdev is None else pdev.shape[0], seed,
                                               scratch.data_ptr(), scratch.numel() * 8, out.data_ptr(), _stream()),
                   'istvt_perturb_u8')
    return out
