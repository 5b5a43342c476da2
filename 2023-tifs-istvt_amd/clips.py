"""Training clips as the decoder delivers them: uint8, channels last, with crop / flip augmentation as a VIEW.

A training step takes ``model(u8, view=view)``: ``u8`` uint8 (B, T, Hs, Ws, 3) source frames, ``view`` int32 (B, 3) with
one (y0, x0, flip) per clip.  Output pixel (y, x) of a frame is source pixel (y0 + y, x0 + (S-1-x if flip else x)); the
channel order inside a pixel is never reversed.  conv1 reads the bytes through that view and normalises them itself
(istvt_conv1_fwd_u8_view / istvt_conv1_wgrad_u8 / istvt_im2col_conv1_u8), so the crop, the flip and the float32 clip are
never made: 3 bytes per pixel cross the host boundary and are saved for the backward pass instead of 12.

``to_float`` is the definition: the float32 NCHW tensor the host makes of the same bytes.  The byte path gives the bits of
the float path on that tensor (DESIGN.md "Training from bytes").
"""
from typing import Optional

import torch

Tensor = torch.Tensor


def random_views(B: int, Hs: int, Ws: int, S: int, generator: Optional[torch.Generator] = None, flip_p: float = 0.5) -> Tensor:
    """One random (y0, x0, flip) per clip: y0 uniform in [0, Hs-S], x0 in [0, Ws-S], flip with probability flip_p.
    Returns an int32 (B, 3) host tensor (contiguous: ready for pin_memory()); reproducible from `generator`."""
    if B < 1 or S < 3 or S > min(Hs, Ws):
        raise ValueError('random_views: need B >= 1 and 3 <= S <= min(Hs, Ws), got B=%d Hs=%d Ws=%d S=%d' % (B, Hs, Ws, S))
    if not 0.0 <= flip_p <= 1.0:
        raise ValueError('random_views: flip_p must be a probability, got %r' % (flip_p,))
    y0 = torch.randint(0, Hs - S + 1, (B,), generator=generator)
    x0 = torch.randint(0, Ws - S + 1, (B,), generator=generator)
    flip = torch.rand((B,), generator=generator) < flip_p
    return torch.stack([y0, x0, flip.to(torch.int64)], dim=1).to(torch.int32).contiguous()


def check_views(view, n: int, Hs: int, Ws: int, S: Optional[int]) -> Optional[Tensor]:
    """Host validation of a view table before any launch: int32 (n, 3) with 0 <= y0 <= Hs-S, 0 <= x0 <= Ws-S and flip in
    {0, 1}; n is the number of frames (a per-frame table) or of clips (a per-clip one).  None (the identity view of every
    frame) passes when the source is already S x S.  Returns the table on the host (a device tensor is copied back, which
    waits for the device: hand over the loader's host tensor)."""
    if S is None:
        if view is not None:
            raise ValueError('a view needs the crop side S')
        if Hs != Ws:
            raise ValueError('without a view and a crop side the source frames must be square, got %d x %d' % (Hs, Ws))
        S = Hs
    if S < 3 or S > min(Hs, Ws):
        raise ValueError('the crop side must satisfy 3 <= S <= min(Hs, Ws), got S=%d for %d x %d frames' % (S, Hs, Ws))
    if view is None:
        if Hs != S or Ws != S:
            raise ValueError('%d x %d source frames need a view to give %d x %d crops' % (Hs, Ws, S, S))
        return None
    if not torch.is_tensor(view):
        raise TypeError('view must be an int32 tensor (n, 3), got %s' % type(view).__name__)
    if view.dtype != torch.int32:
        raise TypeError('view must be int32, got %s' % view.dtype)
    if view.dim() != 2 or tuple(view.shape) != (n, 3):
        raise ValueError('view must have shape (%d, 3) = (y0, x0, flip) per entry, got %s' % (n, tuple(view.shape)))
    v = view.detach().cpu()
    y0, x0, flip = v[:, 0], v[:, 1], v[:, 2]
    if bool((y0 < 0).any()) or bool((y0 > Hs - S).any()):
        raise ValueError('view: y0 must lie in [0, %d] (Hs=%d, S=%d), got [%d, %d]' % (Hs - S, Hs, S, int(y0.min()), int(y0.max())))
    if bool((x0 < 0).any()) or bool((x0 > Ws - S).any()):
        raise ValueError('view: x0 must lie in [0, %d] (Ws=%d, S=%d), got [%d, %d]' % (Ws - S, Ws, S, int(x0.min()), int(x0.max())))
    if bool(((flip != 0) & (flip != 1)).any()):
        raise ValueError('view: flip must be 0 or 1')
    return v


def to_float(u8: Tensor, mean, std, view: Optional[Tensor] = None, S: Optional[int] = None) -> Tensor:
    """The host restatement of what the byte path computes: uint8 (..., Hs, Ws, 3) -> float32 (..., 3, S, S), cropped and
    flipped by `view` and normalised as torchvision's ToTensor + Normalize do, ((u.float() / 255) - mean) / std.  The
    leading dimensions are (frames,) with a per-frame view (frames, 3), or (B, T) with a per-clip view (B, 3) shared by the
    T frames of a clip.  Runs where u8 lives; the bit-identity statement holds for the host (the device's float division
    differs in the last bit)."""
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError('to_float expects uint8 (frames, Hs, Ws, 3) or (B, T, Hs, Ws, 3), got %s %s' % (u8.dtype, tuple(u8.shape)))
    Hs, Ws = u8.shape[-3], u8.shape[-2]
    v = check_views(view, u8.shape[0], Hs, Ws, S)
    S = Hs if S is None else S
    if v is not None:
        parts = []
        for i in range(u8.shape[0]):
            y0, x0, flip = (int(q) for q in v[i])
            c = u8[i, ..., y0:y0 + S, x0:x0 + S, :]
            parts.append(c.flip(-2) if flip else c)
        u8 = torch.stack(parts)
    m = torch.as_tensor(mean, dtype=torch.float32, device=u8.device).reshape(3)
    s = torch.as_tensor(std, dtype=torch.float32, device=u8.device).reshape(3)
    x = ((u8.float() / 255) - m) / s
    return x.movedim(-1, -3).contiguous()


def per_frame_views(view: Tensor, T: int) -> Tensor:
    """(B, 3) per-clip table -> (B*T, 3) per-frame table (each clip's row repeated for its T frames), where `view` lives"""
    return view.repeat_interleave(T, dim=0).contiguous()
