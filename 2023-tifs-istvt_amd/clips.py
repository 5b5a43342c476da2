"""Training clips as the decoder delivers them: uint8, channels last, with crop / flip augmentation as a VIEW.

A training step takes ``model(u8, view=view)``: ``u8`` uint8 (B, T, Hs, Ws, 3) source frames, ``view`` int32 (B, 3) with
one (y0, x0, flip) per clip.  Output pixel (y, x) of a frame is source pixel (y0 + y, x0 + (S-1-x if flip else x)); the
channel order inside a pixel is never reversed.  conv1 reads the bytes through that view and normalises them itself
(istvt_conv1_fwd_u8_view / istvt_conv1_wgrad_u8 / istvt_im2col_conv1_u8), so the crop, the flip and the float32 clip are
never made: 3 bytes per pixel cross the host boundary and are saved for the backward pass instead of 12.

``to_float`` is the definition: the float32 NCHW tensor the host makes of the same bytes.  The byte path gives the bits of
the float path on that tensor (DESIGN.md "Training from bytes").

Whole frames and face boxes (DESIGN.md "Frames and boxes") are the second half of this file: ``check_boxes``,
``resize_weights``, ``crop_resize_host`` (the definition of ops.crop_resize_u8) and ``random_boxes``.
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


# ------------------------------------------------------------------------------------------ frames and boxes
# DESIGN.md "Frames and boxes": whole decoded frames uint8 (n, Hs, Ws, 3) and one face box (y0, x0, h, w) per frame ->
# uint8 (n, S, S, 3).  The box is cut out and resized as torch.nn.functional.interpolate(mode='bilinear',
# align_corners=False, antialias=True) resizes the cropped image: separable, horizontal pass first and kept in float32,
# byte = clamp(floor(v + 0.5), 0, 255).  ops.crop_resize_u8 is the device kernel, crop_resize_host the definition.
MAX_BOX_SCALE = 8                          # h, w <= 8 S: at most 17 taps per axis


def resize_weights(n_in: int, n_out: int):
    """The tap table of one axis n_in -> n_out, in float64: (lo int64 (n_out,), count int64 (n_out,), w float64
    (n_out, K)), K = the largest count; output i is sum_k w[i, k] * src[lo[i] + k], weights past count[i] are zero.

        scale = n_in / n_out;  sup = max(scale, 1);  c = (i + 0.5) * scale
        lo = max(int(c - sup + 0.5), 0);  hi = min(int(c + sup + 0.5), n_in)
        w_j = max(0, 1 - |(j - c + 0.5) / sup|) for j in [lo, hi), divided by their sum

    An upscale is plain half-pixel bilinear, a downscale widens the triangle (as PIL does), n_in == n_out gives 1 and 0."""
    if n_in < 1 or n_out < 1:
        raise ValueError('resize_weights: sizes must be positive, got %d -> %d' % (n_in, n_out))
    scale = n_in / n_out
    sup = max(scale, 1.0)
    los, rows = [], []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(int(c - sup + 0.5), 0)
        hi = min(int(c + sup + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)]
        total = 0.0
        for v in w:
            total += v
        los.append(lo)
        rows.append([v / total for v in w])
    K = max(len(r) for r in rows)
    table = torch.zeros((n_out, K), dtype=torch.float64)
    for i, r in enumerate(rows):
        table[i, :len(r)] = torch.tensor(r, dtype=torch.float64)
    return torch.tensor(los, dtype=torch.int64), torch.tensor([len(r) for r in rows], dtype=torch.int64), table


def check_boxes(boxes, n: int, Hs: int, Ws: int, S: int) -> Tensor:
    """Host validation of a box table before any launch: int32 (n, 4) = (y0, x0, h, w) with 1 <= h, w <= 8 S and the box
    inside [0, Hs) x [0, Ws).  Returns the table on the host (a device tensor is copied back, which waits for the device:
    hand over the tracker's host tensor)."""
    if S is None or S < 1:
        raise ValueError('boxes need the output side S >= 1, got %r' % (S,))
    if not torch.is_tensor(boxes):
        raise TypeError('boxes must be an int32 tensor (n, 4), got %s' % type(boxes).__name__)
    if boxes.dtype != torch.int32:
        raise TypeError('boxes must be int32, got %s' % boxes.dtype)
    if boxes.dim() != 2 or tuple(boxes.shape) != (n, 4):
        raise ValueError('boxes must have shape (%d, 4) = (y0, x0, h, w) per entry, got %s' % (n, tuple(boxes.shape)))
    b = boxes.detach().cpu()
    y0, x0, h, w = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    lim = MAX_BOX_SCALE * S
    if bool((h < 1).any()) or bool((w < 1).any()) or bool((h > lim).any()) or bool((w > lim).any()):
        raise ValueError('boxes: h and w must lie in [1, %d] (8 x the output side %d), got h in [%d, %d], w in [%d, %d]'
                         % (lim, S, int(h.min()), int(h.max()), int(w.min()), int(w.max())))
    if bool((y0 < 0).any()) or bool((y0 + h > Hs).any()):
        raise IndexError('boxes: rows [y0, y0 + h) must lie inside [0, %d), got y0 >= %d, y0 + h <= %d'
                         % (Hs, int(y0.min()), int((y0 + h).max())))
    if bool((x0 < 0).any()) or bool((x0 + w > Ws).any()):
        raise IndexError('boxes: columns [x0, x0 + w) must lie inside [0, %d), got x0 >= %d, x0 + w <= %d'
                         % (Ws, int(x0.min()), int((x0 + w).max())))
    return b


def per_frame_boxes(boxes: Tensor, T: int) -> Tensor:
    """(B, 4) per-clip table -> (B*T, 4) per-frame table (each clip's box repeated for its T frames), where `boxes` lives"""
    return boxes.repeat_interleave(T, dim=0).contiguous()


def crop_resize_host(u8: Tensor, boxes: Tensor, S: int) -> Tensor:
    """The definition on the host: uint8 (n, Hs, Ws, 3) or (B, T, Hs, Ws, 3) and boxes int32 (n, 4) / (B, 4) -> uint8
    (n, S, S, 3) / (B, T, S, S, 3).  Horizontal pass first, its result kept in float32, then the vertical pass in float32;
    byte = clamp(floor(v + 0.5), 0, 255).  Documentation and a fallback for tests: the device path is ops.crop_resize_u8
    (whose float32 sums run in another order: a byte may differ by one where the value lies next to a half)."""
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError('crop_resize_host expects uint8 (n, Hs, Ws, 3) or (B, T, Hs, Ws, 3), got %s %s' % (u8.dtype, tuple(u8.shape)))
    lead = tuple(u8.shape[:-3])
    Hs, Ws = u8.shape[-3], u8.shape[-2]
    b = check_boxes(boxes, u8.shape[0], Hs, Ws, S)
    if u8.dim() == 5:
        b = per_frame_boxes(b, u8.shape[1])
    src = u8.reshape((-1, Hs, Ws, 3)).cpu()
    out = torch.empty((src.shape[0], S, S, 3), dtype=torch.uint8)
    tables = {}
    for i in range(src.shape[0]):
        y0, x0, h, w = (int(q) for q in b[i])
        for n_in in (h, w):
            if n_in not in tables:
                lo, cnt, tab = resize_weights(n_in, S)
                idx = (lo[:, None] + torch.arange(tab.shape[1])[None, :]).clamp_(max=n_in - 1)   # past count: weight 0
                tables[n_in] = (idx, tab.to(torch.float32))
        crop = src[i, y0:y0 + h, x0:x0 + w, :].to(torch.float32)
        xi, xw = tables[w]
        hor = (crop[:, xi, :] * xw[None, :, :, None]).sum(2)                   # (h, S, 3) float32
        yi, yw = tables[h]
        ver = (hor[yi] * yw[:, :, None, None]).sum(1)                          # (S, S, 3)
        out[i] = torch.floor(ver + 0.5).clamp_(0, 255).to(torch.uint8)
    return out.reshape(lead + (S, S, 3)).to(u8.device)


def random_boxes(B: int, Hs: int, Ws: int, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3),
                 generator: Optional[torch.Generator] = None) -> Tensor:
    """One random (y0, x0, h, w) per clip for scale augmentation: the box area is `scale` (uniform) of the largest square of
    the frame, min(Hs, Ws) ** 2, its aspect w / h is log-uniform in `ratio`, a side is cut to the frame where it sticks out,
    and the position is uniform over what is left.  Returns an int32 (B, 4) host tensor, reproducible from `generator`.
    A training step is then ``model(ops.crop_resize_u8(u8, boxes.to(dev), S), view=flips)``."""
    if B < 1 or Hs < 1 or Ws < 1:
        raise ValueError('random_boxes: need B, Hs, Ws >= 1, got B=%d Hs=%d Ws=%d' % (B, Hs, Ws))
    if not (0.0 < scale[0] <= scale[1] <= 1.0) or not (0.0 < ratio[0] <= ratio[1]):
        raise ValueError('random_boxes: need 0 < scale[0] <= scale[1] <= 1 and 0 < ratio[0] <= ratio[1], got %r %r' % (scale, ratio))
    u = torch.rand((4, B), generator=generator, dtype=torch.float64)
    area = (scale[0] + (scale[1] - scale[0]) * u[0]) * float(min(Hs, Ws)) ** 2
    logr = torch.log(torch.tensor(ratio, dtype=torch.float64))
    asp = torch.exp(logr[0] + (logr[1] - logr[0]) * u[1])
    w = torch.sqrt(area * asp).round().clamp_(1, Ws).to(torch.int64)
    h = torch.sqrt(area / asp).round().clamp_(1, Hs).to(torch.int64)
    y0 = torch.floor(u[2] * (Hs - h + 1).to(torch.float64)).to(torch.int64).clamp_(min=0)
    x0 = torch.floor(u[3] * (Ws - w + 1).to(torch.float64)).to(torch.int64).clamp_(min=0)
    y0 = torch.minimum(y0, Hs - h)
    x0 = torch.minimum(x0, Ws - w)
    return torch.stack([y0, x0, h, w], dim=1).to(torch.int32).contiguous()
