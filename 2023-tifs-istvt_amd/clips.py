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

JPEG recompression (DESIGN.md "JPEG round trip") is the third part: ``jpeg_quant_tables``, ``check_qualities``,
``jpeg_roundtrip_host`` (the definition of ops.jpeg_roundtrip_u8, integers only) and ``random_qualities``.  Training needs no
new model code: a loader yields ``(u8, boxes, qualities, flips)`` and the step is
``model(ops.jpeg_roundtrip_u8(ops.crop_resize_u8(u8, boxes, S), q), view=flips)``.

NV12 frames (DESIGN.md "NV12 frames") are the fourth: ``nv12_coefficients``, ``check_nv12``, ``nv12_to_rgb_host`` (the
definition of ops.nv12_to_rgb_u8, integers only), ``crop_resize_nv12_host`` (of ops.crop_resize_nv12) and ``rgb_to_nv12_host``,
a plain float encoder that makes NV12 fixtures.  ``ops.crop_resize_nv12(clips_nv12, boxes, S)`` stands where
``ops.crop_resize_u8(u8, boxes, S)`` stands above.

Aligned crops (DESIGN.md "Aligned crops") are the fifth: ``check_similarities``, ``warp_similarity_host`` (the definition of
ops.warp_similarity_u8, float64), ``similarity_of_boxes``, ``similarity_from_landmarks``, ``similarities_of_squares`` and
``random_similarities``.  A
training step with rotation, scale and flip in one table is ``model(ops.warp_similarity_u8(u8, M.to(dev), S))``.

Perturbations (DESIGN.md "Perturbations") are the sixth: ``perturb_host`` (the definition of ops.perturb_u8, integers only:
brightness, contrast, saturation, Gaussian noise from Philox4x32-10, Gaussian blur with integer taps, pixelation),
``gaussian_taps``, ``check_perturbations``, ``perturbation``, ``perturbation_table``, ``random_perturbations`` and the ladder
``PERTURBATION_LEVELS``.  In training ``ops.perturb_u8(u8, table, taps, seed)`` stands where the JPEG round trip stands above.

Pasting maps onto frames (DESIGN.md "Pasting maps onto frames") is the seventh: ``paste_geometry`` (a box or a similarity as
the map from frame pixels to crop coordinates, and the rectangle to look at), ``paste_maps_host`` (the definition of
ops.relevance_paste_u8 / ops.relevance_paste_nv12: float64 field, int32 blend), ``paste_field_host`` and ``lut_to_ycc``.

JPEG files (DESIGN.md "JPEG files") are the eighth, next to the round trip whose inverse half they share: ``jpeg_parse`` (the
markers of a baseline file, and every refusal), ``jpeg_decode_host`` (the definition of ops.jpeg_decode_u8, integers only),
``jpeg_encode_host`` (files for tests and benchmarks), ``jpeg_batch`` (files packed for one launch), ``whole_boxes`` and
``check_jpeg_status``.  A loader that yields file bytes runs ``model(ops.decode_frames(files, S, boxes).view(B, T, S, S, 3),
view=flips)``: the compressed bytes are what crosses the host boundary.  Files are 4:2:0 or 4:4:4 unless a call passes
``layouts`` (DESIGN.md "JPEG layouts"): ``JPEG_LAYOUTS`` names what ``jpeg_parse``, ``jpeg_decode_host``, ``jpeg_batch``,
``ops.jpeg_decode_u8`` and ``ops.decode_frames`` can be asked to take, 4:2:2 and greyscale files among them, and
``jpeg_encode_layout_host`` writes such files for tests and benchmarks.  ``jpeg_encode_host(optimize=True)`` (DESIGN.md "JPEG
files out, optimised tables") codes a file with its own Huffman tables: ``jpeg_symbol_counts``, ``jpeg_optimal_table``
(libjpeg's, so PIL's ``optimize=True``) and ``jpeg_header_bound``; ``ops.jpeg_encode_u8(optimize=True)`` gives its bytes.
A ``JpegBank`` (DESIGN.md "JPEG bank") keeps the files of a whole set on the device: ``jpeg_bank`` packs host files,
``JpegBank.from_encoded`` takes the encoder's result where it lies, ``jpeg_bank_decode_host`` is the definition of
``ops.jpeg_decode_indexed_u8(bank, index)``, ``jpeg_scan_segments_host`` that of the device's marker scan, and
``check_jpeg_bank_status`` names the two statuses an index adds.

The batch draw (DESIGN.md "Batch draw") is the ninth: ``BatchPlan`` (which videos a run draws its clips from, the base boxes,
the shape bank of ``draw_shapes``, the probabilities as 32-bit thresholds, the seed; built and validated on the host once) and
``batch_draw_host`` (the definition of ops.batch_draw and ops.draw_clips, integers only: the file index, boxes, flips,
qualities, perturbation rows and labels of a batch as a pure function of the seed and the step).  A step that reads no host
data is ``u8, view, label, _ = ops.draw_clips(bank, plan, S)`` and ``model(u8, view=view, view_checked=True, crop=S)``.

PNG files (DESIGN.md "PNG files") are the tenth, at the end of this file: ``png_parse`` (the chunks of a file, and every
refusal), ``png_decode_host`` (the definition of ops.png_decode_u8: zlib's inflate, the five row filters, integers only),
``png_encode_host`` (files for tests and users), ``png_batch`` (files packed for one launch) and ``check_png_status``.  Frames
kept lossless on purpose run ``model(ops.decode_frames(clips.png_batch(files), S, boxes).view(B, T, S, S, 3), view=flips)``.
A whole set of them stays on the device as a ``PngBank`` (DESIGN.md "PNG bank"; ``png_bank``, ``png_bank_scratch_bytes``,
``png_bank_decode_host``, the definition of ops.png_decode_bank_u8), and ``ops.draw_clips(bank, plan, S)`` takes it as it takes
a JpegBank.  Whole video frames whose bands stand alone are decoded through their face boxes (DESIGN.md "PNG windows";
``png_window_plan``, ``png_window_rows``, ``png_bank_window_host``, the definition of ops.png_decode_window_u8): only the bands a
box touches, ``ops.decode_frames(..., window=True)`` and ``ops.draw_clips(bank, plan, S, window=True)``.
"""
import math
from fractions import Fraction
from types import SimpleNamespace
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


# ------------------------------------------------------------------------------------------ JPEG round trip
# DESIGN.md "JPEG round trip": the uint8 RGB a baseline JPEG encoder and decoder hand back at quality q, bytes to bytes and
# without a bitstream (entropy coding is lossless: quantising and de-quantising the DCT coefficients is the whole lossy
# part).  The pipeline is libjpeg's, in int32 from end to end: 16-bit fixed-point colour transforms, the 13-bit fixed-point
# "slow integer" 8-point DCT and IDCT (Loeffler, Ligtenberg and Moschytz; two passes with 2 extra bits between them, the
# forward result scaled by 8), integer quantisation.  ops.jpeg_roundtrip_u8 is the device kernel and gives these bits.
JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)           # ITU-T T.81 Annex K.1
JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32                                    # Annex K.2
JPEG_SUBSAMPLINGS = {'420': 2, '444': 1}   # chroma step per axis; the MCU is 8 * step pixels square


JFIF_COEFFICIENTS = (65536, 0, 91881, 22554, 46802, 116130)     # libjpeg's decoder: ky, yoff, krv, kgu, kgv, kbu


def _ycc_to_rgb(Y: Tensor, Cb: Tensor, Cr: Tensor, coef) -> Tensor:
    """The colour-out expression the JPEG decoder and the NV12 reader share, int32 only: Y and the centred Cb' = Cb - 128,
    Cr' = Cr - 128 as int32 tensors of one shape, coef = (ky, yoff, krv, kgu, kgv, kbu) -> uint8 (..., 3):

        yy = ky (Y - yoff);  R = clamp((yy + krv Cr' + 32768) >> 16);  G = clamp((yy - kgu Cb' - kgv Cr' + 32768) >> 16);
        B = clamp((yy + kbu Cb' + 32768) >> 16)

    with arithmetic shifts and the clamp to 0..255.  With ky = 65536 and yoff = 0, yy is a multiple of 65536 and the three
    lines are Y + ((k C' + 32768) >> 16), libjpeg's own."""
    ky, yoff, krv, kgu, kgv, kbu = coef
    yy = ky * (Y - yoff) + 32768
    return torch.stack([(yy + krv * Cr) >> 16, (yy - kgu * Cb - kgv * Cr) >> 16, (yy + kbu * Cb) >> 16],
                       dim=-1).clamp_(0, 255).to(torch.uint8)


def jpeg_quant_tables(q: int) -> Tensor:
    """The two quantisation tables of quality q in 1..100 as libjpeg scales Annex K: s = 5000 // q for q < 50, else
    200 - 2 q; entry = (base * s + 50) // 100 clamped to 1..255.  int32 (2, 8, 8): luminance, chrominance; row = vertical
    frequency."""
    q = int(q)
    if not 1 <= q <= 100:
        raise ValueError('jpeg_quant_tables: the quality must lie in [1, 100], got %d' % q)
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = torch.tensor([JPEG_LUMA, JPEG_CHROMA], dtype=torch.int32)
    return ((base * s + 50) // 100).clamp_(1, 255).reshape(2, 8, 8)


def check_qualities(quality, n: int) -> Tensor:
    """Host validation of a quality table before any launch: int32 (n,) with every entry <= 100; 1..100 compress, an entry
    <= 0 leaves its frame (or clip) unchanged.  A Python int stands for that quality everywhere.  Returns the table on the
    host (a device tensor is copied back, which waits for the device: hand over the loader's host tensor)."""
    if isinstance(quality, int) and not isinstance(quality, bool):
        quality = torch.full((n,), quality, dtype=torch.int32)
    if not torch.is_tensor(quality):
        raise TypeError('quality must be an int or an int32 tensor (n,), got %s' % type(quality).__name__)
    if quality.dtype != torch.int32:
        raise TypeError('quality must be int32, got %s' % quality.dtype)
    if quality.dim() != 1 or quality.shape[0] != n:
        raise ValueError('quality must have shape (%d,), one entry per frame or clip, got %s' % (n, tuple(quality.shape)))
    q = quality.detach().cpu()
    if bool((q > 100).any()):
        raise ValueError('quality: entries must be at most 100 (1..100 compress, <= 0 copies), got up to %d' % int(q.max()))
    return q


def _jpeg_sub(subsampling) -> int:
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("subsampling must be '420' or '444', got %r" % (subsampling,))
    return JPEG_SUBSAMPLINGS[subsampling]


def _descale(x: Tensor, n: int) -> Tensor:
    return (x + (1 << (n - 1))) >> n


def _fdct8(d, first: bool):
    """One pass of the forward DCT over 8 int32 tensors.  The first pass leaves its results scaled up by 4, the second takes
    that out again; together they give 8 x the DCT."""
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) * 4 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) * 4 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return o


def _idct8(d, first: bool):
    """One pass of the inverse DCT over 8 int32 tensors: the first keeps 2 extra bits, the second removes them and the
    forward transform's factor 8."""
    z1 = (d[2] + d[6]) * 4433
    t2, t3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    t0, t1 = (d[0] + d[4]) * 8192, (d[0] - d[4]) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    return [_descale(t10 + t3, n), _descale(t11 + t2, n), _descale(t12 + t1, n), _descale(t13 + t0, n),
            _descale(t13 - t0, n), _descale(t12 - t1, n), _descale(t11 - t2, n), _descale(t10 - t3, n)]


def _jpeg_plane(p: Tensor, qt: Tensor) -> Tensor:
    """One component through its 8 x 8 blocks: p int32 (n, Hp, Wp) samples 0..255 with Hp, Wp multiples of 8, qt int32
    (n, 8, 8) -> the reconstructed samples, int32 0..255.  Level shift, rows then columns forward, quantise (half away from
    zero) and multiply back, columns then rows inverse, + 128, clamp."""
    return _jpeg_samples(_jpeg_quantise(p, qt) * qt[:, None, :, None, :])


def _jpeg_quantise(p: Tensor, qt: Tensor) -> Tensor:
    """the forward half of _jpeg_plane: p int32 (n, Hp, Wp), qt int32 (n, 8, 8) -> the quantised coefficients a file stores,
    int32 (n, Hp / 8, 8, Wp / 8, 8) = (frame, block row, v, block column, u)"""
    n, Hp, Wp = p.shape
    b = (p - 128).reshape(n, Hp // 8, 8, Wp // 8, 8)
    b = torch.stack(_fdct8(b.unbind(4), True), dim=4)
    b = torch.stack(_fdct8(b.unbind(2), False), dim=2)                        # 8 x the coefficients
    q = qt[:, None, :, None, :]
    k = (b.abs() + q * 4) // (q * 8)                                          # (|c| + q / 2) / q in the units of the table
    return torch.where(b < 0, -k, k)


def _jpeg_samples(b: Tensor) -> Tensor:
    """the inverse half: dequantised coefficients int32 (n, bh, 8, bw, 8) -> samples int32 0..255 (n, 8 bh, 8 bw): columns
    then rows inverse, + 128, clamp"""
    n, bh, _, bw, _ = b.shape
    b = torch.stack(_idct8(b.unbind(2), True), dim=2)
    b = torch.stack(_idct8(b.unbind(4), False), dim=4)
    return (b + 128).clamp_(0, 255).reshape(n, bh * 8, bw * 8)


def _jpeg_upsample(c: Tensor, H: int, W: int) -> Tensor:
    """libjpeg's "fancy" 2 x 2 upsampling of a chroma plane int32 (n, Hc, Wc), Hc = ceil(H / 2), Wc = ceil(W / 2) -> (n, H,
    W): 3/4 of the nearer and 1/4 of the farther sample per axis, vertically first and unrounded, then horizontally with
    + 8 (even columns) or + 7 (odd ones) and >> 4; the plane's edges replicate."""
    Hc, Wc = c.shape[1], c.shape[2]
    y, x = torch.arange(H), torch.arange(W)
    near, far = y >> 1, ((y >> 1) + (y & 1) * 2 - 1).clamp_(0, Hc - 1)
    col = 3 * c[:, near] + c[:, far]
    this, other = x >> 1, ((x >> 1) + (x & 1) * 2 - 1).clamp_(0, Wc - 1)
    return (3 * col[:, :, this] + col[:, :, other] + (8 - (x & 1)).to(torch.int32)) >> 4


def _jpeg_colour_in(src: Tensor, mh: int, mw: int):
    """src uint8 (n, H, W, 3) padded to whole MCUs of mh x mw pixels by edge replication, colour in -> Y, Cb, Cr int32 (n, Hp,
    Wp), all at full resolution"""
    H, W = src.shape[1], src.shape[2]
    Hp, Wp = -(-H // mh) * mh, -(-W // mw) * mw
    rgb = src[:, torch.arange(Hp).clamp_(max=H - 1)][:, :, torch.arange(Wp).clamp_(max=W - 1)].to(torch.int32)
    R, G, B = rgb.unbind(3)
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def _jpeg_planes_in(src: Tensor, sub: int):
    """colour in, padding and downsample of jpeg_roundtrip_host: src uint8 (n, H, W, 3) on the host -> Y int32 (n, Hp, Wp)
    and Cb, Cr int32 (n, Hp / sub, Wp / sub), whole MCUs"""
    H = src.shape[1]
    Y, Cb, Cr = _jpeg_colour_in(src, 8 * sub, 8 * sub)
    Hp, Wp = Y.shape[1], Y.shape[2]
    if sub == 2:
        bias = torch.tensor([1, 2], dtype=torch.int32).repeat(Wp // 4)
        Cb, Cr = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + bias) >> 2 for c in (Cb, Cr))
        rows = torch.arange(Hp // 2).clamp_(max=(H + 1) // 2 - 1)              # below the frame: the last chroma row again
        Cb, Cr = Cb[:, rows], Cr[:, rows]
    return Y, Cb, Cr


def jpeg_roundtrip_host(u8: Tensor, quality, subsampling: str = '420') -> Tensor:
    """The definition on the host: uint8 (n, H, W, 3) or (B, T, H, W, 3), any H, W >= 1, and quality int32 (n,) / (B,) (one
    entry per frame, or per clip and shared by its T frames; an int for all) -> the uint8 RGB of the same shape that a
    baseline JPEG encoder and decoder would hand back.  Entries 1..100 compress, an entry <= 0 copies the frame.  int32
    arithmetic only:

      colour in    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16;  Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767)
                   >> 16;  Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
      padding      to whole MCUs (16 x 16 pixels for '420', 8 x 8 for '444') by edge replication
      downsample   '420': 2 x 2 box, (sum + bias) >> 2, bias 1, 2, 1, 2, ... along a row; chroma rows below the frame's
                   ceil(H / 2) repeat the last of those (libjpeg pads the width and an odd height before the downsample,
                   the rest of the height after it)
      blocks       _jpeg_plane with jpeg_quant_tables(q): luminance table for Y, chrominance table for Cb and Cr
      upsample     '420': _jpeg_upsample on the ceil(H / 2) x ceil(W / 2) chroma samples that belong to the frame
      colour out   R = Y + ((91881 Cr' + 32768) >> 16);  G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16);  B = Y +
                   ((116130 Cb' + 32768) >> 16) with Cb' = Cb - 128, Cr' = Cr - 128; clamp to 0..255; crop to H x W

    No product or sum leaves int32: the samples have 8 bits, the colour constants 17, the DCT constants 15 with at most 13
    bits of headroom used by the passes (libjpeg's own argument for its 32-bit "slow integer" transforms)."""
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3 or u8.numel() == 0:
        raise ValueError('jpeg_roundtrip_host expects non-empty uint8 (n, H, W, 3) or (B, T, H, W, 3), got %s %s'
                         % (u8.dtype, tuple(u8.shape)))
    sub = _jpeg_sub(subsampling)
    q = check_qualities(quality, u8.shape[0])
    if u8.dim() == 5:
        q = q.repeat_interleave(u8.shape[1])
    H, W = u8.shape[-3], u8.shape[-2]
    src = u8.reshape((-1, H, W, 3)).cpu()
    Y, Cb, Cr = _jpeg_planes_in(src, sub)
    tables = torch.stack([jpeg_quant_tables(min(max(int(v), 1), 100)) for v in q])       # (n, 2, 8, 8); unused where q <= 0
    Y = _jpeg_plane(Y, tables[:, 0])[:, :H, :W]
    Cb, Cr = _jpeg_plane(Cb, tables[:, 1]), _jpeg_plane(Cr, tables[:, 1])
    if sub == 2:
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        Cb, Cr = _jpeg_upsample(Cb[:, :Hc, :Wc], H, W), _jpeg_upsample(Cr[:, :Hc, :Wc], H, W)
    else:
        Cb, Cr = Cb[:, :H, :W], Cr[:, :H, :W]
    out = _ycc_to_rgb(Y, Cb - 128, Cr - 128, JFIF_COEFFICIENTS)
    keep = q <= 0
    out[keep] = src[keep]
    return out.reshape(u8.shape).to(u8.device)


def random_qualities(n: int, p: float = 0.5, lo: int = 30, hi: int = 95, generator: Optional[torch.Generator] = None) -> Tensor:
    """One random quality per frame or clip for compression augmentation: 0 (leave it alone) with probability 1 - p, otherwise
    uniform in [lo, hi].  Returns an int32 (n,) host tensor (contiguous: ready for pin_memory()), reproducible from
    `generator`."""
    if n < 1:
        raise ValueError('random_qualities: need n >= 1, got %d' % n)
    if not 0.0 <= p <= 1.0:
        raise ValueError('random_qualities: p must be a probability, got %r' % (p,))
    if not 1 <= lo <= hi <= 100:
        raise ValueError('random_qualities: need 1 <= lo <= hi <= 100, got lo=%r hi=%r' % (lo, hi))
    on = torch.rand((n,), generator=generator) < p
    q = torch.randint(lo, hi + 1, (n,), generator=generator)
    return torch.where(on, q, torch.zeros_like(q)).to(torch.int32).contiguous()


# ------------------------------------------------------------------------------------------ JPEG files
# DESIGN.md "JPEG files": baseline JPEG files decoded on the device.  jpeg_parse reads a file's markers, jpeg_decode_host is
# the definition of ops.jpeg_decode_u8 (canonical Huffman decoding in front of the inverse half of the round trip above),
# jpeg_encode_host writes files for tests and benchmarks, jpeg_batch packs files for one launch.
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
               62, 63)                                  # natural index of the k-th coefficient of a block (T.81 figure A.6)
JPEG_MAX_SIDE = 16384
# the ISTVT_JPEG_* sizes of include/istvt_hip.h (tests/test_abi_cpu.py holds the two together)
JPEG_HUFF_INTS = 288                        # a decode table: limit[16], offset[16], values[256] (csrc/jpeg_entropy.h)
JPEG_IMAGE_INTS = 20                        # a row of the per-image table
JPEG_IDCT_BLOCKS = 24                       # blocks per workgroup of the IDCT kernel
# The layouts a file may have: '420' / '444' / '422' are three components sampled 2x2 / 1x1 / 2x1 (Y) and 1x1 (Cb, Cr), 'grey'
# is Y alone.  What a call accepts is opt-in: without a `layouts` argument it is JPEG_LAYOUTS_DEFAULT.
JPEG_LAYOUTS = ('420', '444', '422', 'grey')
JPEG_LAYOUTS_DEFAULT = ('420', '444')
JPEG_SAMPLINGS = {((2, 2), (1, 1), (1, 1)): '420', ((1, 1), (1, 1), (1, 1)): '444', ((2, 1), (1, 1), (1, 1)): '422'}
JPEG_LAYOUT_CODES = {'420': 0, '444': 0, '422': 1, 'grey': 2}     # the last int of an images row: ISTVT_JPEG_LAYOUT_*


def _std_ac(head, runs):
    """the tail of an Annex K.3 AC value list: after `head`, run r carries sizes lo..10"""
    return tuple(head) + tuple((r << 4) | s for r, lo in runs for s in range(lo, 11))


# ITU-T T.81 Annex K.3: (number of codes of length 1..16, values in code order) of the four typical Huffman tables
JPEG_STD_HUFFMAN = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), _std_ac(
        (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
         0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a),
        ((1, 6), (2, 5), (3, 4), (4, 3), (5, 3), (6, 3), (7, 3), (8, 3), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 1),
         (15, 1)))),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _std_ac(
        (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
         0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
         0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a),
        ((2, 6), (3, 5), (4, 3), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 2), (15, 2)))),
}


class JpegHeader:
    """What jpeg_parse reads from one baseline file.  H, W; layout: one of JPEG_LAYOUTS; factors: (h, v), the luma blocks of
    an MCU per axis ((1, 1) for 'grey': a one-component scan has one block per MCU whatever the file's factors say); sub: the
    horizontal chroma step h (2 at 4:2:0, 1 at 4:4:4); mcus = (rows, columns) of MCUs, which are 8 h x 8 v pixels; quant: per
    component the file has, the 64 entries of its table in natural order; huffman: per component, ((counts, values) of its
    DC table, (counts, values) of its AC table); restart_interval (0: none); segments: [(begin, end)] byte ranges of `data`
    between the restart markers, one per restart interval; eoi: whether the scan ended with EOI."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def mcu_blocks(self) -> tuple:
        """the component of every block of an MCU, in the order of the scan: (0, 0, 0, 0, 1, 2) at 4:2:0, (0,) for 'grey'"""
        h, v = self.factors
        return (0,) * (h * v) + tuple(range(1, len(self.quant)))

    @property
    def block_factors(self) -> list:
        """per component, its (h, v) blocks in an MCU"""
        return [self.factors] + [(1, 1)] * (len(self.quant) - 1)


def _jpeg_refuse(text: str):
    raise ValueError('jpeg_parse: ' + text)


def _jpeg_layouts(layouts, who: str = 'jpeg_parse') -> tuple:
    """the `layouts` argument: a tuple of names from JPEG_LAYOUTS, or 'all'"""
    if isinstance(layouts, str) and layouts == 'all':
        return JPEG_LAYOUTS
    names = layouts if isinstance(layouts, (tuple, list)) else ()
    if not names or any(not isinstance(v, str) or v not in JPEG_LAYOUTS for v in names):
        raise ValueError("%s: layouts is 'all' or a tuple of names from %r, got %r" % (who, JPEG_LAYOUTS, layouts))
    return tuple(layouts)


def jpeg_parse(data, layouts=JPEG_LAYOUTS_DEFAULT) -> JpegHeader:
    """The markers of one baseline JPEG file (bytes): SOI, APPn / COM (skipped), DQT, SOF0, DHT, DRI, SOS, and RSTn / EOI
    inside the scan.  Accepted: 8-bit precision, one scan of all components, 8-bit quantisation tables, and the layouts named
    in `layouts` (a tuple of names from JPEG_LAYOUTS, or 'all'): three components sampled 2x2 / 1x1 / 1x1 ('420'), 1x1 / 1x1 /
    1x1 ('444') or 2x1 / 1x1 / 1x1 ('422'), or one component ('grey', whose sampling factors are read and ignored: T.81
    A.2.2).  By default '420' and '444' alone.  Everything else is refused by name (ValueError, 'jpeg_parse: ...').  A scan
    that ends without EOI runs to the end of the data; restart intervals it no longer holds become empty segments, and
    decoding reports status 1."""
    layouts = _jpeg_layouts(layouts)
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        _jpeg_refuse('the file does not start with SOI (FF D8)')
    pos = 2
    quant, huff = {}, {}
    frame = None
    ri = 0
    while True:
        if pos + 4 > n:
            _jpeg_refuse('the file has no SOS: it ends at byte %d inside its headers' % n)
        if data[pos] != 0xFF:
            _jpeg_refuse('a marker expected at byte %d, got %02X' % (pos, data[pos]))
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos + 3 > n:
            _jpeg_refuse('the file has no SOS: it ends at byte %d inside its headers' % n)
        m = data[pos]
        pos += 1
        if m == 0xD9:
            _jpeg_refuse('the file has no SOS: EOI at byte %d' % (pos - 2))
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2 or pos + length > n:
            _jpeg_refuse('segment %02X at byte %d reaches past the end of the file' % (m, pos - 2))
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xDA:
            break
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            if m == 0xEE and seg[:5] == b'Adobe' and len(seg) >= 12 and seg[11] == 0:
                _jpeg_refuse('an Adobe APP14 segment with transform 0 (RGB or CMYK samples, not YCbCr)')
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    _jpeg_refuse('16-bit quantisation table %d' % tq)
                if tq > 3 or at + 65 > len(seg):
                    _jpeg_refuse('a malformed DQT segment')
                t = [0] * 64
                for k in range(64):
                    t[JPEG_ZIGZAG[k]] = seg[at + 1 + k]
                if min(t) < 1:
                    _jpeg_refuse('quantisation table %d has a zero entry' % tq)
                quant[tq] = tuple(t)
                at += 65
        elif m == 0xC0:
            if frame is not None:
                _jpeg_refuse('a second SOF0')
            if len(seg) < 6:
                _jpeg_refuse('a malformed SOF0 segment')
            if seg[0] != 8:
                _jpeg_refuse('%d-bit precision (8 expected)' % seg[0])
            H, W, nf = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nf != 3 and not (nf == 1 and 'grey' in layouts):
                _jpeg_refuse('%d component%s (three expected: Y, Cb, Cr%s)'
                             % (nf, '' if nf == 1 else 's', '; or one' if 'grey' in layouts else ''))
            if len(seg) != 6 + 3 * nf:
                _jpeg_refuse('a malformed SOF0 segment')
            if H < 1 or W < 1:
                _jpeg_refuse('zero width or height (%d x %d)' % (H, W))
            if H > JPEG_MAX_SIDE or W > JPEG_MAX_SIDE:
                _jpeg_refuse('a side above %d (%d x %d)' % (JPEG_MAX_SIDE, H, W))
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nf)]
            samp = tuple((h, v) for _, h, v, _ in comps)
            layout = 'grey' if nf == 1 else JPEG_SAMPLINGS.get(samp)
            if layout not in layouts:
                # a layout that has a name and was not asked for is refused as it always was
                names = [k for k, v in JPEG_SAMPLINGS.items() if v in (JPEG_LAYOUTS_DEFAULT if layout else layouts)]
                names = ['/'.join('%dx%d' % s for s in k) for k in names]
                _jpeg_refuse('sampling %s (%s expected)' % ('/'.join('%dx%d' % s for s in samp),
                                                            ' or '.join([', '.join(names[:-1])] * (len(names) > 1) + names[-1:])))
            frame = (H, W, comps, layout)
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            _jpeg_refuse('%s (SOF%d); baseline SOF0 expected'
                         % ('progressive' if m in (0xC2, 0xC6, 0xCA, 0xCE) else 'not baseline', m - 0xC0))
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = seg[at] >> 4, seg[at] & 15
                if tc > 1 or th > 3 or at + 17 > len(seg):
                    _jpeg_refuse('a malformed DHT segment')
                counts = tuple(seg[at + 1:at + 17])
                total = sum(counts)
                space = 1                                 # codes still free at this length
                for c in counts:
                    space = 2 * space - c
                    if space < 0:
                        _jpeg_refuse('Huffman table %d/%d assigns more codes than its lengths hold' % (tc, th))
                if total > 256 or at + 17 + total > len(seg):
                    _jpeg_refuse('a malformed DHT segment')
                huff[(tc, th)] = (counts, tuple(seg[at + 17:at + 17 + total]))
                at += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                _jpeg_refuse('a malformed DRI segment')
            ri = (seg[0] << 8) | seg[1]
        else:
            _jpeg_refuse('marker %02X at byte %d is not part of a baseline file' % (m, pos - length - 2))
    if frame is None:
        _jpeg_refuse('SOS before SOF0')
    H, W, comps, layout = frame
    nf = len(comps)
    ns = seg[0] if seg else 0
    if ns != nf:
        _jpeg_refuse('several scans: the first holds %d of the %d component%s (one %s expected)'
                     % (ns, nf, 's' if nf > 1 else '', 'interleaved scan' if nf > 1 else 'scan'))
    if len(seg) != 1 + 2 * ns + 3:
        _jpeg_refuse('a malformed SOS segment')
    if tuple(seg[1 + 2 * ns:]) != (0, 63, 0):
        _jpeg_refuse('a scan of coefficients %d..%d, approximation %02X (progressive); 0..63 expected' % tuple(seg[1 + 2 * ns:]))
    tables = []
    for c in range(nf):
        if seg[1 + 2 * c] != comps[c][0]:
            _jpeg_refuse('the scan lists component %d where the frame has %d' % (seg[1 + 2 * c], comps[c][0]))
        td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
        if comps[c][3] not in quant:
            _jpeg_refuse('component %d refers to quantisation table %d, which the file never defines' % (c, comps[c][3]))
        if (0, td) not in huff:
            _jpeg_refuse('component %d refers to DC Huffman table %d, which the file never defines' % (c, td))
        if (1, ta) not in huff:
            _jpeg_refuse('component %d refers to AC Huffman table %d, which the file never defines' % (c, ta))
        tables.append((huff[(0, td)], huff[(1, ta)]))
    factors = (1, 1) if layout == 'grey' else (comps[0][1], comps[0][2])
    mcus = (-(-H // (8 * factors[1])), -(-W // (8 * factors[0])))
    # the scan: stuffed FF 00 pairs are data, RSTn splits it, any other marker ends it
    segments, marks = [], []
    begin = at = pos
    eoi, end = False, n
    while at < n:
        if data[at] != 0xFF:
            at += 1
            continue
        k = at + 1
        while k < n and data[k] == 0xFF:                 # fill bytes in front of a marker
            k += 1
        if k >= n:
            break                                         # FF at the very end: the scan runs to the end of the data
        if data[k] == 0 and k == at + 1:
            at += 2
            continue
        if 0xD0 <= data[k] <= 0xD7:
            segments.append((begin, at))
            marks.append(data[k] - 0xD0)
            begin = at = k + 1
            continue
        end, eoi = at, data[k] == 0xD9
        if not eoi:
            _jpeg_refuse('several scans: marker %02X follows the first scan at byte %d' % (data[k], at))
        break
    segments.append((begin, end))
    total = mcus[0] * mcus[1]
    want = -(-total // ri) if ri else 1
    if marks != [i % 8 for i in range(len(marks))]:
        _jpeg_refuse('restart markers out of sequence: RST%s' % ', RST'.join(str(v) for v in marks[:16]))
    if len(segments) > want or (eoi and len(segments) != want):
        _jpeg_refuse('%d restart intervals in the scan, %d expected (%d MCUs, restart interval %d)'
                     % (len(segments), want, total, ri))
    segments += [(end, end)] * (want - len(segments))
    return JpegHeader(H=H, W=W, layout=layout, factors=factors, sub=factors[0], mcus=mcus,
                      quant=tuple(quant[c[3]] for c in comps), huffman=tuple(tables), restart_interval=ri, segments=segments,
                      eoi=eoi, data=data)


def jpeg_huffman_table(counts, values):
    """The decode form of one Huffman table (csrc/jpeg_entropy.h reads the same 288 ints): with c the next 16 bits of the
    stream, the code has the smallest length l with c < limit[l - 1], and its value is values[(offset[l - 1] + (c >>
    (16 - l))) & 255].  limit[l - 1] = (first code of length l + number of such codes) << (16 - l): canonical codes of one
    length are consecutive (T.81 F.2.2.3), so limit does not decrease."""
    limit, offset = [], []
    code = at = 0
    for l in range(1, 17):
        offset.append(at - code)
        code += counts[l - 1]
        at += counts[l - 1]
        limit.append(code << (16 - l))
        code <<= 1
    return limit + offset + list(values) + [0] * (256 - len(values))


class _JpegBits:
    """The bit reader of a segment: bytes [pos, end) of data, FF 00 un-stuffed, zeros fed past the end (status 1 once one of
    them is consumed).  At most 23 bits wait in buf."""

    def __init__(self, data, pos, end):
        self.data, self.pos, self.end = data, pos, end
        self.buf = self.n = self.fake = self.status = 0

    def need(self, k):
        while self.n < k:
            b = 0
            if self.pos < self.end:
                b = self.data[self.pos]
                self.pos += 1
                if b == 0xFF and self.pos < self.end and self.data[self.pos] == 0:
                    self.pos += 1
            else:
                self.fake += 8
            self.buf = ((self.buf << 8) | b) & 0xFFFFFFFF
            self.n += 8

    def skip(self, k):
        self.n -= k
        if self.n < self.fake:
            self.status, self.fake = max(self.status, 1), self.n

    def huffman(self, t):
        self.need(16)
        c = (self.buf >> (self.n - 16)) & 0xFFFF
        for l in range(1, 17):
            if c < t[l - 1]:
                self.skip(l)
                return t[32 + ((t[16 + l - 1] + (c >> (16 - l))) & 255)]
        return -1

    def receive(self, s):
        """s <= 15 bits, extended to a signed value (T.81 F.2.2.1)"""
        self.need(s)
        r = (self.buf >> (self.n - s)) & ((1 << s) - 1)
        self.skip(s)
        return r if r >= (1 << (s - 1)) else r - (1 << s) + 1


def _jpeg_block(bits: _JpegBits, dc, ac, pred: int, out) -> tuple:
    """one block into out (64 ints, natural order, zero on entry) -> (error status or 0, the new DC prediction)"""
    s = bits.huffman(dc)
    if s < 0 or s > 11:
        return 2, pred
    if s:
        pred = ((pred + bits.receive(s) + 32768) & 65535) - 32768   # the prediction lives in the int16 a coefficient has
    out[0] = pred
    k = 1
    while k < 64:
        rs = bits.huffman(ac)
        if rs < 0:
            return 2, pred
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            if k > 64:
                return 3, pred
            continue
        k += r
        if k > 63:
            return 3, pred
        out[JPEG_ZIGZAG[k]] = bits.receive(s)
        k += 1
    return 0, pred


def _jpeg_coefficients(hd: JpegHeader):
    """every segment of a parsed file through the entropy decoder -> (coefficient planes [Y, Cb, Cr] ([Y] for 'grey'), int32
    (block rows, 8, block columns, 8) in natural order and whole MCUs, status)"""
    fac, (my, mx) = hd.block_factors, hd.mcus
    planes = [torch.zeros((my * v, mx * h, 64), dtype=torch.int32) for h, v in fac]
    tabs = [(jpeg_huffman_table(*dc), jpeg_huffman_table(*ac)) for dc, ac in hd.huffman]
    ri = hd.restart_interval or my * mx
    status = 0
    for i, (begin, end) in enumerate(hd.segments):
        bits = _JpegBits(hd.data, begin, end)
        pred, dead = [0] * len(fac), 0
        for mcu in range(i * ri, min((i + 1) * ri, my * mx)):
            y, x = divmod(mcu, mx)
            for c, (nh, nv) in enumerate(fac):
                for v in range(nv):
                    for h in range(nh):
                        if dead:
                            continue                      # the rest of the segment's blocks stay zero
                        blk = [0] * 64
                        dead, pred[c] = _jpeg_block(bits, tabs[c][0], tabs[c][1], pred[c], blk)
                        planes[c][y * nv + v, x * nh + h] = torch.tensor(blk, dtype=torch.int32)
        status = max(status, dead, bits.status)
    return [p.reshape(p.shape[0], p.shape[1], 8, 8).permute(0, 2, 1, 3) for p in planes], status


def _jpeg_upsample_h2v1(c: Tensor, W: int) -> Tensor:
    """libjpeg's "fancy" h2v1 upsampling of a 4:2:2 chroma plane int32 (n, H, Wc), Wc = ceil(W / 2) -> (n, H, W): 3/4 of the
    nearer and 1/4 of the farther sample of the row, + 1 (even columns) or + 2 (odd ones), >> 2; the plane's edges replicate"""
    x = torch.arange(W)
    this, other = x >> 1, ((x >> 1) + (x & 1) * 2 - 1).clamp_(0, c.shape[2] - 1)
    return (3 * c[:, :, this] + c[:, :, other] + (1 + (x & 1)).to(torch.int32)) >> 2


def jpeg_decode_host(data, return_status: bool = False, layouts=JPEG_LAYOUTS_DEFAULT):
    """The definition of ops.jpeg_decode_u8, int32 only: one baseline file (bytes, parsed with `layouts`, or a JpegHeader) ->
    uint8 (H, W, 3), with return_status=True (frame, status).

      entropy      canonical Huffman decoding (T.81 F.2.2) of each restart interval: bytes un-stuffed, the DC prediction
                   reset at each restart, coefficients de-zigzagged
      blocks       times the file's own table; _idct8 columns then rows; + 128; clamp
      chroma       cut to the ceil(H / 2) x ceil(W / 2) samples that belong to the frame, then _jpeg_upsample ('420'); cut to
                   H x ceil(W / 2), then _jpeg_upsample_h2v1, which has no vertical step ('422'); none: Cb = Cr = 128 ('grey')
      colour out   _ycc_to_rgb(..., JFIF_COEFFICIENTS); crop to H x W.  For 'grey' that is R = G = B = Y

    status: 0 fine | 1 bits were needed past the end of a segment (zeros are fed) | 2 a 16-bit prefix with no code, or a DC
    category above 11 | 3 a run that carries the coefficient index past 63.  After 2 or 3 the rest of that segment's blocks
    are zero; the largest status of a file's segments is the file's.  The device gives these bytes where the status is 0
    and the dequantised blocks stay inside libjpeg's 32-bit argument (every file an encoder makes from 8-bit samples)."""
    hd = data if isinstance(data, JpegHeader) else jpeg_parse(data, layouts)
    coef, status = _jpeg_coefficients(hd)
    H, W = hd.H, hd.W
    planes = [_jpeg_samples((c * torch.tensor(q, dtype=torch.int32).reshape(8, 1, 8)[None])[None]) for c, q in zip(coef, hd.quant)]
    Y = planes[0]
    Cb, Cr = planes[1:] if hd.layout != 'grey' else (torch.full_like(Y, 128),) * 2
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    if hd.layout == '420':
        Cb, Cr = _jpeg_upsample(Cb[:, :Hc, :Wc], H, W), _jpeg_upsample(Cr[:, :Hc, :Wc], H, W)
    elif hd.layout == '422':
        Cb, Cr = _jpeg_upsample_h2v1(Cb[:, :H, :Wc], W), _jpeg_upsample_h2v1(Cr[:, :H, :Wc], W)
    out = _ycc_to_rgb(Y[:, :H, :W], Cb[:, :H, :W] - 128, Cr[:, :H, :W] - 128, JFIF_COEFFICIENTS)[0]
    return (out, status) if return_status else out


def check_jpeg_status(status) -> None:
    """reads the status table of ops.jpeg_decode_u8 back (this waits for the device) and raises for the first damaged file"""
    names = {1: 'its scan ends early', 2: 'a Huffman code or DC category no table holds', 3: 'a run past coefficient 63'}
    for i, s in enumerate(status.detach().cpu().tolist()):
        if s != 0:
            raise ValueError('jpeg_decode: file %d is damaged (status %d: %s)' % (i, s, names.get(s, 'unknown')))


def _huffman_codes(counts, values):
    """value -> (code, length) of a canonical table"""
    codes, code, at = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            codes[values[at]] = (code, l)
            code += 1
            at += 1
        code <<= 1
    return codes


JPEG_LAYOUT_FACTORS = {'420': ((2, 2), (1, 1), (1, 1)), '444': ((1, 1), (1, 1), (1, 1)), '422': ((2, 1), (1, 1), (1, 1)),
                       'grey': ((1, 1),)}      # (h, v) of a layout's components: the MCU is 8 h x 8 v pixels of Y


def _jpeg_encode_layout(subsampling, layout, who: str) -> str:
    """The layout an encoder call names: subsampling ('420' or '444') where layout is None, else layout, one of JPEG_LAYOUTS,
    which then stands alone: '420' and '444' are the subsampling of that name."""
    if layout is None:
        _jpeg_sub(subsampling)
        return subsampling
    if layout not in JPEG_LAYOUTS:
        raise ValueError("%s: layout must be one of '420', '444', '422', 'grey', got %r" % (who, layout))
    if subsampling != '420':
        raise ValueError('%s: layout=%r takes the place of subsampling: leave subsampling at its default, got %r'
                         % (who, layout, subsampling))
    return layout


def jpeg_restart_interval(restart_interval, W: int, subsampling: str = '420', layout=None) -> int:
    """The restart interval in MCUs that a file's DRI segment carries: an int in 0..65535 (0: no restart markers) as it is,
    or 'row' for one MCU row, ceil(W / (8 * sub)) MCUs -- the interval that gives the device decoder one lane per MCU row.
    layout (one of JPEG_LAYOUTS, in the place of subsampling): a row is ceil(W / 16) MCUs at '422' and ceil(W / 8) at 'grey'."""
    sub = JPEG_LAYOUT_FACTORS[_jpeg_encode_layout(subsampling, layout, 'jpeg_restart_interval')][0][0]
    if isinstance(restart_interval, str):
        if restart_interval != 'row':
            raise ValueError("the restart interval is an int in [0, 65535] or 'row', got %r" % (restart_interval,))
        return -(-int(W) // (8 * sub))
    ri = int(restart_interval)
    if not 0 <= ri <= 65535:
        raise ValueError('the restart interval must lie in [0, 65535], got %d' % ri)
    return ri


JPEG_HEADER_DQT = (25, 94)                  # where the 64 bytes of the two quantisation tables lie in jpeg_header's bytes
JPEG_HEADER_DHT = (177, 609)                # where the four Huffman table segments of jpeg_header's bytes begin and end
JPEG_HEADER_DHT_GREY = (171, 603)           # ... in a one-component header: its SOF0 is 6 bytes shorter (and its SOS 4)


def jpeg_header_dht(layout: str) -> tuple:
    """JPEG_HEADER_DHT for a layout of JPEG_LAYOUTS: the quantisation tables lie in front of SOF0, at JPEG_HEADER_DQT always"""
    return JPEG_HEADER_DHT_GREY if layout == 'grey' else JPEG_HEADER_DHT


def jpeg_header(H: int, W: int, quality: int, subsampling: str = '420', restart_interval=0, layout=None) -> bytes:
    """SOI through the SOS header of the file jpeg_encode_host writes for an H x W frame: JFIF APP0, the two quantisation
    tables of `quality` in zig-zag order (at JPEG_HEADER_DQT), SOF0, the four Annex K.3 Huffman tables, DRI where the
    restart interval is not 0, SOS.  Everything but the 2 x 64 table bytes is shared by the frames of a batch.
    layout (one of JPEG_LAYOUTS, in the place of subsampling): 'grey' names one component in SOF0 and SOS and still holds all
    six tables, the Huffman ones at JPEG_HEADER_DHT_GREY."""
    word = _jpeg_encode_layout(subsampling, layout, 'jpeg_header')
    H, W = int(H), int(W)
    if not (1 <= H <= JPEG_MAX_SIDE and 1 <= W <= JPEG_MAX_SIDE):
        raise ValueError('jpeg_header: frames of 1 x 1 to %d x %d, got %d x %d' % (JPEG_MAX_SIDE, JPEG_MAX_SIDE, H, W))
    ri = jpeg_restart_interval(restart_interval, W, subsampling, layout)
    return _jpeg_header(H, W, quality, list(JPEG_LAYOUT_FACTORS[word]), ri)


def _jpeg_header(H: int, W: int, quality: int, fac, ri: int, tables=None) -> bytes:
    """jpeg_header for components sampled fac = [(h, v)]: Y, or Y, Cb, Cr; component c has id c + 1, and all but Y take the
    second quantisation table and the second pair of Huffman tables.  All six tables are written whatever the components.
    tables: {(class, id): (counts, values)} of the four Huffman tables, JPEG_STD_HUFFMAN by default"""
    tables = JPEG_STD_HUFFMAN if tables is None else tables
    qt = jpeg_quant_tables(quality)
    zz = torch.tensor(JPEG_ZIGZAG)
    out = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(2):
        out += b'\xff\xdb\x00\x43' + bytes([t]) + bytes(qt[t].reshape(64)[zz].tolist())
    out += b'\xff\xc0' + bytes([0, 8 + 3 * len(fac), 8, H >> 8, H & 255, W >> 8, W & 255, len(fac)])
    for c, (h, v) in enumerate(fac):
        out += bytes([c + 1, (h << 4) | v, min(c, 1)])
    for (tc, th), (counts, values) in sorted(tables.items()):
        out += b'\xff\xc4' + bytes([(19 + len(values)) >> 8, (19 + len(values)) & 255, (tc << 4) | th]) + bytes(counts) + bytes(values)
    if ri:
        out += b'\xff\xdd\x00\x04' + bytes([ri >> 8, ri & 255])
    out += b'\xff\xda' + bytes([0, 6 + 2 * len(fac), len(fac)])
    for c in range(len(fac)):
        out += bytes([c + 1, 0x11 * min(c, 1)])
    return bytes(out + b'\x00\x3f\x00')


def jpeg_symbol_counts(coef, fac, my: int, mx: int, ri: int) -> list:
    """How often the scan of _jpeg_scan(out, coef, fac, my, mx, ri) uses every Huffman symbol -> four lists of 256 counts: DC
    and AC of table id 0 (Y), then DC and AC of table id 1 (the rest).  The walk is _jpeg_scan's: the DC prediction starts
    at 0 and again every ri MCUs (0: never again), a ZRL per 16 zeros in front of a coded coefficient, an EOB where zeros
    end the block.  Values are clamped as the device coder clamps them: a DC difference to +-2047, an AC value to +-1023."""
    counts = [[0] * 256 for _ in range(4)]
    pred = [0] * len(fac)
    for mcu in range(my * mx):
        if ri and mcu and mcu % ri == 0:
            pred = [0] * len(fac)
        y, x = divmod(mcu, mx)
        for c, (nh, nv) in enumerate(fac):
            dc, ac = counts[2 * min(c, 1)], counts[2 * min(c, 1) + 1]
            for v in range(nv):
                for h in range(nh):
                    blk = coef[c][y * nv + v][x * nh + h]
                    diff = max(-2047, min(2047, blk[0] - pred[c]))
                    pred[c] = blk[0]
                    dc[abs(diff).bit_length()] += 1
                    run = 0
                    for k in range(1, 64):
                        if blk[k] == 0:
                            run += 1
                            continue
                        ac[0xF0] += run >> 4
                        ac[((run & 15) << 4) | abs(max(-1023, min(1023, blk[k]))).bit_length()] += 1
                        run = 0
                    if run:
                        ac[0] += 1
    return counts


def jpeg_code_lengths(counts):
    """The first half of jpeg_optimal_table: 256 symbol counts -> (lengths of the 257 symbols before any limiting, 0 for a
    symbol without a count; the symbols with one, ascending).  No length is above 32."""
    counts = [int(c) for c in counts]
    if len(counts) != 256 or min(counts) < 0:
        raise ValueError('jpeg_optimal_table: 256 non-negative counts expected')
    if not any(counts):
        return [0] * 257, []
    for shift in range(33):
        freq = [(c + (1 << shift) - 1) >> shift for c in counts] + [1]
        live = [s for s in range(257) if freq[s]]
        size, others = [0] * 257, [-1] * 257
        while True:
            c1 = c2 = -1
            for s in live:
                if freq[s] and (c1 < 0 or freq[s] <= freq[c1]):
                    c1 = s
            for s in live:
                if freq[s] and s != c1 and (c2 < 0 or freq[s] <= freq[c2]):
                    c2 = s
            if c2 < 0:
                break
            freq[c1] += freq[c2]
            freq[c2] = 0
            size[c1] += 1
            while others[c1] >= 0:
                c1 = others[c1]
                size[c1] += 1
            others[c1] = c2                                       # the chain of c2 behind the chain of c1
            size[c2] += 1
            while others[c2] >= 0:
                c2 = others[c2]
                size[c2] += 1
        if max(size) <= 32:
            break
    return size, live


def jpeg_optimal_table(counts):
    """256 symbol counts -> (counts16, values): the Huffman table libjpeg's jpeg_gen_optimal_table makes of them, which is
    what PIL writes with optimize=True.  A reserved symbol 256 with count 1 joins the counted ones, so that no code is all
    ones.  The two smallest non-zero counts are merged until one is left; among equal counts the larger symbol is taken, for
    the first and for the second.  A symbol's code length is the number of merges its chain of `others` went through.
    Lengths above 16 are folded down by the loop of T.81 K.2 from length 32: two codes of length i become one of length
    i - 1, and a code of the longest shorter length j becomes two of length j + 1.  One code of the longest length is taken
    out, the reserved symbol's.  Values are ordered by length, then by symbol.  Where a length would pass 32 (libjpeg stops
    there; the counts of no image of JPEG_MAX_SIDE do it unless they grow like Fibonacci numbers) every count is halved,
    rounding up, and the merging starts again: at most 32 times, after which all counts are 1.
    All-zero counts give an empty table, 16 zero counts and no values: no scan symbol refers to such a table, since a
    component that is coded counts a DC symbol and an AC symbol (a coefficient or EOB) in every block.
    csrc/jpeg_entropy_opt.h (jo_optimal_table) is the same steps for the device."""
    size, live = jpeg_code_lengths(counts)
    if not live:
        return (0,) * 16, ()
    bits = [0] * 33
    for s in live:
        bits[size[s]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while j > 0 and bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    values = tuple(s for l in range(1, 33) for s in live if s < 256 and size[s] == l)
    return tuple(bits[1:17]), values


def jpeg_optimal_tables(coef, fac, my: int, mx: int, ri: int) -> dict:
    """{(class, id): (counts, values)} as _jpeg_header and _jpeg_scan take it: jpeg_optimal_table of jpeg_symbol_counts"""
    dc0, ac0, dc1, ac1 = (jpeg_optimal_table(c) for c in jpeg_symbol_counts(coef, fac, my, mx, ri))
    return {(0, 0): dc0, (0, 1): dc1, (1, 0): ac0, (1, 1): ac1}


def jpeg_header_bound(H: int, W: int, subsampling: str = '420', restart_interval=0, layout=None) -> int:
    """The largest header a file of jpeg_encode_host(optimize=True) can have.  A DC table holds at most the 12 categories
    0..11 and an AC table at most 160 (run, size) pairs, EOB and ZRL, since the coder clamps a DC difference to +-2047 and an
    AC value to +-1023: as many values as the Annex K.3 tables list, so the bound is the length of jpeg_header -- in every
    layout, since the argument counts symbols, not components."""
    return len(jpeg_header(H, W, 50, subsampling, restart_interval, layout))


def jpeg_encode_host(u8: Tensor, quality: int, subsampling: str = '420', restart_interval=0, optimize: bool = False,
                     layout=None) -> bytes:
    """A baseline JFIF file of one frame, the definition of ops.jpeg_encode_u8: u8 uint8 (H, W, 3) -> bytes.  The front half
    of jpeg_roundtrip_host (colour in, padding, downsample, _fdct8, quantise with jpeg_quant_tables(quality)), then Huffman
    coding with the Annex K.3 tables, a restart marker every restart_interval MCUs (0: none; 'row': every MCU row,
    jpeg_restart_interval).  Its defining property:
    jpeg_decode_host(jpeg_encode_host(x, q, s)) == jpeg_roundtrip_host(x[None], q, s)[0], exactly.
    optimize=True (DESIGN.md "JPEG files out, optimised tables") codes the same coefficients with the frame's own four
    tables, jpeg_optimal_table of jpeg_symbol_counts, written in the places of the Annex K.3 ones: the header's length then
    varies with the frame, the scan is never longer, and the file decodes to the same pixels.
    layout (DESIGN.md "JPEG files out, 4:2:2 and greyscale"): one of JPEG_LAYOUTS in the place of subsampling, which then
    keeps its default.  '420' and '444' are the subsampling of that name.  '422' pads to MCUs of 16 x 8 pixels and takes
    chroma as the mean of horizontal pairs with libjpeg's alternating bias, (a + b + (chroma column & 1)) >> 1; 'grey' pads
    to 8 x 8 and keeps Y of the colour transform alone, coded with the first pair of tables: with optimize=False the bytes
    of jpeg_encode_layout_host.  The header holds all six tables in every layout, so an optimised 'grey' file has two empty
    tables of id 1, which no scan symbol refers to."""
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 3 or u8.shape[-1] != 3 or u8.numel() == 0:
        raise ValueError('jpeg_encode_host expects a non-empty uint8 (H, W, 3) frame')
    if not isinstance(optimize, bool):
        raise ValueError('jpeg_encode_host: optimize is True or False, got %r' % (optimize,))
    word = _jpeg_encode_layout(subsampling, layout, 'jpeg_encode_host')
    H, W = int(u8.shape[0]), int(u8.shape[1])
    if H > JPEG_MAX_SIDE or W > JPEG_MAX_SIDE:
        raise ValueError('jpeg_encode_host: frames of at most %d x %d' % (JPEG_MAX_SIDE, JPEG_MAX_SIDE))
    ri = jpeg_restart_interval(restart_interval, W, subsampling, layout)
    qt = jpeg_quant_tables(quality)
    fac = list(JPEG_LAYOUT_FACTORS[word])
    mh, mv = fac[0]
    if word in JPEG_SUBSAMPLINGS:
        planes = _jpeg_planes_in(u8[None].cpu(), mh)
    else:
        Y, Cb, Cr = _jpeg_colour_in(u8[None].cpu(), 8 * mv, 8 * mh)
        planes = [Y]
        if word == '422':
            bias = torch.tensor([0, 1], dtype=torch.int32).repeat(Y.shape[2] // 4)
            planes += [(c[:, :, 0::2] + c[:, :, 1::2] + bias) >> 1 for c in (Cb, Cr)]
    zz = torch.tensor(JPEG_ZIGZAG)
    coef = []                                               # per component (block rows, block columns, 64) in zigzag order
    for c, p in enumerate(planes):
        k = _jpeg_quantise(p, qt[min(c, 1)][None])[0].permute(0, 2, 1, 3)
        coef.append(k.reshape(k.shape[0], k.shape[1], 64)[:, :, zz].tolist())
    my, mx = -(-H // (8 * mv)), -(-W // (8 * mh))
    tables = jpeg_optimal_tables(coef, fac, my, mx, ri) if optimize else None
    return _jpeg_scan(bytearray(_jpeg_header(H, W, quality, fac, ri, tables)), coef, fac, my, mx, ri, tables)


def _jpeg_scan(out: bytearray, coef, fac, my: int, mx: int, ri: int, tables=None) -> bytes:
    """The scan writer of the host encoders: behind the header in `out`, my x mx MCUs of components sampled fac = [(h, v)],
    coef per component [block row][block column][64] in zigzag order; Huffman coding with `tables` ({(class, id): (counts,
    values)}, the Annex K.3 tables by default; the first pair for Y, the second for the rest), a restart marker and a
    prediction reset every ri MCUs (0: none), ones to the byte boundary in front of every marker, FF stuffed; EOI -> the file"""
    codes = {k: _huffman_codes(*v) for k, v in (JPEG_STD_HUFFMAN if tables is None else tables).items()}
    acc = nacc = 0

    def put(code, length):
        nonlocal acc, nacc
        acc, nacc = (acc << length) | code, nacc + length
        while nacc >= 8:
            b = (acc >> (nacc - 8)) & 255
            out.append(b)
            if b == 255:
                out.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1

    def magnitude(v):
        s = abs(v).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    pred = [0] * len(fac)
    for mcu in range(my * mx):
        if ri and mcu and mcu % ri == 0:
            if nacc:
                put((1 << (8 - nacc)) - 1, 8 - nacc)
            out += bytes([0xFF, 0xD0 + (mcu // ri - 1) % 8])
            pred = [0] * len(fac)
        y, x = divmod(mcu, mx)
        for c, (nh, nv) in enumerate(fac):
            dc, ac = codes[(0, min(c, 1))], codes[(1, min(c, 1))]
            for v in range(nv):
                for h in range(nh):
                    blk = coef[c][y * nv + v][x * nh + h]
                    size, bits = magnitude(blk[0] - pred[c])
                    pred[c] = blk[0]
                    put(*dc[size])
                    if size:
                        put(bits, size)
                    run = 0
                    last = max([k for k in range(1, 64) if blk[k]] or [0])
                    for k in range(1, last + 1):
                        if blk[k] == 0:
                            run += 1
                            continue
                        while run > 15:
                            put(*ac[0xF0])
                            run -= 16
                        size, bits = magnitude(blk[k])
                        put(*ac[(run << 4) | size])
                        put(bits, size)
                        run = 0
                    if last < 63:
                        put(*ac[0])
    if nacc:
        put((1 << (8 - nacc)) - 1, 8 - nacc)
    return bytes(out + b'\xff\xd9')


def jpeg_encode_layout_host(u8: Tensor, quality: int, layout: str, restart_interval: int = 0) -> bytes:
    """jpeg_encode_host for the layouts that have no device encoder, for tests and benchmarks: u8 uint8 (H, W, 3) -> a
    baseline file in layout '422' or 'grey'.  Colour in is the round trip's; the frame is padded to whole MCUs (16 x 8
    pixels at '422', 8 x 8 for 'grey') by edge replication; '422' chroma is the mean of horizontal pairs with libjpeg's
    alternating bias, (a + b + (column & 1)) >> 1 with `column` that of the chroma sample; 'grey' keeps Y alone.  Then
    _fdct8, quantisation with jpeg_quant_tables(quality) and the scan writer of jpeg_encode_host, with a restart marker every
    restart_interval MCUs (an int in 0..65535; 0: none)."""
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 3 or u8.shape[-1] != 3 or u8.numel() == 0:
        raise ValueError('jpeg_encode_layout_host expects a non-empty uint8 (H, W, 3) frame')
    if layout not in ('422', 'grey'):
        raise ValueError("jpeg_encode_layout_host: the layout is '422' or 'grey' (jpeg_encode_host writes the rest), got %r"
                         % (layout,))
    H, W = int(u8.shape[0]), int(u8.shape[1])
    if H > JPEG_MAX_SIDE or W > JPEG_MAX_SIDE:
        raise ValueError('jpeg_encode_layout_host: frames of at most %d x %d' % (JPEG_MAX_SIDE, JPEG_MAX_SIDE))
    ri = restart_interval
    if isinstance(ri, bool) or not isinstance(ri, int) or not 0 <= ri <= 65535:
        raise ValueError('jpeg_encode_layout_host: the restart interval is an int in [0, 65535] MCUs, got %r' % (restart_interval,))
    qt = jpeg_quant_tables(quality)
    fac = [(2, 1), (1, 1), (1, 1)] if layout == '422' else [(1, 1)]
    Y, Cb, Cr = _jpeg_colour_in(u8[None].cpu(), 8, 8 * fac[0][0])
    planes = [Y]
    if layout == '422':
        bias = torch.tensor([0, 1], dtype=torch.int32).repeat(Y.shape[2] // 4)
        planes += [(c[:, :, 0::2] + c[:, :, 1::2] + bias) >> 1 for c in (Cb, Cr)]
    zz = torch.tensor(JPEG_ZIGZAG)
    coef = []
    for c, p in enumerate(planes):
        k = _jpeg_quantise(p, qt[min(c, 1)][None])[0].permute(0, 2, 1, 3)
        coef.append(k.reshape(k.shape[0], k.shape[1], 64)[:, :, zz].tolist())
    my, mx = Y.shape[1] // 8, Y.shape[2] // (8 * fac[0][0])
    return _jpeg_scan(bytearray(_jpeg_header(H, W, quality, fac, ri)), coef, fac, my, mx, ri)


def check_encode_qualities(quality, n: int) -> Tensor:
    """check_qualities for an encoder: every entry compresses, so it lies in 1..100"""
    q = check_qualities(quality, n)
    if bool((q < 1).any()):
        raise ValueError('quality: an encoder takes entries in [1, 100], got down to %d' % int(q.min()))
    return q


def jpeg_encode_files_host(frames: Tensor, quality, subsampling: str = '420', restart_interval='row', optimize: bool = False,
                           layout=None) -> list:
    """The definition of ops.jpeg_encode_u8 for a batch: frames uint8 (n, H, W, 3) or (B, T, H, W, 3), quality an int or
    int32 (n,) / (B,) as check_qualities takes it, every entry in 1..100 -> [jpeg_encode_host(frame, its quality, ...)];
    optimize=True: every file with its own Huffman tables; layout: one of JPEG_LAYOUTS in the place of subsampling."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() not in (4, 5) or frames.shape[-1] != 3 \
            or frames.numel() == 0:
        raise ValueError('jpeg_encode_files_host expects non-empty uint8 (n, H, W, 3) or (B, T, H, W, 3) frames')
    q = check_encode_qualities(quality, frames.shape[0])
    if frames.dim() == 5:
        q = q.repeat_interleave(frames.shape[1])
    flat = frames.reshape((-1,) + tuple(frames.shape[-3:])).cpu()
    return [jpeg_encode_host(f, int(v), subsampling, restart_interval, optimize, layout) for f, v in zip(flat, q.tolist())]


JPEG_ENCODE_STATUS = {1: 'the file does not fit in data: offsets[n] is the capacity a retry needs', 2: 'quality <= 0: no file',
                      3: 'a coefficient outside the categories of baseline JPEG, coded clamped'}


class _EncodedFiles:
    """data, offsets, status of an encoder call on the device and the way back to the host, shared by JpegFiles and PngFiles;
    a subclass names itself, its status words and the statuses whose file is empty"""
    geometry = None
    _name, _who, _status, _empty = '', '', {}, ()

    def __init__(self, data: Tensor, offsets: Tensor, status: Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 \
                or status.dtype != torch.int32 or tuple(status.shape) != (offsets.shape[0] - 1,) or status.shape[0] < 1:
            raise ValueError('%s: data uint8 (capacity,), offsets int64 (n + 1,), status int32 (n,) expected' % self._name)
        self.data, self.offsets, self.status = data, offsets, status

    def __len__(self) -> int:
        return int(self.status.shape[0])

    def nbytes(self) -> int:
        """the bytes of all files, offsets[n] (this waits for the device); more than the capacity where a status is 1"""
        return int(self.offsets[-1])

    def files(self, check: bool = True) -> list:
        """-> [bytes] of every file.  Waits for the device once, for offsets and status, then copies offsets[n] bytes back
        (at most the capacity).  check: a non-zero status raises ValueError with its name; with check=False such a file is
        handed over as it is: b'' for a status that writes no file."""
        table = torch.cat([self.offsets, self.status.to(torch.int64)]).cpu().tolist()
        n = len(self)
        offsets, status = table[:n + 1], table[n + 1:]
        if check:
            for i, s in enumerate(status):
                if s != 0:
                    raise ValueError('%s: file %d has status %d (%s)' % (self._who, i, s, self._status.get(s, 'unknown')))
        host = self.data[:max(0, min(offsets[n], int(self.data.shape[0])))].cpu().numpy().tobytes()
        return [b'' if s in self._empty else host[offsets[i]:offsets[i + 1]] for i, s in enumerate(status)]


class JpegFiles(_EncodedFiles):
    """What ops.jpeg_encode_u8 hands back, on the device: data uint8 (capacity,): the files end to end | offsets int64
    (n + 1,): file i is data[offsets[i]:offsets[i + 1]] | status int32 (n,): 0 fine, the rest as JPEG_ENCODE_STATUS names
    them.  Nothing here has waited for the device until files() or nbytes() is called (b'' for status 1 and 2).  geometry:
    what the files of one encoder call share (H, W, layout, restart_interval in MCUs, optimize), left here by
    ops.jpeg_encode_u8 for JpegBank.from_encoded; None for a JpegFiles put together by hand."""
    _name, _who, _status, _empty = 'JpegFiles', 'jpeg_encode', JPEG_ENCODE_STATUS, (1, 2)


class JpegBatch:
    """Files packed for one launch of ops.jpeg_decode_u8 (jpeg_batch makes it): host tensors, pinned where a device is there
    to take them.  data uint8: the scan bytes of every file, end to end | images int32 (n, 20): H, W, chroma step, MCU
    columns, MCU rows, the quantisation slots of Y, Cb, Cr, the (DC, AC) Huffman slots of Y, Cb, Cr, first block in the
    scratch, first workgroup of the IDCT, first segment, segments, blocks, layout code (JPEG_LAYOUT_CODES) | segments int32
    (s, 5): image, first byte, end byte, first MCU, MCUs | qtabs int32 (q, 64): the distinct quantisation tables, natural
    order | htabs int32 (h, 288): the distinct Huffman tables as jpeg_huffman_table makes them | sizes: [(H, W)] | blocks:
    8 x 8 blocks of the whole batch."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._on = {}

    @property
    def scratch_bytes(self) -> int:
        """what a launch needs: int16 coefficients and uint8 planes of every block, an int32 status per segment"""
        return 192 * self.blocks + 4 * int(self.segments.shape[0])

    def on(self, device):
        """the five tensors on `device`: .data .images .segments .qtabs .htabs.  Uploaded once, without blocking, on the
        stream that is current at the first call: a caller that decodes on another stream later orders the two itself."""
        key = str(device)
        if key not in self._on:
            names = ('data', 'images', 'segments', 'qtabs', 'htabs')
            self._on[key] = SimpleNamespace(**{k: getattr(self, k).to(device, non_blocking=True) for k in names})
        return self._on[key]


def jpeg_batch(files, layouts=JPEG_LAYOUTS_DEFAULT) -> JpegBatch:
    """A sequence of baseline JPEG files (bytes) -> the JpegBatch of one launch.  Every file goes through jpeg_parse with
    `layouts`, so a file the decoder does not take is refused here, before anything is uploaded.  A JpegFiles (the encoder's
    result) is read back through its files().  A row of a 'grey' image repeats Y's table slots for Cb and Cr."""
    layouts = _jpeg_layouts(layouts, 'jpeg_batch')
    files = files.files() if isinstance(files, JpegFiles) else list(files)
    if not files:
        raise ValueError('jpeg_batch: an empty batch')
    chunks, images, segments, qtabs, htabs, sizes = [], [], [], {}, {}, []
    nbytes = blocks = groups = 0
    for i, f in enumerate(files):
        hd = f if isinstance(f, JpegHeader) else jpeg_parse(f, layouts)
        my, mx = hd.mcus
        q = [qtabs.setdefault(t, len(qtabs)) for t in hd.quant]
        h = [htabs.setdefault(t, len(htabs)) for pair in hd.huffman for t in pair]
        q, h = q + q[:1] * (3 - len(q)), h + h[:2] * (3 - len(hd.huffman))
        nb = my * mx * len(hd.mcu_blocks)
        images.append([hd.H, hd.W, hd.sub, mx, my] + q + h + [blocks, groups, len(segments), len(hd.segments), nb,
                                                              JPEG_LAYOUT_CODES[hd.layout]])
        blocks, groups = blocks + nb, groups + -(-nb // JPEG_IDCT_BLOCKS)
        lo, hi = hd.segments[0][0], hd.segments[-1][1]
        ri = hd.restart_interval or my * mx
        for k, (b, e) in enumerate(hd.segments):
            segments.append([i, nbytes + b - lo, nbytes + e - lo, k * ri, min(ri, my * mx - k * ri)])
        chunks.append(hd.data[lo:hi])
        nbytes += hi - lo
        sizes.append((hd.H, hd.W))
    pin = torch.cuda.is_available()

    def host(t):
        return t.pin_memory() if pin and t.numel() else t
    data = torch.frombuffer(bytearray(b''.join(chunks) or b'\0'), dtype=torch.uint8)
    return JpegBatch(data=host(data), nbytes=nbytes, images=host(torch.tensor(images, dtype=torch.int32)),
                     segments=host(torch.tensor(segments, dtype=torch.int32)),
                     qtabs=host(torch.tensor(list(qtabs), dtype=torch.int32)),
                     htabs=host(torch.tensor([jpeg_huffman_table(*t) for t in htabs], dtype=torch.int32)),
                     sizes=sizes, n=len(files), blocks=blocks, groups=groups)


# DESIGN.md "JPEG files without restart markers": a restart interval decoded from several start points at once.
# jpeg_split_plan is the chunk rule, jpeg_split_host the definition of the state table (csrc/jpeg_entropy_split.h has the
# same steps for the device); the definition of the pixels stays jpeg_decode_host.
JPEG_SPLIT_LANES = 256                      # chunks of a segment at the most: the lanes of its workgroup
JPEG_SPLIT_MIN = 16                         # the smallest chunk_bytes
JPEG_SPLIT_DEFAULT = 128                    # what split='auto' takes (DESIGN.md has the sweep it comes from)
JPEG_SPLIT_AUTO_BYTES = 12 * 128            # ... where some segment is longer than this: measured to lose at 850, to win at 1700
JPEG_STATE_INTS = 8                         # a state row: ISTVT_JPEG_STATE_INTS of include/istvt_hip.h


def check_split(chunk_bytes) -> int:
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, int) or chunk_bytes < JPEG_SPLIT_MIN:
        raise ValueError('jpeg split: the chunk size is an int of at least %d bytes, got %r' % (JPEG_SPLIT_MIN, chunk_bytes))
    return chunk_bytes


def jpeg_split_chunks(length: int, chunk_bytes: int):
    """the chunk rule for one segment of `length` bytes -> (chunk size, number of chunks): js_chunk_bytes and js_chunks of
    csrc/jpeg_entropy_split.h"""
    c = max(chunk_bytes, -(-length // JPEG_SPLIT_LANES))
    return c, max(1, -(-length // c))


def jpeg_split_plan(batch_or_header, chunk_bytes: int) -> SimpleNamespace:
    """How ops.jpeg_decode_u8(..., split=chunk_bytes) cuts the segments of a JpegBatch (or of one parsed file, packed alone):
    a segment of `length` bytes into chunks of max(chunk_bytes, ceil(length / 256)) bytes, at least one and at most 256 of
    them; the last ends with the segment.  -> chunk, count, row0: per segment, the chunk size, the number of chunks and the
    first of its rows in the state table (first byte // chunk_bytes + segment: segments lie in order, so rows never meet) |
    rows: rows of the table | states_at: where the table starts in the scratch | scratch_bytes: what the launch needs."""
    chunk_bytes = check_split(chunk_bytes)
    batch = batch_or_header if isinstance(batch_or_header, JpegBatch) else jpeg_batch([batch_or_header])
    chunk, count, row0 = [], [], []
    for s, (_, b, e, _, _) in enumerate(batch.segments.tolist()):
        c, k = jpeg_split_chunks(e - b, chunk_bytes)
        chunk.append(c)
        count.append(k)
        row0.append(b // chunk_bytes + s)
    rows = batch.nbytes // chunk_bytes + len(chunk)
    at = -(-batch.scratch_bytes // 16) * 16
    return SimpleNamespace(chunk=chunk, count=count, row0=row0, rows=rows, states_at=at,
                           scratch_bytes=at + 4 * JPEG_STATE_INTS * rows)


class _JpegPosBits:
    """_JpegBits for the split path: a reader that knows where it is and can be opened at any (pos, bit).  pos: the raw
    index of the byte that holds the next bit (never a stuffed 00; the zeros fed past `end` count on as bytes end, end + 1,
    ...), bit: bits of it already taken.  Three bytes wait in win; p[0..2] are their indices, p[3] the next to fetch."""

    def __init__(self, data, end, pos, bit):
        self.data, self.end, self.bit, self.status = data, end, bit, 0
        self.p, self.win = [pos], 0
        for _ in range(3):
            b, at = self._fetch(self.p[-1])
            self.win = (self.win << 8) | b
            self.p.append(at)

    def _fetch(self, at):
        if at >= self.end:
            return 0, at + 1
        b = self.data[at]
        at += 1
        if b == 0xFF and at < self.end and self.data[at] == 0:
            at += 1
        return b, at

    @property
    def pos(self):
        return self.p[0]

    def skip(self, k):
        last = self.p[0]
        self.bit += k
        while self.bit >= 8:
            last = self.p[0]
            b, at = self._fetch(self.p[3])
            self.win = ((self.win << 8) | b) & 0xFFFFFF
            self.p = self.p[1:] + [at]
            self.bit -= 8
        if self.bit > 0:
            last = self.p[0]
        if last >= self.end:
            self.status = 1

    def huffman(self, t):
        c = (self.win >> (8 - self.bit)) & 0xFFFF
        for l in range(1, 17):
            if c < t[l - 1]:
                self.skip(l)
                return t[32 + ((t[16 + l - 1] + (c >> (16 - l))) & 255)]
        return -1

    def receive(self, s):
        r = (self.win >> (24 - self.bit - s)) & ((1 << s) - 1)
        self.skip(s)
        return r if r >= (1 << (s - 1)) else r - (1 << s) + 1


def _split_chunk(data, end, limit, tabs, seq, state):
    """The lenient transition of one lane (js_chunk): the symbols from `state` that start before `limit` -> (the exit state,
    blocks started up to the first error, that error or 0).  A prefix no code matches takes 16 bits and counts as 0, a DC
    category above 11 counts as 0, a run past 63 ends the block: it cannot die, and up to the first of these it is the
    decoder of _jpeg_block.  seq: the component of every block of an MCU (JpegHeader.mcu_blocks)."""
    pos, bit, blk, k = state
    bits = _JpegPosBits(data, end, pos, bit)
    nblk, blocks, err = len(seq), 0, 0
    while bits.pos < limit:
        c = seq[blk]
        done = False
        if k == 0:
            s = bits.huffman(tabs[c][0])
            blocks += 0 if err else 1
            if s < 0:
                bits.skip(16)
            if s < 0 or s > 11:
                err = err or 2
            else:
                bits.skip(s)
            k = 1
        else:
            rs = bits.huffman(tabs[c][1])
            if rs < 0:
                bits.skip(16)
                err, rs = err or 2, 0
            r, s = rs >> 4, rs & 15
            if s == 0:
                k = k + 16 if r == 15 else 64
                if k > 64:
                    err = err or 3
                done = k >= 64
            else:
                k += r
                if k > 63:
                    err, done = err or 3, True
                else:
                    bits.skip(s)
                    k += 1
                    done = k == 64
        if done:
            k, blk = 0, (blk + 1) % nblk
    return (bits.pos, bits.bit, blk, k), blocks, err


def _split_strict(data, end, limit, last, tabs, seq, total, state, nxt):
    """The strict decode of one lane (js_write without its stores): _jpeg_block's steps from a converged state on the symbols
    that start before `limit`, or with last=True until block `total` of the segment would start; nxt: the number of the next
    block to start -> (status, blocks started)"""
    pos, bit, _, k = state
    bits = _JpegPosBits(data, end, pos, bit)
    started, c = 0, 0
    if k > 0:
        if not 1 <= nxt <= total:
            return 0, 0
        c = seq[(nxt - 1) % len(seq)]
    while last or bits.pos < limit:
        if k == 0:
            if nxt >= total:
                break
            c = seq[nxt % len(seq)]
            nxt, started = nxt + 1, started + 1
            s = bits.huffman(tabs[c][0])
            if s < 0 or s > 11:
                return 2, started
            if s:
                bits.receive(s)
            k = 1
            continue
        rs = bits.huffman(tabs[c][1])
        if rs < 0:
            return 2, started
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                k = 0
                continue
            k += 16
            if k > 64:
                return 3, started
            k %= 64
            continue
        k += r
        if k > 63:
            return 3, started
        bits.receive(s)
        k = (k + 1) % 64
    return bits.status, started


def jpeg_split_host(header, chunk_bytes: int) -> SimpleNamespace:
    """The host model of the split entropy decode of one parsed file (a JpegHeader, or bytes): per segment, S chunks by
    jpeg_split_plan's rule and as many lanes.

      guess    lane 0 starts at (begin, 0, 0, 0); lane i at byte begin + i * chunk, bit 0, block 0, k 0, one byte later
               where that byte is the 00 stuffed behind an FF
      relax    in every round lane i recomputes its exit state from the exit state lane i - 1 had the round before
               (_split_chunk); the loop ends when no state changed.  After round r lanes 0..r hold the sequential
               decoder's states, so there are at most S - 1 rounds and the guesses cannot change the result.
      strict   every lane decodes its chunk once by the rules of _jpeg_block (_split_strict), up to the first lane that
               meets an error; the segment stops at its MCU count, and only its last lane reads past the end.

    -> segments: per segment a namespace of states [(pos, bit, blk, k)], the entry state of every lane, pos an index into
    the file; blocks: blocks started per lane; first: each lane's first block; lane_status; rounds: the rounds in which a
    state changed; status; rows: the eight ints per lane the device leaves in the scratch | status: the largest of the
    segments', jpeg_decode_host's | rounds: the largest.  The fixed point is asserted against one walk from lane 0 on."""
    hd = header if isinstance(header, JpegHeader) else jpeg_parse(header)
    chunk_bytes = check_split(chunk_bytes)
    seq, (my, mx) = hd.mcu_blocks, hd.mcus
    nblk = len(seq)
    tabs = [(jpeg_huffman_table(*dc), jpeg_huffman_table(*ac)) for dc, ac in hd.huffman]
    ri = hd.restart_interval or my * mx
    data, segments = hd.data, []
    for i, (begin, end) in enumerate(hd.segments):
        total = nblk * min(ri, my * mx - i * ri)
        chunk = max(chunk_bytes, -(-(end - begin) // JPEG_SPLIT_LANES))
        S = max(1, -(-(end - begin) // chunk))
        limits = [begin + (j + 1) * chunk for j in range(S)]
        entry = [(begin, 0, 0, 0)]
        for j in range(1, S):
            at = begin + j * chunk
            entry.append((at + 1 if data[at - 1] == 0xFF and data[at] == 0 else at, 0, 0, 0))
        step = [_split_chunk(data, end, limits[j], tabs, seq, entry[j]) for j in range(S - 1)]
        rounds = 0
        for _ in range(1, S):
            changed = False
            before = [st[0] for st in step]
            for j in range(1, S):
                if before[j - 1] != entry[j]:
                    entry[j] = before[j - 1]
                    if j < S - 1:
                        new = _split_chunk(data, end, limits[j], tabs, seq, entry[j])
                        changed = changed or new[0] != step[j][0]
                        step[j] = new
            if not changed:
                break
            rounds += 1
        walk = [(begin, 0, 0, 0)]
        for j in range(S - 1):
            walk.append(_split_chunk(data, end, limits[j], tabs, seq, walk[j])[0])
        assert entry == walk and rounds <= max(S - 1, 0), 'jpeg_split_host: the relaxation did not reach the sequential states'
        # a lane's first block: the tallies of the lanes in front; the lanes up to the first whose tally met an error decode
        dead = min([j for j in range(S - 1) if step[j][2]], default=S)
        blocks, first, lane_status, nxt = [], [], [], 0
        for j in range(S):
            first.append(min(nxt, total))                         # bits behind the last block can look like blocks
            st, started = _split_strict(data, end, limits[j], j == S - 1, tabs, seq, total, entry[j], nxt) if j <= dead else (0, 0)
            nxt += step[j][1] if j < S - 1 else 0
            blocks.append(started)
            lane_status.append(st)
        status = max(lane_status)
        rows = [list(entry[j]) + [blocks[j], first[j], lane_status[j], rounds] for j in range(S)]
        segments.append(SimpleNamespace(states=entry, blocks=blocks, first=first, lane_status=lane_status, rounds=rounds,
                                        status=status, chunk=chunk, rows=rows))
    return SimpleNamespace(segments=segments, status=max(s.status for s in segments), rounds=max(s.rounds for s in segments))


def whole_boxes(sizes) -> Tensor:
    """[(H, W)] -> int32 (n, 4): the box (0, 0, H, W) of every frame, for crop_resize_u8 on the decoder's canvas"""
    return torch.tensor([[0, 0, int(h), int(w)] for h, w in sizes], dtype=torch.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------ JPEG bank
# DESIGN.md "JPEG bank": the files of a whole set parsed once and kept on the device, then decoded in any order and any
# number of times through an index that lives on the device too (ops.jpeg_decode_indexed_u8).  jpeg_bank packs host files,
# JpegBank.from_encoded takes the encoder's result without leaving the device, jpeg_bank_decode_host is the definition of the
# indexed decode and jpeg_scan_segments_host that of the device's marker scan.
JPEG_BANK_MAX_BYTES = 2 ** 31 - 1           # segment rows are int32 byte offsets
JPEG_BANK_STATUS = {4: 'the index is outside the bank', 5: 'the bank holds no decodable file at that place'}
JPEG_SCAN_LANE_BYTES = 16                   # JB_LANE_BYTES of csrc/jpeg_bank_scan.h: the bytes of a lane of the marker scan
JPEG_SCAN_TILE_BYTES = 256 * 16             # ... and of a workgroup's trip


def _bank_bytes(nbytes: int, who: str) -> int:
    if nbytes > JPEG_BANK_MAX_BYTES:
        raise ValueError('%s: %d bytes; a bank holds fewer than 2^31 (its segment rows are int32 byte offsets): use several banks'
                         % (who, nbytes))
    return nbytes


def _bank_split(split, who: str):
    """the `split` argument of a bank, checked: None, 'auto' or a chunk size that check_split accepts"""
    if split is None or (isinstance(split, str) and split == 'auto'):
        return split
    if isinstance(split, bool) or not isinstance(split, int) or split < JPEG_SPLIT_MIN:
        raise ValueError("%s: split is None, 'auto' or a chunk size in bytes (an int of at least %d), got %r"
                         % (who, JPEG_SPLIT_MIN, split))
    return split


class JpegBank:
    """A set of files ready for ops.jpeg_decode_indexed_u8: what a JpegBatch of the whole set holds -- data, images (n, 20),
    segments, qtabs, htabs, sizes, as JpegBatch describes them -- and the two numbers that make a call's geometry independent
    of which files it draws: seg_max, the most segments of any file, and block_stride, the most 8 x 8 blocks of any, rounded
    up to a multiple of JPEG_IDCT_BLOCKS.  Hmax, Wmax: the largest height and width.  An images row with 0 segments is an
    empty place (the device ingest marks files so): drawing it gives status 5.

    jpeg_bank builds one from host files: the tensors are host tensors (pinned where a device is there to take them),
    `headers` keeps the parsed files for jpeg_bank_decode_host, and on(device) uploads once.  from_encoded and extend build
    one on a device: data .. htabs are None, `device` says where it lives, and on(device) hands those tensors back.

    How the bank's restart intervals are decoded is a property of the bank (DESIGN.md "JPEG bank, split"), not of a call,
    because it fixes a call's scratch layout and workgroup size.  split: None, one lane per interval, or the chunk size in
    bytes of the split entropy kernel, one lane per chunk (ops.jpeg_decode_u8 describes both; files without restart markers
    want the second).  seg_bytes_max: the longest interval of the set in bytes, or None where the host has not seen the
    lengths (an ingested bank whose caller named none).  chunk_rows: the state rows a split bank reserves per segment."""

    def __init__(self, **kw):
        self.device = self.headers = self.split = self.seg_bytes_max = None
        self.__dict__.update(kw)
        self._on = {}

    def __len__(self) -> int:
        return self.n

    @property
    def chunk_rows(self):
        """min(256, max(1, ceil(seg_bytes_max / split))): an upper bound of jpeg_split_plan's chunk count for every length up
        to seg_bytes_max (ceil(L / max(split, ceil(L / 256))) <= ceil(L / split), which grows with L, and <= 256) -- not
        the count at seg_bytes_max itself, which is not monotone once the 256-lane cap raises the chunk size.  256 where
        seg_bytes_max is not known: no interval has more chunks.  None for a bank without a split."""
        if self.split is None:
            return None
        if self.seg_bytes_max is None:
            return JPEG_SPLIT_LANES
        return min(JPEG_SPLIT_LANES, max(1, -(-self.seg_bytes_max // self.split)))

    def _resolve_split(self, split, who: str):
        """the `split` argument of jpeg_bank / with_split -> None or a chunk size: JPEG_SPLIT_DEFAULT for 'auto' where the
        longest interval exceeds JPEG_SPLIT_AUTO_BYTES (ops.jpeg_decode_u8's rule, decided once per bank)"""
        if _bank_split(split, who) != 'auto':
            return split
        if self.seg_bytes_max is None:
            raise ValueError("%s: split='auto' needs the longest interval of the bank, which the host has not seen for an "
                             "ingested bank: name seg_bytes_max= in JpegBank.from_encoded, or a chunk size" % who)
        return JPEG_SPLIT_DEFAULT if self.seg_bytes_max > JPEG_SPLIT_AUTO_BYTES else None

    def with_split(self, split) -> 'JpegBank':
        """A second JpegBank over the same files with another `split` (None, 'auto' or a chunk size): the same tensors and
        the same uploaded copies, nothing copied or uploaded again.  with_split(None) is the bank of one lane per interval.
        The two share what on() has uploaded; extend() and release_host() act on the bank they are called on alone."""
        other = JpegBank.__new__(JpegBank)
        other.__dict__.update(self.__dict__)                     # _on included: one cache
        other.split = self._resolve_split(split, 'JpegBank.with_split')
        return other

    def on(self, device):
        """the five tensors on `device`: .data .images .segments .qtabs .htabs, uploaded once without blocking (JpegBatch.on)"""
        key = str(torch.device(device))
        if key not in self._on:
            if self.data is None:
                raise RuntimeError('JpegBank: this bank was built on %s and has no host copy to upload to %s' % (self.device, key))
            names = ('data', 'images', 'segments', 'qtabs', 'htabs')
            self._on[key] = SimpleNamespace(**{k: getattr(self, k).to(device, non_blocking=True) for k in names})
        return self._on[key]

    def release_host(self) -> None:
        """drops the host copies (the bytes, the tables, the parsed files) of a bank that has been uploaded: the device
        copies are what a decode reads"""
        if not self._on:
            raise RuntimeError('JpegBank.release_host: upload the bank first (on(device))')
        self.device = self.device or next(iter(self._on))
        self.data = self.images = self.segments = self.qtabs = self.htabs = self.headers = None

    @classmethod
    def from_encoded(cls, jf, H=None, W=None, layout=None, restart_interval=None, seg_bytes_max=None) -> 'JpegBank':
        """The result of ops.jpeg_encode_u8 / ops.encode_frames (a JpegFiles) -> a bank over the same bytes, on their device:
        no files(), no readback, no synchronisation (frames.jpeg_bank_ingest has the launches).  The geometry all files of
        the call share comes from jf.geometry, which the encoder call leaves there; H, W, layout (one of JPEG_LAYOUTS) and
        restart_interval name it for a JpegFiles put together by hand.  Files with optimised tables are refused.
        seg_bytes_max: the longest restart interval in bytes, where the caller knows a bound -- the host does not read the
        lengths here.  A split decode then reserves chunk_rows for it instead of 256 per segment, and a file with a longer
        interval decodes to status 5; without it split='auto' is refused."""
        from . import frames
        return frames.jpeg_bank_ingest(jf, H, W, layout, restart_interval, seg_bytes_max)

    def extend(self, other: 'JpegBank', device=None) -> 'JpegBank':
        """Appends the files of `other` (another encode call's bank, say) behind this bank's, on the device both live on (or
        `device` for two host banks): the bytes are joined, and offsets, table slots and first segments of `other` are
        rebased with tensor expressions there.  Nothing is read back.  Afterwards this bank lives on that device alone.
        seg_bytes_max becomes the larger of the two, or None where either is; split stays this bank's."""
        if not isinstance(other, JpegBank):
            raise TypeError('JpegBank.extend takes a JpegBank, got %s' % type(other).__name__)
        device = device or self.device or other.device
        if device is None:
            raise ValueError('JpegBank.extend: two host banks are joined on the `device` the call names')
        for b in (self, other):
            if b.device is not None and str(torch.device(b.device)) != str(torch.device(device)):
                raise RuntimeError('JpegBank.extend: the banks live on %s and %s' % (b.device, device))
        _bank_bytes(self.nbytes + other.nbytes, 'JpegBank.extend')
        a, b = self.on(device), other.on(device)
        I = JPEG_IMAGE_INTS
        add = torch.zeros(I, dtype=torch.int32)
        add[5:8], add[8:14], add[14], add[15], add[16] = self.nq, self.nh, self.blocks, self.groups, self.nseg
        seg_add = torch.tensor([self.n, self.nbytes, self.nbytes, 0, 0], dtype=torch.int32)
        joined = SimpleNamespace(
            data=torch.cat([a.data[:self.nbytes], b.data[:other.nbytes]]),
            images=torch.cat([a.images, b.images + add.to(device)]),
            segments=torch.cat([a.segments, b.segments + seg_add.to(device)]),
            qtabs=torch.cat([a.qtabs, b.qtabs]), htabs=torch.cat([a.htabs, b.htabs]))
        self.n, self.nbytes, self.nseg = self.n + other.n, self.nbytes + other.nbytes, self.nseg + other.nseg
        self.nq, self.nh = self.nq + other.nq, self.nh + other.nh
        self.blocks, self.groups = self.blocks + other.blocks, self.groups + other.groups
        self.sizes = list(self.sizes) + list(other.sizes)
        self.seg_max, self.block_stride = max(self.seg_max, other.seg_max), max(self.block_stride, other.block_stride)
        self.Hmax, self.Wmax = max(self.Hmax, other.Hmax), max(self.Wmax, other.Wmax)
        known = self.seg_bytes_max is not None and other.seg_bytes_max is not None
        self.seg_bytes_max = max(self.seg_bytes_max, other.seg_bytes_max) if known else None
        self.data = self.images = self.segments = self.qtabs = self.htabs = self.headers = None
        self.device, self._on = torch.device(device), {str(torch.device(device)): joined}
        return self


def jpeg_bank(files, layouts=JPEG_LAYOUTS_DEFAULT, split=None) -> JpegBank:
    """A sequence of baseline JPEG files (bytes, or parsed JpegHeaders) -> the JpegBank of the set, on the host.  Every file
    goes through jpeg_parse with `layouts`, which refuses what the decoder does not take, and jpeg_batch packs the tables:
    the rows are those of jpeg_batch(files).  A set of 2^31 scan bytes or more is refused.  split: how the bank's restart
    intervals are decoded (JpegBank): None, by one lane each; a chunk size in bytes, by one lane per chunk, for files
    without restart markers; 'auto', JPEG_SPLIT_DEFAULT where the longest interval of the set (bank.seg_bytes_max) exceeds
    JPEG_SPLIT_AUTO_BYTES, else None."""
    layouts = _jpeg_layouts(layouts, 'jpeg_bank')
    _bank_split(split, 'jpeg_bank')                               # said before anything is parsed
    if isinstance(files, (bytes, bytearray, JpegFiles)) or not hasattr(files, '__len__'):
        raise TypeError('jpeg_bank expects a sequence of files (bytes); JpegBank.from_encoded takes a JpegFiles, got %s'
                        % type(files).__name__)
    if len(files) == 0:
        raise ValueError('jpeg_bank: an empty bank')
    headers = [f if isinstance(f, JpegHeader) else jpeg_parse(f, layouts) for f in files]
    _bank_bytes(sum(hd.segments[-1][1] - hd.segments[0][0] for hd in headers), 'jpeg_bank')
    batch = jpeg_batch(headers, layouts)
    bank = JpegBank(data=batch.data, nbytes=batch.nbytes, images=batch.images, segments=batch.segments, qtabs=batch.qtabs,
                    htabs=batch.htabs, sizes=batch.sizes, n=batch.n, nseg=int(batch.segments.shape[0]),
                    nq=int(batch.qtabs.shape[0]), nh=int(batch.htabs.shape[0]), blocks=batch.blocks, groups=batch.groups,
                    seg_max=int(batch.images[:, 17].max()),
                    block_stride=-(-int(batch.images[:, 18].max()) // JPEG_IDCT_BLOCKS) * JPEG_IDCT_BLOCKS,
                    Hmax=max(h for h, _ in batch.sizes), Wmax=max(w for _, w in batch.sizes), headers=headers,
                    seg_bytes_max=int((batch.segments[:, 2] - batch.segments[:, 1]).max()))
    bank.split = bank._resolve_split(split, 'jpeg_bank')
    return bank


def jpeg_bank_scratch_bytes(bank: JpegBank, m: int) -> int:
    """The scratch of ops.jpeg_decode_indexed_u8 for m places: coefficients and planes of m * block_stride blocks | an int32
    status per segment row and one more per place | from the next multiple of 16 bytes, the planned images (m, 20) and
    segments (m * seg_max, 5).  For a bank with a split, from the next multiple of 16 bytes behind those the state rows of the
    split kernel, int32 (m * seg_max * chunk_rows, 8): planned segment row s owns rows [s * chunk_rows, (s + 1) * chunk_rows)."""
    m = int(m)
    front = 192 * m * bank.block_stride + 4 * (m * bank.seg_max + m)
    need = -(-front // 16) * 16 + 4 * JPEG_IMAGE_INTS * m + 20 * m * bank.seg_max
    if bank.split is None:
        return need
    return -(-need // 16) * 16 + 4 * JPEG_STATE_INTS * m * bank.seg_max * bank.chunk_rows


def check_bank_index(index, who: str = 'jpeg_bank_decode_host') -> Tensor:
    """the `index` argument of an indexed decode: a list of ints, or a contiguous int32 / int64 tensor of one dimension, not
    empty; values are not looked at (a value outside the bank is status 4, not an error)"""
    if not torch.is_tensor(index):
        if isinstance(index, (str, bytes)) or not hasattr(index, '__len__') or \
                any(isinstance(v, bool) or not isinstance(v, int) for v in index):
            raise TypeError('%s: index is a list of ints or an int32 / int64 tensor, got %s' % (who, type(index).__name__))
        index = torch.tensor(list(index), dtype=torch.int64)
    if index.dtype not in (torch.int32, torch.int64) or index.dim() != 1:
        raise TypeError('%s: index is int32 or int64 of one dimension, got %s %s' % (who, index.dtype, tuple(index.shape)))
    if index.numel() == 0:
        raise ValueError('%s: an empty index' % who)
    if not index.is_contiguous():
        raise ValueError('%s: index must be contiguous, got stride %d' % (who, index.stride(0)))
    return index


def jpeg_bank_decode_host(bank_or_files, index, canvas=None, layouts=JPEG_LAYOUTS_DEFAULT):
    """The definition of ops.jpeg_decode_indexed_u8: -> (frames, sizes, status), frames uint8 (m, Hc, Wc, 3) with place j
    holding jpeg_decode_host(files[index[j]]) in its top left corner and 0 elsewhere, sizes int32 (m, 2) = (H, W), status
    int32 (m,).  bank_or_files: a JpegBank that jpeg_bank built, or a sequence of files (parsed with `layouts`) in which b''
    or None stands for an empty place.  Beside the statuses of jpeg_decode_host: 4 where index[j] is outside [0, n), 5 for an
    empty place; both with size (0, 0) and a frame of zeros.  canvas = (Hc, Wc) defaults to the largest H and W of the set."""
    if isinstance(bank_or_files, JpegBank):
        if bank_or_files.headers is None:
            raise ValueError('jpeg_bank_decode_host: this bank has no host copy of its files: pass the files')
        files = bank_or_files.headers
    else:
        files = list(bank_or_files)
    index = check_bank_index(index).tolist()
    drawn = {}
    for i in set(index):
        if 0 <= i < len(files) and files[i] is not None and not (isinstance(files[i], (bytes, bytearray)) and len(files[i]) == 0):
            drawn[i] = jpeg_decode_host(files[i], return_status=True, layouts=layouts)
    if isinstance(bank_or_files, JpegBank):
        Hmax, Wmax = bank_or_files.Hmax, bank_or_files.Wmax
    else:
        Hmax, Wmax = max([1] + [f.shape[0] for f, _ in drawn.values()]), max([1] + [f.shape[1] for f, _ in drawn.values()])
    Hc, Wc = (Hmax, Wmax) if canvas is None else (int(canvas[0]), int(canvas[1]))
    if any(f.shape[0] > Hc or f.shape[1] > Wc for f, _ in drawn.values()):
        raise ValueError('jpeg_bank_decode_host: the canvas %d x %d does not hold every image drawn' % (Hc, Wc))
    frames = torch.zeros((len(index), Hc, Wc, 3), dtype=torch.uint8)
    sizes = torch.zeros((len(index), 2), dtype=torch.int32)
    status = torch.zeros((len(index),), dtype=torch.int32)
    for j, i in enumerate(index):
        if i in drawn:
            f, s = drawn[i]
            frames[j, :f.shape[0], :f.shape[1]] = f.to(torch.uint8)
            sizes[j, 0], sizes[j, 1], status[j] = f.shape[0], f.shape[1], s
        else:
            status[j] = 5 if 0 <= i < len(files) else 4
    return frames, sizes, status


def check_jpeg_bank_status(status) -> None:
    """check_jpeg_status for an indexed decode: reads the status table back (this waits for the device) and raises for the
    first place that is not fine, statuses 4 and 5 (JPEG_BANK_STATUS) included"""
    names = {1: 'its scan ends early', 2: 'a Huffman code or DC category no table holds', 3: 'a run past coefficient 63'}
    names.update(JPEG_BANK_STATUS)
    for j, s in enumerate(status.detach().cpu().tolist()):
        if s in JPEG_BANK_STATUS:
            raise ValueError('jpeg_decode_indexed: place %d has status %d (%s)' % (j, s, names[s]))
        if s != 0:
            raise ValueError('jpeg_decode_indexed: the file of place %d is damaged (status %d: %s)' % (j, s, names.get(s, 'unknown')))


def jpeg_scan_segments_host(data, begin: int, end: int, expected: int):
    """The definition of the device's marker scan (jpeg_bank_scan_kernel): data[begin:end] are the entropy-coded bytes of one
    file whose EOI stands at `end` -> [(first byte, end byte)] of its restart intervals, cut at every pair FF D0..D7 (inside
    a scan an FF is followed by 00, an RSTn or EOI alone, so such a pair is a marker wherever it stands), or None where
    they are not `expected` many.  For a file of jpeg_encode_host these are jpeg_parse(file).segments."""
    data = bytes(data)
    out, first, at = [], begin, begin
    while at + 1 < end:
        if data[at] == 0xFF and 0xD0 <= data[at + 1] <= 0xD7:
            out.append((first, at))
            first = at = at + 2
        else:
            at += 1
    out.append((first, end))
    return out if len(out) == expected else None


# ------------------------------------------------------------------------------------------ NV12 frames
# DESIGN.md "NV12 frames": what a video decoder hands back.  A frame is Hs rows of Y followed by Hs / 2 rows of Ws / 2
# interleaved (Cb, Cr) pairs: uint8 (N, 3 * Hs / 2, Ws) or, for clips, (B, T, 3 * Hs / 2, Ws), Hs and Ws even.  The last
# dimension is contiguous; the row stride (a decoder's pitch >= Ws) and the frame stride are whatever the tensor's strides
# say.  Pixel (y, x) takes the chroma pair (y >> 1, x >> 1): nearest chroma, no interpolation.
NV12_MATRICES = {'bt601': (Fraction(299, 1000), Fraction(114, 1000)), 'bt709': (Fraction(2126, 10000), Fraction(722, 10000))}
YUV_MATRICES = ('bt601', 'bt709', 'jfif')


def nv12_coefficients(matrix: str):
    """(ky, yoff, krv, kgu, kgv, kbu) of _ycc_to_rgb for `matrix`.  'bt601' and 'bt709' are limited range (Y 16..235, chroma
    16..240): with Kg = 1 - Kr - Kb the exact rationals are ky = 255 / 219, krv = 255 / 224 * 2 (1 - Kr), kgu = 255 / 224 *
    2 Kb (1 - Kb) / Kg, kgv = 255 / 224 * 2 Kr (1 - Kr) / Kg, kbu = 255 / 224 * 2 (1 - Kb); each becomes round(65536 c).
    'jfif' is full range with the JPEG decoder's own integers."""
    if matrix == 'jfif':
        return JFIF_COEFFICIENTS
    if matrix not in NV12_MATRICES:
        raise ValueError("matrix must be 'bt601', 'bt709' or 'jfif', got %r" % (matrix,))
    kr, kb = NV12_MATRICES[matrix]
    kg = 1 - kr - kb
    c = Fraction(255, 224)
    exact = (Fraction(255, 219), c * 2 * (1 - kr), c * 2 * kb * (1 - kb) / kg, c * 2 * kr * (1 - kr) / kg, c * 2 * (1 - kb))
    ky, krv, kgu, kgv, kbu = ((v * 65536 + Fraction(1, 2)).__floor__() for v in exact)
    return (ky, 16, krv, kgu, kgv, kbu)


def check_nv12(frames):
    """(Hs, Ws) of an NV12 batch uint8 (N, 3 * Hs / 2, Ws) or (B, T, 3 * Hs / 2, Ws).  TypeError for anything but a uint8
    tensor; ValueError for a wrong rank, a row count that is no multiple of 3, odd Hs or Ws, or a last dimension that is
    not contiguous."""
    if not torch.is_tensor(frames):
        raise TypeError('NV12 frames must be a uint8 tensor, got %s' % type(frames).__name__)
    if frames.dtype != torch.uint8:
        raise TypeError('NV12 frames must be uint8, got %s' % frames.dtype)
    if frames.dim() not in (3, 4):
        raise ValueError('NV12 frames must be (N, 3 * Hs / 2, Ws) or (B, T, 3 * Hs / 2, Ws), got %s' % (tuple(frames.shape),))
    rows, Ws = int(frames.shape[-2]), int(frames.shape[-1])
    if rows < 3 or rows % 3 != 0:
        raise ValueError('NV12 frames have 3 * Hs / 2 rows (Hs of Y, Hs / 2 of CbCr), got %d' % rows)
    Hs = rows // 3 * 2
    if Hs % 2 != 0 or Ws < 2 or Ws % 2 != 0:
        raise ValueError('NV12 frames need even sizes, got Hs=%d Ws=%d' % (Hs, Ws))
    if frames.stride(-1) != 1:
        raise ValueError('NV12 frames need a contiguous last dimension (a row of bytes), got strides %s' % (tuple(frames.stride()),))
    return Hs, Ws


def nv12_to_rgb_host(frames: Tensor, matrix: str = 'bt709') -> Tensor:
    """The definition on the host: NV12 uint8 (N, 3 * Hs / 2, Ws) or (B, T, 3 * Hs / 2, Ws) -> packed RGB uint8 (N, Hs, Ws, 3)
    / (B, T, Hs, Ws, 3) through _ycc_to_rgb with nv12_coefficients(matrix); int32 arithmetic only.  Input bytes outside the
    nominal range are legal and clamp."""
    Hs, Ws = check_nv12(frames)
    coef = nv12_coefficients(matrix)
    src = frames.cpu()
    Y = src[..., :Hs, :].to(torch.int32)
    cbcr = src[..., Hs:, :].to(torch.int32)
    yi, xi = torch.arange(Hs) >> 1, torch.arange(Ws) >> 1
    Cb = cbcr[..., 0::2][..., yi, :][..., xi]
    Cr = cbcr[..., 1::2][..., yi, :][..., xi]
    return _ycc_to_rgb(Y, Cb - 128, Cr - 128, coef).contiguous().to(frames.device)


def crop_resize_nv12_host(frames: Tensor, boxes: Tensor, S: int, matrix: str = 'bt709') -> Tensor:
    """The definition of ops.crop_resize_nv12: crop_resize_host(nv12_to_rgb_host(frames, matrix), boxes, S)"""
    return crop_resize_host(nv12_to_rgb_host(frames, matrix), boxes, S)


def rgb_to_nv12_host(u8: Tensor, matrix: str = 'bt709') -> Tensor:
    """A plain float64 encoder, to make NV12 from RGB fixtures: uint8 (..., Hs, Ws, 3) with Hs, Ws even -> NV12 uint8
    (..., 3 * Hs / 2, Ws), contiguous.  Y' = Kr R + Kg G + Kb B, Pb = (B - Y') / (2 (1 - Kb)), Pr = (R - Y') / (2 (1 - Kr));
    limited range: Y = 16 + 219 Y' / 255, C = 128 + 224 P / 255; 'jfif': Y = Y', C = 128 + P (BT.601 weights); chroma is the
    mean of its 2 x 2 pixels; round half up, clamp to 0..255.  Runs where u8 lives.  It promises nothing bit-wise: nv12_to_rgb_host of its result
    is close to the input where the 2 x 2 blocks are flat, no more."""
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() < 3 or u8.shape[-1] != 3:
        raise ValueError('rgb_to_nv12_host expects uint8 (..., Hs, Ws, 3)')
    Hs, Ws = int(u8.shape[-3]), int(u8.shape[-2])
    if Hs < 2 or Ws < 2 or Hs % 2 or Ws % 2:
        raise ValueError('NV12 frames need even sizes, got Hs=%d Ws=%d' % (Hs, Ws))
    if matrix not in YUV_MATRICES:
        raise ValueError("matrix must be 'bt601', 'bt709' or 'jfif', got %r" % (matrix,))
    kr, kb = (float(v) for v in NV12_MATRICES['bt601' if matrix == 'jfif' else matrix])
    ys, cs = (1.0, 1.0) if matrix == 'jfif' else (219.0 / 255.0, 224.0 / 255.0)
    R, G, B = u8.to(torch.float64).unbind(-1)
    yp = kr * R + (1.0 - kr - kb) * G + kb * B
    lead = tuple(u8.shape[:-3])

    def pool(p):
        return p.reshape(lead + (Hs // 2, 2, Ws // 2, 2)).mean(dim=(-3, -1))

    Y = (0.0 if matrix == 'jfif' else 16.0) + ys * yp
    Cb = 128.0 + cs * pool((B - yp) / (2.0 * (1.0 - kb)))
    Cr = 128.0 + cs * pool((R - yp) / (2.0 * (1.0 - kr)))
    out = torch.empty(lead + (Hs + Hs // 2, Ws), dtype=torch.uint8, device=u8.device)
    out[..., :Hs, :] = torch.floor(Y + 0.5).clamp_(0, 255).to(torch.uint8)
    out[..., Hs:, 0::2] = torch.floor(Cb + 0.5).clamp_(0, 255).to(torch.uint8)
    out[..., Hs:, 1::2] = torch.floor(Cr + 0.5).clamp_(0, 255).to(torch.uint8)
    return out


# ------------------------------------------------------------------------------------------ aligned crops
# DESIGN.md "Aligned crops": whole frames uint8 (n, Hs, Ws, 3) and one similarity per frame, M float32 (n, 2, 3) -> uint8
# (n, S, S, 3).  M takes the CENTRE of output pixel (ox, oy) to continuous source coordinates; source pixel j covers
# [j, j + 1) and has its centre at j + 0.5, the convention of resize_weights:
#
#     cx = m00 (ox + .5) + m01 (oy + .5) + m02        cy = m10 (ox + .5) + m11 (oy + .5) + m12
#     u = (m00, m10), v = (m01, m11);  e1 = u / |u|, e2 = v / |v|;  s = sqrt(|det|);  sup = max(s, 1)
#     for every integer (jx, jy):  d = (jx + .5 - cx, jy + .5 - cy)
#         w = max(0, 1 - |d . e1| / sup) * max(0, 1 - |d . e2| / sup)
#     value_c = sum w * frame[clamp(jy, 0, Hs - 1), clamp(jx, 0, Ws - 1), c] / sum w        (all in float64)
#     byte = clamp(floor(value + 0.5), 0, 255)
#
# the antialiased triangle of crop_resize in the rotated frame of the output, with the border replicated: an aligned face
# next to the frame's edge still gives a crop.  ops.warp_similarity_u8 is the device kernel, warp_similarity_host the
# definition.
MIN_SIMILARITY_SCALE = 2.0 ** -6
MAX_SIMILARITY_SCALE = 8.0                 # about 4 sup^2 taps per pixel: some 260 at the most
SIMILARITY_TOLERANCE = 1e-4


def _similarity_parts(M: Tensor):
    """float64 pieces of a table (n, 2, 3): |u|, |v|, u . v, s = sqrt |det|"""
    m = M.detach().cpu().to(torch.float64)
    m00, m01, m10, m11 = m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1]
    nu = torch.sqrt(m00 * m00 + m10 * m10)
    nv = torch.sqrt(m01 * m01 + m11 * m11)
    return m, nu, nv, m00 * m01 + m10 * m11, torch.sqrt((m00 * m11 - m01 * m10).abs())


def check_similarities(M, n: int, Hs: int, Ws: int, S: int) -> Tensor:
    """Host validation of a table of similarities before any launch: float32 (n, 2, 3), every number finite; a similarity,
    ||u| - |v|| <= 1e-4 max(|u|, |v|) and |u . v| <= 1e-4 |u| |v| for the columns u = (m00, m10), v = (m01, m11); a scale
    s = sqrt |det| with 2^-6 <= s <= 8; and the image of the output centre (S / 2, S / 2) inside [0, Ws] x [0, Hs]
    (IndexError otherwise).  Returns the table on the host (a device tensor is copied back, which waits for the device: hand
    over the host tensor)."""
    if S is None or S < 1:
        raise ValueError('similarities need the output side S >= 1, got %r' % (S,))
    if not torch.is_tensor(M):
        raise TypeError('similarities must be a float32 tensor (n, 2, 3), got %s' % type(M).__name__)
    if M.dtype != torch.float32:
        raise TypeError('similarities must be float32, got %s' % M.dtype)
    if M.dim() != 3 or tuple(M.shape) != (n, 2, 3):
        raise ValueError('similarities must have shape (%d, 2, 3), one 2 x 3 map per entry, got %s' % (n, tuple(M.shape)))
    t = M.detach().cpu()
    if not bool(torch.isfinite(t).all()):
        raise ValueError('similarities: every entry must be finite')
    m, nu, nv, dot, s = _similarity_parts(t)
    tol = SIMILARITY_TOLERANCE
    if bool(((nu - nv).abs() > tol * torch.maximum(nu, nv)).any()) or bool((dot.abs() > tol * nu * nv).any()):
        raise ValueError('similarities: a rotation, a uniform scale and an optional mirror expected (columns of equal length '
                         'at right angles, to 1e-4); general affine maps are not supported')
    if bool((s < MIN_SIMILARITY_SCALE).any()) or bool((s > MAX_SIMILARITY_SCALE).any()):
        raise ValueError('similarities: the scale sqrt|det| (source pixels per output pixel) must lie in [2^-6, 8], got '
                         '[%g, %g]' % (float(s.min()), float(s.max())))
    h = 0.5 * S
    px = (m[:, 0, 0] * h + m[:, 0, 1] * h) + m[:, 0, 2]
    py = (m[:, 1, 0] * h + m[:, 1, 1] * h) + m[:, 1, 2]
    if bool((px < 0).any()) or bool((px > Ws).any()) or bool((py < 0).any()) or bool((py > Hs).any()):
        raise IndexError('similarities: the output centre (%g, %g) must land inside the frame [0, %d] x [0, %d], got x in '
                         '[%g, %g], y in [%g, %g]' % (h, h, Ws, Hs, float(px.min()), float(px.max()), float(py.min()),
                                                     float(py.max())))
    return t


def per_frame_similarities(M: Tensor, T: int) -> Tensor:
    """(B, 2, 3) per-clip table -> (B*T, 2, 3) per-frame table (each clip's map repeated for its T frames), where `M` lives"""
    return M.repeat_interleave(T, dim=0).contiguous()


def warp_similarity_host(u8: Tensor, M: Tensor, S: int) -> Tensor:
    """The definition on the host, in float64: uint8 (n, Hs, Ws, 3) or (B, T, Hs, Ws, 3) and M float32 (n, 2, 3) / (B, 2, 3)
    -> uint8 (n, S, S, 3) / (B, T, S, S, 3), as the comment above states it.  Every output pixel sums the (2 K + 1)^2 source
    pixels around the pixel under its centre, K = ceil(sqrt 2 sup) + 1: all that can have a weight, one pass over the S x S
    output per tap offset (memory does not grow with s; the passes do, 729 at s = 8).  Documentation and a
    reference for tests: the device path is ops.warp_similarity_u8 (double sums in another order: a byte may differ by one
    where the value lies within rounding of a half)."""
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError('warp_similarity_host expects uint8 (n, Hs, Ws, 3) or (B, T, Hs, Ws, 3), got %s %s'
                         % (u8.dtype, tuple(u8.shape)))
    lead = tuple(u8.shape[:-3])
    Hs, Ws = int(u8.shape[-3]), int(u8.shape[-2])
    t = check_similarities(M, u8.shape[0], Hs, Ws, S)
    if u8.dim() == 5:
        t = per_frame_similarities(t, u8.shape[1])
    src = u8.reshape((-1, Hs, Ws, 3)).cpu()
    m, nu, nv, _, sc = _similarity_parts(t)
    out = torch.empty((src.shape[0], S, S, 3), dtype=torch.uint8)
    o = torch.arange(S, dtype=torch.float64) + 0.5
    for i in range(src.shape[0]):
        sup = max(float(sc[i]), 1.0)
        e1 = (float(m[i, 0, 0] / nu[i]), float(m[i, 1, 0] / nu[i]))
        e2 = (float(m[i, 0, 1] / nv[i]), float(m[i, 1, 1] / nv[i]))
        cx = (m[i, 0, 0] * o[None, :] + m[i, 0, 1] * o[:, None]) + m[i, 0, 2]             # (S, S): [oy, ox]
        cy = (m[i, 1, 0] * o[None, :] + m[i, 1, 1] * o[:, None]) + m[i, 1, 2]
        bx, by = torch.floor(cx).to(torch.int64), torch.floor(cy).to(torch.int64)
        K = int(math.ceil(math.sqrt(2.0) * sup)) + 1
        img = src[i].to(torch.float64)
        num = torch.zeros((S, S, 3), dtype=torch.float64)
        den = torch.zeros((S, S), dtype=torch.float64)
        for ky in range(-K, K + 1):                            # one pass per tap offset: (S, S) at a time, whatever s is
            jy = by + ky
            dy = jy.to(torch.float64) + 0.5 - cy
            yc = jy.clamp(0, Hs - 1)
            for kx in range(-K, K + 1):
                jx = bx + kx
                dx = jx.to(torch.float64) + 0.5 - cx
                w = (1.0 - (dx * e1[0] + dy * e1[1]).abs() / sup).clamp_(min=0.0) * \
                    (1.0 - (dx * e2[0] + dy * e2[1]).abs() / sup).clamp_(min=0.0)
                num += w[:, :, None] * img[yc, jx.clamp(0, Ws - 1)]
                den += w
        out[i] = torch.floor(num / den[:, :, None] + 0.5).clamp_(0, 255).to(torch.uint8)
    return out.reshape(lead + (S, S, 3)).to(u8.device)


def similarity_of_boxes(boxes: Tensor, S: int) -> Tensor:
    """Square boxes int32 (n, 4) = (y0, x0, h, w) with h == w as similarities: M = [[s, 0, x0], [0, s, y0]], s = h / S, float32
    (n, 2, 3) where `boxes` lives.  Away from the crop's border (output rows and columns 1 .. S - 2) the warp then weighs
    what crop_resize weighs; in the border it sees the frame outside the box, which the crop does not.  ValueError for
    h != w."""
    if not torch.is_tensor(boxes) or boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise TypeError('similarity_of_boxes: boxes must be an int32 tensor (n, 4) = (y0, x0, h, w)')
    if S is None or S < 1:
        raise ValueError('similarity_of_boxes: the output side S >= 1, got %r' % (S,))
    if bool((boxes[:, 2] != boxes[:, 3]).any()):
        raise ValueError('similarity_of_boxes: a similarity has one scale: square boxes (h == w) only')
    b = boxes.to(torch.float64)
    M = torch.zeros((boxes.shape[0], 2, 3), dtype=torch.float64, device=boxes.device)
    M[:, 0, 0] = M[:, 1, 1] = b[:, 2] / S
    M[:, 0, 2], M[:, 1, 2] = b[:, 1], b[:, 0]
    return M.to(torch.float32)


def similarity_from_landmarks(landmarks: Tensor, template: Tensor, S: Optional[int] = None) -> Tensor:
    """The similarity that lays a template over detected landmarks: landmarks float (n, K, 2) as (x, y) in source
    coordinates, template (K, 2) as (x, y) in coordinates of the output crop, K >= 2 -> M float32 (n, 2, 3), output to
    source, as ops.warp_similarity_u8 takes it.  BOTH arguments use continuous coordinates in which pixel j covers [j, j + 1)
    and has its centre at j + 0.5: a detector that reports pixel indices adds 0.5.  The template is the caller's (none is
    shipped); with S given it must lie inside the crop [0, S]^2.

    Least squares over rotation, uniform scale and translation, without reflection, closed form in float64: with p' = p -
    mean p (template) and q' = q - mean q (landmarks), a = sum(p' . q') / sum |p'|^2, b = sum(p'x q'y - p'y q'x) / sum |p'|^2,
    A = [[a, -b], [b, a]], t = mean q - A mean p.  ValueError for K < 2 and for a template whose points coincide."""
    if not torch.is_tensor(landmarks) or not torch.is_tensor(template):
        raise TypeError('similarity_from_landmarks: landmarks and template must be tensors')
    if not landmarks.is_floating_point() or landmarks.dim() != 3 or landmarks.shape[2] != 2:
        raise ValueError('similarity_from_landmarks: landmarks must be float (n, K, 2), got %s %s'
                         % (landmarks.dtype, tuple(landmarks.shape)))
    K = int(landmarks.shape[1])
    if K < 2:
        raise ValueError('similarity_from_landmarks: two points at least determine a similarity, got K = %d' % K)
    if template.dim() != 2 or tuple(template.shape) != (K, 2):
        raise ValueError('similarity_from_landmarks: the template must be (%d, 2), got %s' % (K, tuple(template.shape)))
    p = template.detach().cpu().to(torch.float64)
    q = landmarks.detach().cpu().to(torch.float64)
    if not bool(torch.isfinite(p).all()) or not bool(torch.isfinite(q).all()):
        raise ValueError('similarity_from_landmarks: every coordinate must be finite')
    if S is not None and (bool((p < 0).any()) or bool((p > S).any())):
        raise ValueError('similarity_from_landmarks: the template must lie inside the crop [0, %d]^2' % S)
    pm, qm = p.mean(0), q.mean(1)
    pc, qc = p - pm, q - qm[:, None, :]
    den = (pc * pc).sum()
    if float(den) <= 1e-24 * max(1.0, float((p * p).sum())):
        raise ValueError('similarity_from_landmarks: the points of the template coincide')
    a = (pc[None] * qc).sum(dim=(1, 2)) / den
    b = (pc[None, :, 0] * qc[:, :, 1] - pc[None, :, 1] * qc[:, :, 0]).sum(1) / den
    M = torch.empty((q.shape[0], 2, 3), dtype=torch.float64)
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = a, -b, b, a
    M[:, 0, 2] = qm[:, 0] - (a * pm[0] - b * pm[1])
    M[:, 1, 2] = qm[:, 1] - (b * pm[0] + a * pm[1])
    return M.to(torch.float32).to(landmarks.device)


def similarities_of_squares(side: Tensor, angle: Tensor, cx: Tensor, cy: Tensor, mirror: Tensor, S: int) -> Tensor:
    """The one place that writes the matrix convention down: a source square of side `side` pixels around (cx, cy), turned
    by `angle` (radians, counter-clockwise in (x, y) with y down the frame) and mirrored where `mirror` is true, as the map of
    an S x S crop: M = s R(angle) with s = side / S, the first column negated for a mirror, the output centre (S / 2, S / 2)
    taken to (cx, cy).  All arguments (n,) tensors; computed in float64 -> float32 (n, 2, 3) on the host.  A side within 1e-6
    of S / 64 or 8 S is moved inside by that much, so that the float32 rounding of s cos and s sin cannot carry sqrt |det|
    over a limit of check_similarities (a float32 has 6e-8)."""
    side = side.detach().cpu().to(torch.float64).clamp(S * MIN_SIMILARITY_SCALE * (1.0 + 1e-6), S * MAX_SIMILARITY_SCALE * (1.0 - 1e-6))
    angle, cx, cy = (t.detach().cpu().to(torch.float64) for t in (angle, cx, cy))
    sgn = torch.where(mirror.detach().cpu().to(torch.bool), -1.0, 1.0).to(torch.float64)
    s, cos, sin = side / S, torch.cos(angle), torch.sin(angle)
    M = torch.empty((side.shape[0], 2, 3), dtype=torch.float64)
    M[:, 0, 0], M[:, 0, 1] = sgn * s * cos, -s * sin
    M[:, 1, 0], M[:, 1, 1] = sgn * s * sin, s * cos
    M[:, 0, 2] = cx - (M[:, 0, 0] + M[:, 0, 1]) * (0.5 * S)
    M[:, 1, 2] = cy - (M[:, 1, 0] + M[:, 1, 1]) * (0.5 * S)
    return M.to(torch.float32).contiguous()


def random_similarities(B: int, Hs: int, Ws: int, S: int, scale=(0.5, 1.0), degrees: float = 10.0, flip_p: float = 0.5,
                        generator: Optional[torch.Generator] = None) -> Tensor:
    """One random similarity per clip for rotation, scale and flip augmentation in one table: the source square has the side
    random_boxes draws for a square (area `scale`, uniform, of min(Hs, Ws) ** 2; cut to [S / 64, 8 S]), the angle is uniform
    in [-degrees, degrees], the mirror (probability flip_p) is folded into the matrix, and the centre is uniform over the
    positions that keep the rotated square inside the frame (the frame's centre along an axis that has none).  Returns a
    float32 (B, 2, 3) host tensor, reproducible from `generator`.  A training step is then
    ``model(ops.warp_similarity_u8(u8, M.to(dev), S))``: no view is needed, the flip is in M."""
    if B < 1 or Hs < 1 or Ws < 1 or S < 1:
        raise ValueError('random_similarities: need B, Hs, Ws, S >= 1, got B=%d Hs=%d Ws=%d S=%d' % (B, Hs, Ws, S))
    if not (0.0 < scale[0] <= scale[1] <= 1.0):
        raise ValueError('random_similarities: need 0 < scale[0] <= scale[1] <= 1, got %r' % (scale,))
    if not 0.0 <= degrees <= 180.0:
        raise ValueError('random_similarities: degrees must lie in [0, 180], got %r' % (degrees,))
    if not 0.0 <= flip_p <= 1.0:
        raise ValueError('random_similarities: flip_p must be a probability, got %r' % (flip_p,))
    u = torch.rand((5, B), generator=generator, dtype=torch.float64)
    area = (scale[0] + (scale[1] - scale[0]) * u[0]) * float(min(Hs, Ws)) ** 2
    # cut to the scales a similarity may have; similarities_of_squares keeps a side that lands on a limit just inside it
    side = torch.sqrt(area).round().clamp_(1, min(Hs, Ws)).clamp_(S * MIN_SIMILARITY_SCALE, S * MAX_SIMILARITY_SCALE)
    ang = (2.0 * u[1] - 1.0) * (degrees * math.pi / 180.0)
    cos, sin = torch.cos(ang), torch.sin(ang)
    half = 0.5 * side * (cos.abs() + sin.abs())                # half the bounding box of the rotated square
    cx = torch.where(Ws - 2.0 * half > 0, half + u[2] * (Ws - 2.0 * half), torch.full_like(half, 0.5 * Ws))
    cy = torch.where(Hs - 2.0 * half > 0, half + u[3] * (Hs - 2.0 * half), torch.full_like(half, 0.5 * Hs))
    return similarities_of_squares(side, ang, cx, cy, u[4] < flip_p, S)


# ------------------------------------------------------------------------------------------ perturbations
# DESIGN.md "Perturbations": the degradations a robustness table grades a detector by, next to JPEG -- brightness, contrast,
# saturation, Gaussian noise, Gaussian blur, pixelation -- bytes to bytes in int32 arithmetic with arithmetic shifts and no
# floating point on the pixel path.  A frame's row of the table is (kind, param, frame_id, stream); ops.perturb_u8 is the
# device kernel and gives the bits of perturb_host.
PERTURBATION_KINDS = ('copy', 'brightness', 'contrast', 'saturation', 'noise', 'blur', 'pixelate')
PERTURB_TAPS = 21                          # taps of a blur row: radius 10 around index 10
PERTURB_TAPS_SUM = 2048                    # a row sums to 2^11: two passes leave 22 bits to shift out
PERTURB_MAX_TAPS_ROWS = 16
PERTURB_PARAM_RANGE = {0: None, 1: (0, 1024), 2: (0, 1024), 3: (0, 1024), 4: (0, 1023), 5: None, 6: (2, 32)}
# Five steps per kind for a robustness table, mild to severe, in the units clips.perturbation takes.  The steps are this
# project's choice: the usual protocol names the distortions and that there are five levels of each, not these numbers.
PERTURBATION_LEVELS = {
    'brightness': (0.9, 0.8, 0.7, 0.6, 0.5),
    'contrast': (0.85, 0.725, 0.6, 0.475, 0.35),
    'saturation': (0.8, 0.6, 0.4, 0.2, 0.0),
    'noise': (4.0, 8.0, 12.0, 16.0, 20.0),
    'blur': (0.8, 1.6, 2.4, 3.2, 4.0),
    'pixelate': (2, 3, 4, 5, 6),
}


def _mulhilo32(m: int, c: Tensor):
    """(high, low) 32-bit words of m * c for a 32-bit constant m and int64 c in [0, 2^32), without leaving int64"""
    a, b = m * (c >> 16), m * (c & 0xffff)                         # both below 2^48; m * c = a * 2^16 + b
    return (a + (b >> 16)) >> 16, (((a & 0xffff) << 16) + b) & 0xffffffff


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror and Shaw, SC'11): counter = four int64 tensors of one shape (or Python ints) holding
    32-bit words, key = two 32-bit Python ints -> the four output words, int64 tensors in [0, 2^32)."""
    c0, c1, c2, c3 = torch.broadcast_tensors(*[torch.as_tensor(c, dtype=torch.int64) & 0xffffffff for c in counter])
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        h0, l0 = _mulhilo32(0xD2511F53, c0)
        h1, l1 = _mulhilo32(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c0, c1, c2, c3


def gaussian_taps(sigmas) -> Tensor:
    """One blur row per sigma in [0.3, 4], int32 (K, 21), K <= 16: w_i = exp(-i^2 / 2 sigma^2) for |i| <= min(10, ceil(3 sigma))
    and zero outside, in float64; scaled so that the row sums to 2048 and rounded half up; what the rounding leaves of 2048
    goes to the centre tap.  The kernel reads these integers only."""
    sigmas = [float(s) for s in (sigmas if isinstance(sigmas, (list, tuple)) else [sigmas])]
    if not 1 <= len(sigmas) <= PERTURB_MAX_TAPS_ROWS:
        raise ValueError('gaussian_taps: between 1 and %d sigmas, got %d' % (PERTURB_MAX_TAPS_ROWS, len(sigmas)))
    rows = []
    for s in sigmas:
        if not 0.3 <= s <= 4.0:
            raise ValueError('gaussian_taps: sigma must lie in [0.3, 4], got %r' % (s,))
        R = min(PERTURB_TAPS // 2, math.ceil(3.0 * s))
        w = [math.exp(-(i * i) / (2.0 * s * s)) if abs(i) <= R else 0.0 for i in range(-10, 11)]
        tot = sum(w)
        t = [int(math.floor(v * PERTURB_TAPS_SUM / tot + 0.5)) for v in w]
        t[10] += PERTURB_TAPS_SUM - sum(t)
        rows.append(t)
    return torch.tensor(rows, dtype=torch.int32)


def check_perturbations(table, n: int, taps=None) -> Tensor:
    """Host validation of a perturbation table before any launch: int32 (n, 4) = (kind, param, frame_id, stream) per frame or
    clip; kind in 0..6 (PERTURBATION_KINDS); param 0..1024 for the Q8 gains of kinds 1 to 3, 0..1023 for the Q4 sigma of kind
    4, a row of `taps` for kind 5, 2..32 for the block side of kind 6, anything for kind 0; frame_id and stream >= 0.  taps,
    whenever it is passed: int32 (K, 21), 1 <= K <= 16, every row symmetric about index 10, non-negative and summing to
    exactly 2048; a table with a kind 5 row needs it.  Returns the table on the host (a device tensor is copied back, which
    waits for the device: hand over the loader's host tensor)."""
    if not torch.is_tensor(table):
        raise TypeError('perturbations: the table must be an int32 tensor (n, 4), got %s' % type(table).__name__)
    if table.dtype != torch.int32:
        raise TypeError('perturbations: the table must be int32, got %s' % table.dtype)
    if table.dim() != 2 or tuple(table.shape) != (n, 4):
        raise ValueError('perturbations: the table must have shape (%d, 4) = (kind, param, frame_id, stream) per entry, got %s'
                         % (n, tuple(table.shape)))
    K = 0
    if taps is not None:
        if not torch.is_tensor(taps):
            raise TypeError('perturbations: taps must be an int32 tensor (K, 21), got %s' % type(taps).__name__)
        if taps.dtype != torch.int32:
            raise TypeError('perturbations: taps must be int32, got %s' % taps.dtype)
        if taps.dim() != 2 or taps.shape[1] != PERTURB_TAPS or not 1 <= taps.shape[0] <= PERTURB_MAX_TAPS_ROWS:
            raise ValueError('perturbations: taps must have shape (K, 21) with 1 <= K <= %d, got %s'
                             % (PERTURB_MAX_TAPS_ROWS, tuple(taps.shape)))
        tp = taps.detach().cpu()
        if bool((tp < 0).any()) or not torch.equal(tp, tp.flip(1)) or bool((tp.sum(1) != PERTURB_TAPS_SUM).any()):
            raise ValueError('perturbations: every row of taps must be non-negative, symmetric about index 10 and sum to %d'
                             % PERTURB_TAPS_SUM)
        K = int(tp.shape[0])
    t = table.detach().cpu()
    kind, param = t[:, 0], t[:, 1]
    if bool((kind < 0).any()) or bool((kind >= len(PERTURBATION_KINDS)).any()):
        raise ValueError('perturbations: kind must lie in [0, %d], got [%d, %d]'
                         % (len(PERTURBATION_KINDS) - 1, int(kind.min()), int(kind.max())))
    for k, rng in PERTURB_PARAM_RANGE.items():
        if rng is not None and bool(((kind == k) & ((param < rng[0]) | (param > rng[1]))).any()):
            raise ValueError('perturbations: the param of kind %d (%s) must lie in [%d, %d]' % (k, PERTURBATION_KINDS[k], *rng))
    blur = kind == 5
    if bool(blur.any()):
        if taps is None:
            raise ValueError('perturbations: a blurred frame (kind 5) needs taps (clips.gaussian_taps)')
        if bool((blur & ((param < 0) | (param >= K))).any()):
            raise ValueError('perturbations: the param of kind 5 (blur) names a row of taps, 0..%d' % (K - 1))
    if bool((t[:, 2:] < 0).any()):
        raise ValueError('perturbations: frame_id and stream must not be negative')
    return t


def perturbation(kind_name: str, value):
    """A user's (name, strength) -> (kind, param, taps): the gain of 'brightness', 'contrast' and 'saturation' in Q8
    (round(256 value), 0..4 -> 0..1024), the sigma of 'noise' in grey levels in Q4 (round(16 value), below 64), the sigma
    of 'blur' (0.3..4) as row 0 of the one-row bank taps = gaussian_taps([value]), the block side of 'pixelate' (an int in
    2..32) as it is, and 'copy' (the value is ignored).  taps is None for every kind but 'blur'.  ValueError for a name or a
    value outside these."""
    if kind_name not in PERTURBATION_KINDS:
        raise ValueError('perturbation: the kind must be one of %s, got %r' % (', '.join(PERTURBATION_KINDS), kind_name))
    kind = PERTURBATION_KINDS.index(kind_name)
    if kind == 0:
        return 0, 0, None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value):
        raise ValueError('perturbation: %s takes a finite number, got %r' % (kind_name, value))
    if kind == 5:
        return 5, 0, gaussian_taps([value])
    if kind == 6:
        if not isinstance(value, int):
            raise ValueError('perturbation: pixelate takes an int block side, got %r' % (value,))
        param = value
    else:
        param = int(math.floor(value * (16.0 if kind == 4 else 256.0) + 0.5))
    lo, hi = PERTURB_PARAM_RANGE[kind]
    if not lo <= param <= hi:
        raise ValueError('perturbation: %s = %r gives param %d outside [%d, %d]' % (kind_name, value, param, lo, hi))
    return kind, param, None


def perturbation_table(n: int, kind_name: str, value, first_frame: int = 0, stream: int = 0):
    """"This perturbation on every frame" -> (table int32 (n, 4), taps or None): n rows (kind, param, first_frame + i, stream)
    for the n frames of one video; what VideoScorer(perturb=(kind_name, value)) applies to a video that is `stream` in its
    call and whose first frame is `first_frame`."""
    if n < 1 or first_frame < 0 or stream < 0 or first_frame + n > 2 ** 31:
        raise ValueError('perturbation_table: need n >= 1, first_frame >= 0 and stream >= 0, got %r, %r, %r' % (n, first_frame, stream))
    kind, param, taps = perturbation(kind_name, value)
    table = torch.empty((n, 4), dtype=torch.int32)
    table[:, 0], table[:, 1], table[:, 3] = kind, param, stream
    table[:, 2] = torch.arange(first_frame, first_frame + n, dtype=torch.int32)
    return table, taps


def random_perturbations(B: int, p: float = 0.5, kinds=('brightness', 'contrast', 'saturation', 'noise', 'blur', 'pixelate'),
                         generator: Optional[torch.Generator] = None, brightness=(0.6, 1.4), contrast=(0.6, 1.4),
                         saturation=(0.0, 1.5), noise=(2.0, 16.0), blur=(0.5, 3.0), pixelate=(2, 6)):
    """One random perturbation per clip for training -> (table int32 (B, 4), taps int32 (8, 21)), host tensors reproducible
    from `generator`.  A clip is perturbed with probability p and is kind 0 otherwise; the kind is uniform among `kinds`; the
    strength is uniform in the kind's range, a keyword each: the gains of brightness and contrast in [0.6, 1.4] and of
    saturation in [0, 1.5], the noise sigma in [2, 16] grey levels, the blur sigma one of the 8 rows of the bank (sigmas
    evenly spaced over [0.5, 3]: the bank depends on the range only, so it is uploaded once), the block side an int in
    [2, 6].  stream = the clip's index and frame_id is drawn from [0, 2^30): the T frames of a clip take frame_id .. frame_id +
    T - 1, so no two clips of a batch share noise, and two batches do only by a coincidence of 1 in 2^30 per pair.  The step
    is ``model(ops.perturb_u8(u8, table, taps, seed), view=flips)``, as with random_qualities and ops.jpeg_roundtrip_u8."""
    if B < 1:
        raise ValueError('random_perturbations: need B >= 1, got %d' % B)
    if not 0.0 <= p <= 1.0:
        raise ValueError('random_perturbations: p must be a probability, got %r' % (p,))
    kinds = tuple(kinds)
    if not kinds or any(k not in PERTURBATION_KINDS[1:] for k in kinds):
        raise ValueError('random_perturbations: kinds must name some of %s, got %r' % (', '.join(PERTURBATION_KINDS[1:]), kinds))
    ranges = {'brightness': brightness, 'contrast': contrast, 'saturation': saturation, 'noise': noise, 'blur': blur,
              'pixelate': pixelate}
    for k in kinds:                                                 # both ends must be values perturbation() takes
        lo, hi = ranges[k]
        if not lo <= hi:
            raise ValueError('random_perturbations: the range of %s must be (low, high), got %r' % (k, ranges[k]))
        perturbation(k, lo), perturbation(k, hi)
    rows = 8
    taps = gaussian_taps([blur[0] + (blur[1] - blur[0]) * i / (rows - 1) for i in range(rows)])
    u = torch.rand((3, B), generator=generator, dtype=torch.float64)
    fid = torch.randint(0, 2 ** 30, (B,), generator=generator)
    table = torch.zeros((B, 4), dtype=torch.int32)
    for b in range(B):
        table[b, 2], table[b, 3] = int(fid[b]), b
        if float(u[0, b]) >= p:
            continue
        name = kinds[min(int(float(u[1, b]) * len(kinds)), len(kinds) - 1)]
        lo, hi = ranges[name]
        if name == 'blur':
            kind, param = 5, min(int(float(u[2, b]) * rows), rows - 1)
        elif name == 'pixelate':
            kind, param = 6, min(int(lo) + int(float(u[2, b]) * (int(hi) - int(lo) + 1)), int(hi))
        else:
            kind, param, _ = perturbation(name, lo + (hi - lo) * float(u[2, b]))
        table[b, 0], table[b, 1] = kind, param
    return table, taps


def _luma(px: Tensor) -> Tensor:
    """the JPEG path's luma of int32 (..., 3) RGB"""
    return (19595 * px[..., 0] + 38470 * px[..., 1] + 7471 * px[..., 2] + 32768) >> 16


def _perturb_frame(v: Tensor, kind: int, p: int, fid: int, stream: int, taps, key) -> Tensor:
    """one frame int32 (H, W, 3) through one row of the table -> int32 (H, W, 3) in 0..255"""
    H, W = v.shape[0], v.shape[1]
    if kind == 1:
        return ((v * p + 128) >> 8).clamp_(0, 255)
    if kind == 2:
        m = (int(_luma(v).to(torch.int64).sum()) + H * W // 2) // (H * W)
        return (m + (((v - m) * p + 128) >> 8)).clamp_(0, 255)
    if kind == 3:
        Y = _luma(v)[..., None]
        return (Y + (((v - Y) * p + 128) >> 8)).clamp_(0, 255)
    if kind == 4:
        words = philox4x32_10((torch.arange(H * W * 3, dtype=torch.int64), fid, stream, 0), key)
        z = sum((w >> s) & 0xff for w in words for s in (0, 8, 16, 24)) - 2040
        d = ((z.to(torch.int32) * p) * 887 + (1 << 21)) >> 22
        return (v + d.reshape(H, W, 3)).clamp_(0, 255)
    if kind == 5:
        t = [int(q) for q in taps[p]]
        ys, xs = torch.arange(H), torch.arange(W)
        h = sum(t[i] * v[:, (xs + (i - 10)).clamp_(0, W - 1)] for i in range(PERTURB_TAPS) if t[i])
        a = sum(t[j] * h[(ys + (j - 10)).clamp_(0, H - 1)] for j in range(PERTURB_TAPS) if t[j])
        return ((a + (1 << 21)) >> 22).clamp_(0, 255)
    if kind == 6:
        by, bx = -(-H // p), -(-W // p)
        pad = torch.zeros((by * p, bx * p, 3), dtype=torch.int32)
        pad[:H, :W] = v
        S = pad.reshape(by, p, bx, p, 3).sum((1, 3))
        rows = (torch.arange(by) * p + p).clamp_(max=H) - torch.arange(by) * p
        cols = (torch.arange(bx) * p + p).clamp_(max=W) - torch.arange(bx) * p
        cnt = (rows[:, None] * cols[None, :]).to(torch.int32)[..., None]
        q = (S + cnt // 2) // cnt
        return q[torch.arange(H) // p][:, torch.arange(W) // p]
    return v


def perturb_host(u8: Tensor, table: Tensor, taps: Optional[Tensor] = None, seed: int = 0) -> Tensor:
    """The definition on the host: uint8 (n, H, W, 3) or (B, T, H, W, 3), any H, W >= 1, table int32 (n, 4) / (B, 4) =
    (kind, param, frame_id, stream) per frame, or per clip (frame t of a clip then takes the clip's kind, param and stream and
    frame_id + t) -> uint8 of the same shape.  int32 arithmetic with arithmetic shifts only; clamp is to 0..255, v is a byte
    of channel c at pixel (y, x), Y = (19595 R + 38470 G + 7471 B + 32768) >> 16 of its pixel:

      0 copy        v
      1 brightness  clamp((v p + 128) >> 8), p the gain in Q8
      2 contrast    clamp(m + (((v - m) p + 128) >> 8)), m = (sum of Y over the frame + H W // 2) // (H W), the sum in 64 bits
      3 saturation  clamp(Y + (((v - Y) p + 128) >> 8))
      4 noise       clamp(v + d), d = ((z p) 887 + (1 << 21)) >> 22, p the sigma in Q4 grey levels; z = the sum of the 16 bytes
                    of Philox4x32-10(counter ((y W + x) 3 + c, frame_id, stream, 0), key (seed & 0xffffffff, seed >> 32)) less
                    2040: Irwin-Hall, standard deviation 295.6, and 2^22 / (16 * 295.6) = 886.8
      5 blur        clamp((sum_j t[j] sum_i t[i] v(y + j - 10, x + i - 10) + (1 << 21)) >> 22), t = taps[p], coordinates
                    clamped into the frame (the border replicates)
      6 pixelate    (S + cnt // 2) // cnt over the p x p block that holds the pixel, blocks laid from the frame's corner and
                    cut to the frame: S the block's sum of channel c, cnt its real number of pixels

    With p = 256 kinds 1 to 3 are the identity.  The noise of a byte depends on (seed, stream, frame_id, y, x, c) alone."""
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3 or u8.numel() == 0:
        raise ValueError('perturb_host expects non-empty uint8 (n, H, W, 3) or (B, T, H, W, 3), got %s %s'
                         % (u8.dtype, tuple(u8.shape)))
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError('perturb_host: the seed must lie in [0, 2^64), got %d' % seed)
    t = check_perturbations(table, u8.shape[0], taps)
    T = u8.shape[1] if u8.dim() == 5 else 1
    H, W = u8.shape[-3], u8.shape[-2]
    src = u8.reshape((-1, H, W, 3)).cpu()
    tp = None if taps is None else taps.detach().cpu()
    key = (seed & 0xffffffff, seed >> 32)
    out = torch.empty_like(src)
    for f in range(src.shape[0]):
        kind, p, fid, stream = (int(q) for q in t[f // T])
        out[f] = _perturb_frame(src[f].to(torch.int32), kind, p, fid + f % T, stream, tp, key).to(torch.uint8)
    return out.reshape(u8.shape).to(u8.device)


# ------------------------------------------------------------------------------------------ pasting maps onto frames
# DESIGN.md "Pasting maps onto frames": a relevance map (g x g, in crop coordinates) blended onto the whole frame it was
# cut from, through the box or the similarity that cut the crop, in the frame's own format.  Per frame a 2 x 3 float64 map
# A takes the CENTRE of source pixel (sx, sy) to crop coordinates,
#
#     u = (a00 (sx + .5) + a01 (sy + .5)) + a02        v = (a10 (sx + .5) + a11 (sy + .5)) + a12
#
# and the crop covers [0, S) x [0, S): a pixel is in the region when 0 <= u < S and 0 <= v < S.  paste_geometry makes A and
# the rectangle to look at, paste_maps_host is the definition, ops.relevance_paste_u8 / _nv12 are the device kernels.
PASTE_MAX_GRID = 19


def _paste_rect(xlo, xhi, ylo, yhi, Hs: int, Ws: int, even: bool) -> Tensor:
    """(y0, x0, h, w) int32 of the pixel ranges [xlo, xhi) x [ylo, yhi) (int64 tensors) clamped into the frame, aligned
    outward to even coordinates for NV12"""
    x0, x1 = xlo.clamp(0, Ws), xhi.clamp(0, Ws)
    y0, y1 = ylo.clamp(0, Hs), yhi.clamp(0, Hs)
    if even:
        x0, y0 = x0 - x0 % 2, y0 - y0 % 2
        x1, y1 = (x1 + x1 % 2).clamp(max=Ws), (y1 + y1 % 2).clamp(max=Hs)
    return torch.stack([y0, x0, (y1 - y0).clamp(min=0), (x1 - x0).clamp(min=0)], dim=1).to(torch.int32).contiguous()


def paste_geometry(n: int, Hs: int, Ws: int, S: int, boxes=None, transforms=None, even: bool = False):
    """The geometry of a paste from the table that cut the crops: exactly one of boxes int32 (n, 4) = (y0, x0, h, w)
    (check_boxes; h != w is fine) and transforms float32 (n, 2, 3) (check_similarities) -> (A float64 (n, 2, 3), rect int32
    (n, 4) = (y0, x0, h, w)), both on the host.  A box gives A = [[S / w, 0, -x0 S / w], [0, S / h, -y0 S / h]]; a similarity M
    gives the closed-form float64 inverse of the float32 table.  rect is the bounding rectangle of the crop square's image in
    the frame, widened by one pixel and clamped into the frame (even=True, for NV12 frames: aligned outward to even
    coordinates; Hs and Ws must be even).  It says only where a kernel has to look: whether a pixel is inside is decided by
    (u, v), so a rectangle that is too large is harmless."""
    if (boxes is None) == (transforms is None):
        raise ValueError('paste_geometry: boxes and transforms are two ways to cut the same crop: pass exactly one of them')
    if even and (Hs % 2 or Ws % 2):
        raise ValueError('paste_geometry: even=True needs even Hs and Ws, got %d x %d' % (Hs, Ws))
    A = torch.zeros((n, 2, 3), dtype=torch.float64)
    if boxes is not None:
        b = check_boxes(boxes, n, Hs, Ws, S).to(torch.int64)
        y0, x0, h, w = (b[:, i].to(torch.float64) for i in range(4))
        A[:, 0, 0], A[:, 1, 1] = S / w, S / h
        A[:, 0, 2], A[:, 1, 2] = -x0 * S / w, -y0 * S / h
        return A, _paste_rect(b[:, 1] - 1, b[:, 1] + b[:, 3] + 1, b[:, 0] - 1, b[:, 0] + b[:, 2] + 1, Hs, Ws, even)
    m = check_similarities(transforms, n, Hs, Ws, S).to(torch.float64)
    det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
    A[:, 0, 0], A[:, 0, 1] = m[:, 1, 1] / det, -m[:, 0, 1] / det
    A[:, 1, 0], A[:, 1, 1] = -m[:, 1, 0] / det, m[:, 0, 0] / det
    A[:, 0, 2] = -(A[:, 0, 0] * m[:, 0, 2] + A[:, 0, 1] * m[:, 1, 2])
    A[:, 1, 2] = -(A[:, 1, 0] * m[:, 0, 2] + A[:, 1, 1] * m[:, 1, 2])
    corners = torch.tensor([[0.0, 0.0, 1.0], [S, 0.0, 1.0], [0.0, S, 1.0], [S, S, 1.0]], dtype=torch.float64)
    pts = torch.einsum('nij,kj->nki', m, corners)                 # (n, 4, 2) as (x, y)
    lo, hi = torch.floor(pts.min(1).values).to(torch.int64), torch.ceil(pts.max(1).values).to(torch.int64)
    return A, _paste_rect(lo[:, 0] - 1, hi[:, 0] + 1, lo[:, 1] - 1, hi[:, 1] + 1, Hs, Ws, even)


def lut_to_ycc(lut: Tensor, matrix: str = 'bt709') -> Tensor:
    """A colour table uint8 (256, 3) of R'G'B' as (Y, Cb, Cr) uint8 (256, 3) in the space of `matrix`: the float64 forward
    formulas of rgb_to_nv12_host on every colour, rounded half up, clamped to 0..255.  Where `lut` lives."""
    if not torch.is_tensor(lut) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError('lut_to_ycc: lut must be uint8 (256, 3)')
    if matrix not in YUV_MATRICES:
        raise ValueError("matrix must be 'bt601', 'bt709' or 'jfif', got %r" % (matrix,))
    kr, kb = (float(v) for v in NV12_MATRICES['bt601' if matrix == 'jfif' else matrix])
    ys, cs = (1.0, 1.0) if matrix == 'jfif' else (219.0 / 255.0, 224.0 / 255.0)
    R, G, B = lut.to(torch.float64).unbind(-1)
    yp = kr * R + (1.0 - kr - kb) * G + kb * B
    Y = (0.0 if matrix == 'jfif' else 16.0) + ys * yp
    Cb = 128.0 + cs * ((B - yp) / (2.0 * (1.0 - kb)))
    Cr = 128.0 + cs * ((R - yp) / (2.0 * (1.0 - kr)))
    return torch.floor(torch.stack([Y, Cb, Cr], dim=1) + 0.5).clamp_(0, 255).to(torch.uint8)


def paste_field_host(grid: Tensor, A: Tensor, rect, S: int):
    """One frame's field: grid float32 (g, g), A float64 (2, 3), rect = (y0, x0, h, w) already clamped into the frame ->
    (m float64 (h, w): the normalised map at every pixel of the rectangle, zero outside the region; inside bool (h, w)), or
    None when the map holds a non-finite entry.  Steps 1 and 2 of paste_maps_host."""
    g = int(grid.shape[0])
    if not bool(torch.isfinite(grid).all()):
        return None
    mn, mx = grid.min().to(torch.float64), grid.max().to(torch.float64)
    mhat = torch.zeros((g, g), dtype=torch.float64) if float(mx) == float(mn) else (grid.to(torch.float64) - mn) / (mx - mn)
    y0, x0, h, w = (int(v) for v in rect)
    px = (torch.arange(x0, x0 + w, dtype=torch.float64) + 0.5)[None, :]
    py = (torch.arange(y0, y0 + h, dtype=torch.float64) + 0.5)[:, None]
    a = A.to(torch.float64)
    u = (a[0, 0] * px + a[0, 1] * py) + a[0, 2]
    v = (a[1, 0] * px + a[1, 1] * py) + a[1, 2]
    inside = (u >= 0) & (u < S) & (v >= 0) & (v < S)
    r = float(g) / float(S)
    gu = torch.where(inside, u * r - 0.5, torch.zeros_like(u))
    gv = torch.where(inside, v * r - 0.5, torch.zeros_like(v))
    fx0, fy0 = torch.floor(gu), torch.floor(gv)
    fx, fy = gu - fx0, gv - fy0
    ix0, iy0 = fx0.to(torch.int64), fy0.to(torch.int64)
    ix1, iy1 = (ix0 + 1).clamp(0, g - 1), (iy0 + 1).clamp(0, g - 1)
    ix0, iy0 = ix0.clamp(0, g - 1), iy0.clamp(0, g - 1)
    m00, m01, m10, m11 = mhat[iy0, ix0], mhat[iy0, ix1], mhat[iy1, ix0], mhat[iy1, ix1]
    top = m00 + fx * (m01 - m00)                                  # horizontal pairs first, then vertical
    bot = m10 + fx * (m11 - m10)
    m = top + fy * (bot - top)
    return torch.where(inside, m, torch.zeros_like(m)), inside


def paste_maps_host(frames: Tensor, maps: Tensor, A: Tensor, rect: Tensor, lut: Tensor, alpha, S: int,
                    pixel_format: str = 'rgb24', yuv_matrix: str = 'bt709') -> Tensor:
    """The definition on the host, in float64 and int32: frames uint8 (n, Hs, Ws, 3) ('rgb24') or NV12 uint8 (n, 3 Hs / 2, Ws)
    ('nv12'), maps float32 (n, g, g) or (n, g * g), g <= 19, A float64 (n, 2, 3) and rect int32 (n, 4) as paste_geometry makes
    them, lut uint8 (256, 3) of R'G'B' colours, alpha a float or float32 (n,) -> the frames with the maps pasted on, a new
    tensor.  Per frame, over the pixels of rect clamped into the frame (NV12: aligned outward to even coordinates):

      1  mhat = (map - min) / (max - min) over the g x g cells, in float64 (a constant map: zeros; a non-finite entry in the
         map, in A or in alpha: the frame is left untouched)
      2  in the region (0 <= u < S and 0 <= v < S): gu = u (g / S) - .5, gv likewise; x = floor(gu), f = gu - x; the four cells
         (clamp(y, 0, g - 1), clamp(x, 0, g - 1)) ... (clamp(y + 1), clamp(x + 1)); a + f (b - a) along x for both rows, then
         along y: m
      3  k = clamp(floor(255 m + .5), 0, 255), w = clamp(floor((256 alpha_n) m + .5), 0, 256); outside the region w = 0
      4  'rgb24': out_c = (frame_c (256 - w) + lut[k][c] w + 128) >> 8
      5  'nv12', with lut_ycc = lut_to_ycc(lut, yuv_matrix): Y_out = (Y (256 - w) + lutY[k] w + 128) >> 8 per pixel; per 2 x 2
         block with its four (k_i, w_i): C_out = (C (1024 - sum w_i) + sum w_i lutC[k_i] + 512) >> 10 for Cb and Cr

    alpha = 0, a constant map and every byte outside the region give the input bytes."""
    if pixel_format not in ('rgb24', 'nv12'):
        raise ValueError("paste_maps_host: pixel_format must be 'rgb24' or 'nv12', got %r" % (pixel_format,))
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8:
        raise TypeError('paste_maps_host: frames must be a uint8 tensor')
    if pixel_format == 'nv12':
        if frames.dim() != 3:
            raise ValueError('paste_maps_host: NV12 frames must be (n, 3 * Hs / 2, Ws), got %s' % (tuple(frames.shape),))
        Hs, Ws = check_nv12(frames)
    else:
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError('paste_maps_host: frames must be (n, Hs, Ws, 3), got %s' % (tuple(frames.shape),))
        Hs, Ws = int(frames.shape[1]), int(frames.shape[2])
    n = int(frames.shape[0])
    maps = maps.detach().cpu()
    if maps.dtype != torch.float32 or maps.dim() not in (2, 3) or maps.shape[0] != n:
        raise ValueError('paste_maps_host: maps must be float32 (%d, g, g) or (%d, g * g), got %s %s'
                         % (n, n, maps.dtype, tuple(maps.shape)))
    g = int(maps.shape[1]) if maps.dim() == 3 else int(round(maps.shape[1] ** 0.5))
    if g < 1 or g > PASTE_MAX_GRID or maps.numel() != n * g * g:
        raise ValueError('paste_maps_host: a square grid of at most %d x %d cells expected, got %s'
                         % (PASTE_MAX_GRID, PASTE_MAX_GRID, tuple(maps.shape)))
    maps = maps.reshape(n, g, g)
    if tuple(A.shape) != (n, 2, 3) or A.dtype != torch.float64 or tuple(rect.shape) != (n, 4) or rect.dtype != torch.int32:
        raise ValueError('paste_maps_host: A float64 (%d, 2, 3) and rect int32 (%d, 4) expected' % (n, n))
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError('paste_maps_host: lut must be uint8 (256, 3)')
    al = alpha.detach().cpu().to(torch.float32) if torch.is_tensor(alpha) else torch.full((n,), float(alpha), dtype=torch.float32)
    if tuple(al.shape) != (n,):
        raise ValueError('paste_maps_host: alpha is a float or float32 (%d,)' % n)
    A, rect = A.detach().cpu(), rect.detach().cpu().to(torch.int64)
    nv = pixel_format == 'nv12'
    table = (lut_to_ycc(lut.cpu(), yuv_matrix) if nv else lut.cpu()).to(torch.int32)
    out = frames.detach().cpu().clone()
    for f in range(n):
        if not bool(torch.isfinite(A[f]).all()) or not bool(torch.isfinite(al[f])):
            continue
        y0, x0 = int(rect[f, 0].clamp(0, Hs)), int(rect[f, 1].clamp(0, Ws))
        y1, x1 = int((rect[f, 0] + rect[f, 2]).clamp(y0, Hs)), int((rect[f, 1] + rect[f, 3]).clamp(x0, Ws))
        if nv:
            y0, x0, y1, x1 = y0 - y0 % 2, x0 - x0 % 2, y1 + y1 % 2, x1 + x1 % 2
        if y1 <= y0 or x1 <= x0:
            continue
        field = paste_field_host(maps[f], A[f], (y0, x0, y1 - y0, x1 - x0), S)
        if field is None:
            continue
        m, inside = field
        k = torch.floor(255.0 * m + 0.5).to(torch.int64).clamp_(0, 255)
        w = torch.floor((256.0 * al[f].to(torch.float64)) * m + 0.5).clamp_(0, 256).to(torch.int32)
        w = torch.where(inside, w, torch.zeros_like(w))
        if not nv:
            px = out[f, y0:y1, x0:x1].to(torch.int32)
            out[f, y0:y1, x0:x1] = ((px * (256 - w)[:, :, None] + table[k] * w[:, :, None] + 128) >> 8).to(torch.uint8)
            continue
        Y = out[f, y0:y1, x0:x1].to(torch.int32)
        out[f, y0:y1, x0:x1] = ((Y * (256 - w) + table[k][:, :, 0] * w + 128) >> 8).to(torch.uint8)
        hb, wb = (y1 - y0) // 2, (x1 - x0) // 2
        sw = w.reshape(hb, 2, wb, 2).sum(dim=(1, 3))
        cy0, cy1 = Hs + y0 // 2, Hs + y1 // 2
        for c in (1, 2):
            sc = (table[k][:, :, c] * w).reshape(hb, 2, wb, 2).sum(dim=(1, 3))
            C = out[f, cy0:cy1, x0 + c - 1:x1:2].to(torch.int32)
            out[f, cy0:cy1, x0 + c - 1:x1:2] = ((C * (1024 - sw) + sc + 512) >> 10).to(torch.uint8)
    return out.to(frames.device)


# ------------------------------------------------------------------------------------------ batch draw
# DESIGN.md "Batch draw": which clips of which videos a training step takes from a JpegBank, and each clip's box, flip, JPEG
# quality and perturbation, as a pure function of (seed, step) in integer arithmetic.  BatchPlan is built and validated on the
# host once per run, batch_draw_host is the definition, and ops.batch_draw / ops.draw_clips give its tables on the device
# (csrc/batch_draw.h), where the step counter lives too: a captured graph draws a new batch on every replay.
DRAW_HEADER_INTS = 36                       # BD_HEADER_INTS of csrc/batch_draw.h: the index of a draw block starts here
DRAW_MAGIC = 0x57524442                     # 'BDRW'
DRAW_PARTS = ('videos', 'base', 'shapes', 'kinds', 'boxes', 'quality', 'view', 'perturb', 'label')     # in the block's order
DRAW_STEP_WORD, DRAW_STATUS_WORD, DRAW_DRAWN_WORD, DRAW_OFFSET_WORD = 20, 22, 24, 26
DRAW_STATUS = {1: 'the header disagrees with the call or a part leaves the block',
               2: 'a row of videos leaves the base table or is shorter than a clip'}
DRAW_PERTURB_RANGES = {'brightness': (0.6, 1.4), 'contrast': (0.6, 1.4), 'saturation': (0.0, 1.5), 'noise': (2.0, 16.0),
                       'blur': (0.5, 3.0), 'pixelate': (2, 6)}          # random_perturbations' defaults
DRAW_BLUR_ROWS = 8                          # the blur bank of random_perturbations


def _i32(v: int) -> int:
    """the 32-bit word v as the int32 that holds its bits"""
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def _threshold(p, what: str) -> int:
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:
        raise ValueError('BatchPlan: %s must be a probability in [0, 1], got %r' % (what, p))
    return int(math.floor(float(p) * 2.0 ** 32 + 0.5))


def draw_shapes(K: int = 1024, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3)) -> Tensor:
    """The shape bank of a BatchPlan, int32 (K, 2): row i holds the Q16 factors (rh, rw) by which the shorter side of a base
    box gives a box's height and width.  random_boxes' float64 formulas on a stratified set of K points (Hammersley: the area
    fraction at (i + 1/2) / K of `scale`, the aspect at the bit-reversed i, plus half a cell, of log `ratio`): h = sqrt(area /
    aspect), w = sqrt(area * aspect), so log, exp and sqrt run here and never on the device."""
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 1 << 20:
        raise ValueError('BatchPlan: the shape bank needs 1 <= K <= 2^20 rows, got %r' % (K,))
    if not (0.0 < scale[0] <= scale[1] <= 1.0) or not (0.0 < ratio[0] <= ratio[1]):
        raise ValueError('BatchPlan: need 0 < scale[0] <= scale[1] <= 1 and 0 < ratio[0] <= ratio[1], got %r %r' % (scale, ratio))
    bits = max(1, (K - 1).bit_length())
    l0, l1 = math.log(ratio[0]), math.log(ratio[1])
    rows = []
    for i in range(K):
        rev = int(format(i, '0%db' % bits)[::-1], 2)
        area = scale[0] + (scale[1] - scale[0]) * (i + 0.5) / K
        asp = math.exp(l0 + (l1 - l0) * (rev + 0.5) / (1 << bits))
        rows.append([int(math.floor(math.sqrt(area / asp) * 65536.0 + 0.5)), int(math.floor(math.sqrt(area * asp) * 65536.0 + 0.5))])
    return torch.tensor(rows, dtype=torch.int32)


def draw_block_layout(B: int, T: int, V: int, N: int, K: int, nk: int, gap: int = 0):
    """Where the parts of a draw block lie -> ({name: (offset, length)} in ints, block_ints): the header, the index at
    DRAW_HEADER_INTS, then DRAW_PARTS in order, each at the next multiple of 4 ints with `gap` more ints in front of it and
    behind the last (tests put sentinels there)."""
    n = B * T
    lengths = dict(videos=3 * V, base=4 * N, shapes=2 * K, kinds=3 * nk, boxes=4 * n, quality=n, view=3 * B, perturb=4 * B, label=B)
    parts, at = {'index': (DRAW_HEADER_INTS, n)}, DRAW_HEADER_INTS + n
    for name in DRAW_PARTS:
        at = -(-(at + gap) // 4) * 4
        parts[name] = (at, lengths[name])
        at += lengths[name]
    return parts, at + gap


class BatchPlan:
    """What a training run draws its batches from, built and validated on the host once:

    bank      a JpegBank or a PngBank (either is read through its .sizes alone), or the [(H, W)] of its places: the frames of
              the whole set, video after video
    videos    int32 (V, 3) rows (first place, frame count, label), or a list of such triples: a video is a run of consecutive
              places.  Class balance is the caller's: a video listed twice is drawn twice as often.
    T, B, stride    a clip is T frames `stride` apart, a batch B clips; a video shorter than (T - 1) * stride + 1 is refused
    base      int32 (N, 4), one (y0, x0, h, w) per place: the face box with its margin, inside its image; None: whole images
    scale, ratio, K    the shape bank (draw_shapes): the box area as a fraction of the base box's largest square, its aspect
    flip_p    the probability of a horizontal flip
    jpeg      (p, lo, hi): with probability p a clip is recompressed at a quality uniform in [lo, hi]; None: never
    perturb   (p, kinds, ranges): with probability p a clip takes one of `kinds`, uniform, at a strength uniform in the kind's
              range; ranges: {name: (low, high)} over DRAW_PERTURB_RANGES, in the units clips.perturbation takes, stored as
              the integer params of both ends.  'blur' draws a row of the 8-row bank gaussian_taps spans over its range, as
              random_perturbations does (plan.taps).  None: never.
    seed      in [0, 2^64): the Philox key of the draw, and the noise key draw_clips hands to perturb_u8.  Ranks that share a
              bank draw different batches from different seeds: fold the rank into it.
    step      where the run starts; a resumed run passes the step it stopped at, or calls seek().

    batch_draw_host(plan, step) is the draw.  on(device) uploads the plan as a draw block, once; from then on the step lives
    on the device: ops.batch_draw(plan) advances it, `step` reads it back (HostScalar: without draining the stream) and
    seek(step) writes it."""

    def __init__(self, bank, videos, T: int, B: int, stride: int = 1, base=None, scale=(0.5, 1.0), ratio=(3 / 4, 4 / 3),
                 K: int = 1024, flip_p: float = 0.5, jpeg=(0.5, 30, 95),
                 perturb=(0.5, ('brightness', 'contrast', 'saturation', 'noise', 'blur', 'pixelate'), None), seed: int = 0,
                 step: int = 0):
        sizes = list(bank.sizes if hasattr(bank, 'sizes') else bank)
        N = len(sizes)
        if N < 1 or any(len(s) != 2 or int(s[0]) < 1 or int(s[1]) < 1 for s in sizes):
            raise ValueError('BatchPlan: the bank is a JpegBank or a list of (H, W), not empty')
        for name, v in (('T', T), ('B', B), ('stride', stride)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError('BatchPlan: %s must be an int >= 1, got %r' % (name, v))
        if B * T > (2 ** 31 - 1) // 8:
            raise ValueError('BatchPlan: B * T = %d frames are too many for one draw' % (B * T))
        videos = torch.as_tensor(videos)
        if videos.dtype not in (torch.int32, torch.int64) or videos.dim() != 2 or videos.shape[1] != 3 or videos.shape[0] < 1:
            raise ValueError('BatchPlan: videos must be an integer table (V, 3) = (first place, frame count, label), V >= 1, got %s %s'
                             % (videos.dtype, tuple(videos.shape)))
        span = (T - 1) * stride + 1
        for v, (first, count, label) in enumerate(videos.tolist()):
            if first < 0 or count < 1 or first + count > N:
                raise IndexError('BatchPlan: video %d = places [%d, %d) leaves the bank of %d places' % (v, first, first + count, N))
            if count < span:
                raise ValueError('BatchPlan: video %d has %d frames, a clip of T=%d at stride %d spans %d' % (v, count, T, stride, span))
            if not -2 ** 31 <= label < 2 ** 31:
                raise ValueError('BatchPlan: the label of video %d does not fit an int32' % v)
        whole = torch.tensor([[0, 0, int(h), int(w)] for h, w in sizes], dtype=torch.int32)
        if base is None:
            base = whole
        else:
            if not torch.is_tensor(base) or base.dtype != torch.int32 or tuple(base.shape) != (N, 4):
                raise ValueError('BatchPlan: base must be int32 (%d, 4) = (y0, x0, h, w) per place of the bank' % N)
            base = base.detach().cpu().contiguous()
            bad = (base[:, 0] < 0) | (base[:, 1] < 0) | (base[:, 2] < 1) | (base[:, 3] < 1) | \
                (base[:, 0].long() + base[:, 2] > whole[:, 2]) | (base[:, 1].long() + base[:, 3] > whole[:, 3])
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                raise IndexError('BatchPlan: the base box %s of place %d lies outside its %d x %d image'
                                 % (base[i].tolist(), i, int(whole[i, 2]), int(whole[i, 3])))
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError('BatchPlan: the seed must lie in [0, 2^64), got %r' % (seed,))
        if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
            raise ValueError('BatchPlan: the step must lie in [0, 2^64), got %r' % (step,))
        self.thr_flip = _threshold(flip_p, 'flip_p')
        self.thr_jpeg, self.jpeg_lo, self.jpeg_hi = 0, 1, 1
        if jpeg is not None:
            p, lo, hi = jpeg
            self.thr_jpeg = _threshold(p, 'the p of jpeg')
            if any(isinstance(q, bool) or not isinstance(q, int) for q in (lo, hi)) or not 1 <= lo <= hi <= 100:
                raise ValueError('BatchPlan: jpeg = (p, lo, hi) needs ints 1 <= lo <= hi <= 100, got lo=%r hi=%r' % (lo, hi))
            self.jpeg_lo, self.jpeg_hi = lo, hi
        self.thr_perturb, self.taps, rows = 0, None, []
        if perturb is not None:
            p, kinds, ranges = perturb
            self.thr_perturb = _threshold(p, 'the p of perturb')
            kinds = tuple(kinds)
            if not kinds or any(k not in PERTURBATION_KINDS[1:] for k in kinds):
                raise ValueError('BatchPlan: the kinds of perturb must name some of %s, got %r' % (', '.join(PERTURBATION_KINDS[1:]), kinds))
            ranges = dict(DRAW_PERTURB_RANGES, **(ranges or {}))
            for k in kinds:
                lo, hi = ranges[k]
                if not lo <= hi:
                    raise ValueError('BatchPlan: the range of %s must be (low, high) with low <= high, got %r' % (k, ranges[k]))
                (kind, plo, _), (_, phi, _) = perturbation(k, lo), perturbation(k, hi)      # both ends are values it takes
                if k == 'blur':
                    plo, phi = 0, DRAW_BLUR_ROWS - 1
                    self.taps = gaussian_taps([lo + (hi - lo) * i / (DRAW_BLUR_ROWS - 1) for i in range(DRAW_BLUR_ROWS)])
                rows.append([kind, plo, phi])
        self.kinds = torch.tensor(rows, dtype=torch.int32).reshape(-1, 3)
        self.shapes = draw_shapes(K, scale, ratio)
        self.videos, self.base = videos.to(torch.int32).contiguous(), base
        self.T, self.B, self.stride, self.N, self.seed, self._step = T, B, stride, N, seed, step
        self.Hmax, self.Wmax = int(whole[:, 2].max()), int(whole[:, 3].max())
        self.max_side = int(base[:, 2:].max())                     # no drawn box is larger: draw_clips asks max_side <= 8 S
        self.block = self.storage = self.draw = self.taps_dev = self.parts = None

    # ---- the draw block
    def block_host(self, gap: int = 0, fill: int = 0):
        """-> (the draw block as an int32 host tensor, {name: (offset, length)}): the header and the four input tables in
        place, every other int `fill`"""
        V, K, nk = int(self.videos.shape[0]), int(self.shapes.shape[0]), int(self.kinds.shape[0])
        parts, ints = draw_block_layout(self.B, self.T, V, self.N, K, nk, gap)
        if ints > 2 ** 31 - 1:
            raise ValueError('BatchPlan: a draw block of %d ints is too large' % ints)
        block = torch.full((ints,), fill, dtype=torch.int32)
        pair = lambda v: [_i32(v), _i32(v >> 32)]
        head = [_i32(DRAW_MAGIC), ints, self.B, self.T, self.stride, V, self.N, K, nk, self.jpeg_lo, self.jpeg_hi, 0] + \
            pair(self.thr_flip) + pair(self.thr_jpeg) + pair(self.thr_perturb) + pair(self.seed) + pair(self._step) + \
            [0, 0, 0, 0] + [parts[name][0] for name in DRAW_PARTS] + [0]
        assert len(head) == DRAW_HEADER_INTS
        block[:DRAW_HEADER_INTS] = torch.tensor(head, dtype=torch.int32)
        for name in ('videos', 'base', 'shapes', 'kinds'):
            off, length = parts[name]
            block[off:off + length] = getattr(self, name).reshape(-1)
        return block, parts

    def on(self, device, gap: int = 0, tail: int = 0, fill: int = 0) -> 'BatchPlan':
        """Uploads the plan as its draw block, once (a second call is a no-op): .block the int32 device tensor, .draw its
        parts as views -- index (B*T,), boxes (B*T, 4), quality (B*T,), view (B, 3), perturb (B, 4), label (B,), status (1,),
        drawn (2,) -- and .taps_dev.  gap, tail, fill: ints left between the parts and behind the block, and what they
        hold (for tests)."""
        if self.block is not None:
            asked = torch.device(device)
            if asked.type != self.block.device.type or asked.index not in (None, self.block.device.index):
                raise RuntimeError('BatchPlan: this plan lives on %s' % self.block.device)
            return self
        host, parts = self.block_host(gap, fill)
        ints = int(host.numel())
        self.storage = torch.cat([host, torch.full((tail,), fill, dtype=torch.int32)]).to(device)
        self.block, self.parts = self.storage[:ints], parts
        n, B = self.B * self.T, self.B
        part = lambda name: self.block[parts[name][0]:parts[name][0] + parts[name][1]]
        self.draw = SimpleNamespace(
            index=part('index'), boxes=part('boxes').view(n, 4), quality=part('quality'), view=part('view').view(B, 3),
            perturb=part('perturb').view(B, 4), label=part('label'), status=self.block[DRAW_STATUS_WORD:DRAW_STATUS_WORD + 1],
            drawn=self.block[DRAW_DRAWN_WORD:DRAW_DRAWN_WORD + 2])
        self.taps_dev = None if self.taps is None else self.taps.to(device)
        return self

    @property
    def step(self) -> int:
        """the step the next draw takes: on the device once on() has run, read back without draining the stream"""
        if self.block is None:
            return self._step
        from .parallel import HostScalar
        return int(HostScalar(self.block[DRAW_STEP_WORD:DRAW_STEP_WORD + 2].view(torch.int64)).item()) & (2 ** 64 - 1)

    def seek(self, step: int) -> 'BatchPlan':
        """the next draw takes `step`: a resumed run, or a batch drawn again"""
        if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
            raise ValueError('BatchPlan: the step must lie in [0, 2^64), got %r' % (step,))
        self._step = step
        if self.block is not None:
            self.block[DRAW_STEP_WORD:DRAW_STEP_WORD + 2].copy_(torch.tensor([_i32(step), _i32(step >> 32)], dtype=torch.int32))
        return self


def batch_draw_host(plan: BatchPlan, step: int) -> SimpleNamespace:
    """The definition of ops.batch_draw: the batch of `step`, int32 host tensors -- index (B*T,) the place of the bank every
    frame is, boxes (B*T, 4), quality (B*T,), view (B, 3), perturb (B, 4), label (B,) -- in the shapes crop_resize_u8,
    jpeg_roundtrip_u8 and perturb_u8 take with checked=True.  Integer arithmetic only.  Clip b takes the twelve words w0..w11
    of philox4x32_10((step & 0xffffffff, step >> 32, b, j), (seed & 0xffffffff, seed >> 32)), j = 0, 1, 2, and with
    u(w, n) = (w * n) >> 32 and on(w, thr) = w < thr:

        video v = u(w0, V);  start = u(w1, count_v - (T - 1) * stride);  index[b, t] = first_v + start + t * stride
        label[b] = label_v;  view[b] = (0, 0, on(w2, thr_flip));  shape row k = u(w3, K)
        per frame, with the base box (by, bx, bh, bw) of its place:
            h = clamp((min(bh, bw) * rh_k + 32768) >> 16, 1, bh),  w likewise with rw_k and bw
            box = (by + u(w4, bh - h + 1), bx + u(w5, bw - w + 1), h, w)
        quality[b] = lo + u(w7, hi - lo + 1) if on(w6, thr_jpeg) else 0
        perturb[b] = (kind_i, lo_i + u(w10, hi_i - lo_i + 1), w11 & (2^30 - 1), b) with i = u(w9, nk) if on(w8, thr_perturb),
                     else (0, 0, w11 & (2^30 - 1), b)

    One draw per clip is applied to each frame's own base box, so a crop follows the face through its clip.  The tables pass
    check_boxes (for S with plan.max_side <= 8 S), check_views, check_qualities and check_perturbations by construction."""
    if isinstance(step, bool) or not isinstance(step, int) or not 0 <= step < 2 ** 64:
        raise ValueError('batch_draw_host: the step must lie in [0, 2^64), got %r' % (step,))
    B, T, stride = plan.B, plan.T, plan.stride
    b = torch.arange(B, dtype=torch.int64)
    key = (plan.seed & 0xffffffff, plan.seed >> 32)
    w = []
    for j in range(3):
        w += list(philox4x32_10((step & 0xffffffff, step >> 32, b, j), key))
    u = lambda word, n: (word * n) >> 32
    vid = plan.videos.long()[u(w[0], plan.videos.shape[0])]
    start = u(w[1], vid[:, 1] - (T - 1) * stride)
    index = (vid[:, 0] + start)[:, None] + torch.arange(T, dtype=torch.int64)[None, :] * stride
    flip = (w[2] < plan.thr_flip).long()
    shape = plan.shapes.long()[u(w[3], plan.shapes.shape[0])]
    bb = plan.base.long()[index]                                    # (B, T, 4)
    by, bx, bh, bw = bb.unbind(-1)
    m = torch.minimum(bh, bw)
    h = torch.minimum(((m * shape[:, 0:1] + 32768) >> 16).clamp(min=1), bh)
    wd = torch.minimum(((m * shape[:, 1:2] + 32768) >> 16).clamp(min=1), bw)
    boxes = torch.stack([by + u(w[4][:, None], bh - h + 1), bx + u(w[5][:, None], bw - wd + 1), h, wd], dim=-1)
    quality = torch.where(w[6] < plan.thr_jpeg, plan.jpeg_lo + u(w[7], plan.jpeg_hi - plan.jpeg_lo + 1), torch.zeros_like(b))
    perturb = torch.zeros((B, 4), dtype=torch.int64)
    perturb[:, 2], perturb[:, 3] = w[11] & (2 ** 30 - 1), b
    if plan.thr_perturb > 0:
        row = plan.kinds.long()[u(w[9], plan.kinds.shape[0])]
        hit = w[8] < plan.thr_perturb
        perturb[:, 0] = torch.where(hit, row[:, 0], torch.zeros_like(b))
        perturb[:, 1] = torch.where(hit, row[:, 1] + u(w[10], row[:, 2] - row[:, 1] + 1), torch.zeros_like(b))
    i32 = lambda t: t.to(torch.int32).contiguous()
    return SimpleNamespace(index=i32(index.reshape(-1)), boxes=i32(boxes.reshape(-1, 4)),
                           quality=i32(quality[:, None].expand(B, T).reshape(-1)),
                           view=i32(torch.stack([torch.zeros_like(flip), torch.zeros_like(flip), flip], dim=1)),
                           perturb=i32(perturb), label=i32(vid[:, 2]), step=step)


# ---- PNG files (DESIGN.md "PNG files") ---------------------------------------------------------------------------------------
# png_parse (the chunks of a file, and every refusal), png_decode_host (the definition of ops.png_decode_u8, integers only:
# zlib's inflate, or _png_inflate where zlib raises; the five row filters in numpy), png_encode_host (files for tests and
# users), png_batch (files packed for one launch) and check_png_status.  _png_inflate is RFC 1951 step by step, in the order of
# csrc/png_inflate.h: the specification the C++ decoder is compared against, and what decides a damaged stream's status.
PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
PNG_MAX_SIDE = 16384
PNG_IMAGE_INTS = 8                          # a row of PngBatch.images: ISTVT_PNG_IMAGE_INTS of include/istvt_hip.h
PNG_MAX_BYTES = 2 ** 31 - 4096              # the streams of a batch at the most: ISTVT_PNG_MAX_BYTES
PNG_BPP = {0: 1, 2: 3, 6: 4}                # bytes per pixel of the colour types the decoder takes
PNG_STATUS = {1: 'the stream ends early', 2: 'a reserved block type, or a stored block whose length and complement disagree',
              3: 'code lengths that are over-subscribed or incomplete, or a code no table holds',
              4: 'a distance beyond the bytes produced', 5: 'more, or fewer, bytes than H (1 + W bpp)',
              6: 'a filter byte above 4'}
# the status only a band-wise decode gives (png_decode_bands_host, ops.png_decode_u8 on a batch with bands); check_png_status
# words it too.  A table of its own, as JPEG_BANK_STATUS is: PNG_STATUS lists what the sequential decoder can give.
PNG_BAND_STATUS = {7: 'the band index disagrees with the stream'}
PNG_BAND_CHUNK = b'baND'                    # ancillary, private, reserved bit clear, not safe to copy: it describes the IDAT bytes
PNG_BAND_INTS = 5                           # a row of PngBatch.bands: ISTVT_PNG_BAND_INTS of include/istvt_hip.h
PNG_BAND_ALONE = 0x80000000                 # bit 31 of the R word of a baND chunk: ISTVT_PNG_BAND_ALONE of include/istvt_hip.h
# the status only a decode of bands that stand alone gives (png_decode_alone_host, ops.png_decode_u8 on a batch packed with
# alone=True, the bank's decode of an alone bank); check_png_status words it too
PNG_ALONE_STATUS = {10: "the index says its bands stand alone, and a band's first row is filtered against the row above"}
# the statuses only a windowed decode gives (png_bank_window_host, ops.png_decode_window_u8); check_png_status words them too
PNG_WINDOW_STATUS = {11: "the file's index does not say its bands stand alone: it is decoded whole, not by a box",
                     12: 'the box does not lie in the image, or its bands do not fit the window'}
_PNG_LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_PNG_LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_PNG_DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577)
_PNG_DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_PNG_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class PngHeader:
    """What png_parse reads from one file: H, W, colour_type (0 grey, 2 RGB, 6 RGBA), bpp (1, 3 or 4 bytes per pixel) and
    data, the raw DEFLATE bytes of the joined IDAT chunks without the zlib header and the Adler-32.  bands: (R, offsets) of a
    usable baND chunk (_png_band_index), else None.  alone: True where that chunk is usable and its R word carries
    PNG_BAND_ALONE, the writer's word that no band's first row is filtered against the row above (png_decode_alone_host
    checks it); bands holds R without the bit."""
    alone = False

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def raw_bytes(self) -> int:
        """the filtered rows: a filter byte and W bpp bytes per row"""
        return self.H * (1 + self.W * self.bpp)


def _png_refuse(text: str):
    raise ValueError('png_parse: ' + text)


def png_parse(data) -> PngHeader:
    """The chunks of one PNG file (bytes): the signature, IHDR, IDAT (joined), IEND; ancillary chunks are skipped, and so is a
    PLTE in a colour type 2 or 6 file (in a grey file it is refused); IDAT chunks follow one another, or the file is refused;
    every chunk's CRC-32 is checked.  Accepted: bit depth 8, no interlace, colour type 0
    (grey), 2 (RGB) or 6 (RGBA; the decoder drops alpha), sides of 1..16384, a zlib header of method 8, a window of at most
    32 KiB and no preset dictionary.  Everything else is refused by name (ValueError, 'png_parse: ...')."""
    import zlib
    data = bytes(data)
    if data[:8] != PNG_SIGNATURE:
        _png_refuse('the file does not start with the PNG signature')
    pos, ihdr, idat, ended, run, index = 8, None, [], False, False, []
    while pos < len(data):
        if pos + 12 > len(data):
            _png_refuse('a chunk header at byte %d reaches past the end of the file' % pos)
        length, kind = int.from_bytes(data[pos:pos + 4], 'big'), data[pos + 4:pos + 8]
        if pos + 12 + length > len(data):
            _png_refuse('chunk %s at byte %d reaches past the end of the file' % (kind.decode('latin-1'), pos))
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(data[pos + 4:pos + 8 + length]) != int.from_bytes(data[pos + 8 + length:pos + 12 + length], 'big'):
            _png_refuse('chunk %s at byte %d has a bad CRC-32' % (kind.decode('latin-1'), pos))
        pos += 12 + length
        if ihdr is None and kind != b'IHDR':
            _png_refuse('the first chunk is %s, not IHDR' % kind.decode('latin-1'))
        if kind == b'IHDR':
            if ihdr is not None or length != 13:
                _png_refuse('a second IHDR, or one that is not 13 bytes long')
            ihdr = body
            W, H = int.from_bytes(body[0:4], 'big'), int.from_bytes(body[4:8], 'big')
            depth, ct, comp, flt, lace = body[8:13]
            if ct not in (0, 2, 3, 4, 6) or depth not in (1, 2, 4, 8, 16):
                _png_refuse('colour type %d with bit depth %d is not a PNG image type' % (ct, depth))
            if depth == 16:
                _png_refuse('16-bit samples are not decoded (bit depth 8 only)')
            if depth < 8:
                _png_refuse('%d-bit samples are not decoded (bit depth 8 only)' % depth)
            if ct == 3:
                _png_refuse('palette images (colour type 3) are not decoded')
            if ct == 4:
                _png_refuse('grey + alpha images (colour type 4) are not decoded')
            if comp != 0 or flt != 0:
                _png_refuse('compression method %d / filter method %d are not PNG' % (comp, flt))
            if lace != 0:
                _png_refuse('Adam7 interlaced files are not decoded')
            if not (1 <= H <= PNG_MAX_SIDE and 1 <= W <= PNG_MAX_SIDE):
                _png_refuse('sides of 1..%d, got %d x %d' % (PNG_MAX_SIDE, H, W))
        elif kind == b'IDAT':
            if idat and not run:
                _png_refuse('IDAT chunks at byte %d that do not follow one another' % (pos - 12 - length))
            idat.append(body)
        elif kind == b'IEND':
            ended = True
            break
        elif kind == b'PLTE':
            if ct == 0:
                _png_refuse('a PLTE chunk in a grey file (colour type 0)')
        elif kind == PNG_BAND_CHUNK:
            index.append((body, not idat))
        elif not kind[0] & 0x20:
            _png_refuse('critical chunk %s is not known' % kind.decode('latin-1'))
        run = kind == b'IDAT'
    if ihdr is None:
        _png_refuse('the file has no IHDR')
    if not ended:
        _png_refuse('the file has no IEND')
    if not idat:
        _png_refuse('the file has no IDAT')
    z = b''.join(idat)
    if len(z) < 6 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or (z[1] & 0x20) or ((z[0] << 8) | z[1]) % 31:
        _png_refuse('a bad zlib header (method 8, a window of at most 32 KiB and no preset dictionary are taken)')
    bands, alone = _png_band_index(index, H, len(z), flag=True)
    return PngHeader(H=H, W=W, colour_type=ct, bpp=PNG_BPP[ct], data=z[2:-4], bands=bands, alone=alone)


def png_band_chunk_bytes(H: int, band_rows: int) -> int:
    """the bytes a baND chunk adds to a file: length, type and CRC-32 12, R and nb 8, nb + 1 offsets"""
    return 12 + 8 + 4 * (-(-int(H) // int(band_rows)) + 1)


def _png_band_chunk(R: int, offsets, alone: bool = False) -> bytes:
    """The band index of one file, the chunk that stands between IHDR and IDAT.  The body is big-endian uint32 words: R, the
    band rows; nb = ceil(H / R); nb + 1 offsets into the zlib stream (the joined IDAT bodies), off[0] = 2 behind the zlib
    header, off[nb] = the stream's length - 4 in front of the Adler-32.  Band k is stream bytes [off[k], off[k + 1]) and holds
    rows [k R, min(H, (k + 1) R)) with their filter bytes.  alone: the R word carries PNG_BAND_ALONE (R <= 16384, so the
    bit is free); nothing else of the chunk differs."""
    import zlib
    body = b''.join(int(v).to_bytes(4, 'big') for v in [R | (PNG_BAND_ALONE if alone else 0), len(offsets) - 1] + list(offsets))
    return len(body).to_bytes(4, 'big') + PNG_BAND_CHUNK + body + zlib.crc32(PNG_BAND_CHUNK + body).to_bytes(4, 'big')


def _png_band_index(chunks, H: int, stream_bytes: int, flag: bool = False):
    """[(body, stands before the first IDAT)] of a file's baND chunks -> (R, [off[0] .. off[nb]]), or None where the index is
    not taken: not exactly one chunk, one behind an IDAT, a length that is not 8 + 4 (nb + 1) for the nb = ceil(H / R) of its
    own R >= 1, an nb that is not that, off[0] != 2, offsets that do not increase strictly, or off[nb] != the stream's length
    - 4.  Never a refusal: the chunk is ancillary, and a decoder that ignores it is a correct one.  flag=True (png_parse):
    PNG_BAND_ALONE is taken off the R word before these checks -> ((R, offsets) or None, the bit where the index is taken);
    without it the word is R as it stands, and one with the bit matches no nb."""
    if flag:
        if len(chunks) != 1 or len(chunks[0][0]) < 4:
            return None, False
        word = int.from_bytes(chunks[0][0][:4], 'big')
        body = (word & ~PNG_BAND_ALONE).to_bytes(4, 'big') + chunks[0][0][4:]
        bands = _png_band_index([(body, chunks[0][1])], H, stream_bytes)
        return bands, bands is not None and bool(word & PNG_BAND_ALONE)
    if len(chunks) != 1 or not chunks[0][1]:
        return None
    body = chunks[0][0]
    if len(body) < 16 or len(body) % 4:
        return None
    words = [int.from_bytes(body[i:i + 4], 'big') for i in range(0, len(body), 4)]
    R, nb, off = words[0], words[1], words[2:]
    if R < 1 or nb != -(-H // R) or len(off) != nb + 1:
        return None
    if off[0] != 2 or off[-1] != stream_bytes - 4 or any(a >= b for a, b in zip(off, off[1:])):
        return None
    return R, off


class _PngBits:
    """bits of a DEFLATE stream, least significant first"""

    def __init__(self, data):
        self.data, self.pos, self.buf, self.cnt = data, 0, 0, 0

    def refill(self):
        while self.cnt <= 32 and self.pos < len(self.data):
            self.buf |= self.data[self.pos] << self.cnt
            self.cnt += 8
            self.pos += 1

    def take(self, n):
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v


def _png_code(lens, single_ok=False):
    """code lengths -> (limit[16], offset[16], symbols) of the canonical code, or None where the set is over-subscribed or
    incomplete (but for the distance code of no symbol, or of one symbol of one bit)"""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    left, used = 1, 0
    for n in range(1, 16):
        left = 2 * left - count[n]
        if left < 0:
            return None
        used += count[n]
    if left and not (single_ok and (used == 0 or (used == 1 and count[1] == 1))):
        return None
    limit, offset, code, index = [0] * 16, [0] * 16, 0, 0
    for n in range(1, 16):
        code <<= 1
        offset[n] = index - code
        code += count[n]
        index += count[n]
        limit[n] = code << (15 - n)
    return limit, offset, sorted((i for i, v in enumerate(lens) if v), key=lambda i: (lens[i], i))


def _png_symbol(bits: _PngBits, code):
    """the next symbol, or -1 (the stream ends early) / -3 (no code); the peek is padded with zeros, as the device's is"""
    limit, offset, syms = code
    c15 = int('{:015b}'.format(bits.buf & 0x7fff)[::-1], 2)
    for n in range(1, 16):
        if c15 < limit[n]:
            if n > bits.cnt:
                return -1
            bits.take(n)
            return syms[offset[n] + (c15 >> (15 - n))]
    return -3


def _png_inflate(raw, expected: int, middle: bool = False):
    """RFC 1951 on one raw stream whose output length is known -> (bytes, status 0..5 of PNG_STATUS); the first fault in stream
    order decides, and a stored block checks its complement, then the room, then the bytes it has.  middle=True is the band
    mode of png_decode_bands_host for a band that is not its file's last: `raw` is the band's bytes alone; a block header
    with BFINAL set is status 7, whatever its type; the band stops behind a stored block that ends on the last byte of
    `raw`, and then checks the count as the end of a stream does."""
    bits, out = _PngBits(bytes(raw)), bytearray()
    while True:
        bits.refill()
        if bits.cnt < 3:
            return out, 1
        last, kind = bits.take(1), bits.take(2)
        if middle and last:
            return out, 7
        if kind == 3:
            return out, 2
        if kind == 0:
            bits.take(bits.cnt & 7)
            bits.refill()
            if bits.cnt < 32:
                return out, 1
            n, c = bits.take(16), bits.take(16)
            if n ^ 0xffff != c:
                return out, 2
            if len(out) + n > expected:
                return out, 5
            if n > bits.cnt // 8 + len(bits.data) - bits.pos:
                return out, 1
            for _ in range(n):
                bits.refill()
                out.append(bits.take(8))
            if middle and bits.pos - bits.cnt // 8 == len(bits.data):
                break
        else:
            if kind == 1:
                lit, dist = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
            else:
                bits.refill()
                if bits.cnt < 14:
                    return out, 1
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if hlit > 286 or hdist > 30:
                    return out, 3
                cl = [0] * 19
                for i in range(hclen):
                    bits.refill()
                    if bits.cnt < 3:
                        return out, 1
                    cl[_PNG_CL_ORDER[i]] = bits.take(3)
                cl = _png_code(cl)
                if cl is None:
                    return out, 3
                lens = []
                while len(lens) < hlit + hdist:
                    bits.refill()
                    s = _png_symbol(bits, cl)
                    if s < 0:
                        return out, -s
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16 and not lens:
                        return out, 3
                    need, base, val = {16: (2, 3, lens[-1] if lens else 0), 17: (3, 3, 0), 18: (7, 11, 0)}[s]
                    if bits.cnt < need:
                        return out, 1
                    rep = base + bits.take(need)
                    if len(lens) + rep > hlit + hdist:
                        return out, 3
                    lens += [val] * rep
                lit, dist = lens[:hlit], lens[hlit:]
                if lit[256] == 0:
                    return out, 3
            lit, dist = _png_code(lit), _png_code(dist, single_ok=True)
            if lit is None or dist is None:
                return out, 3
            while True:
                bits.refill()
                s = _png_symbol(bits, lit)
                if s < 0:
                    return out, -s
                if s < 256:
                    if len(out) >= expected:
                        return out, 5
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    return out, 3
                if bits.cnt < _PNG_LEXT[s - 257]:
                    return out, 1
                L = _PNG_LBASE[s - 257] + bits.take(_PNG_LEXT[s - 257])
                bits.refill()
                d = _png_symbol(bits, dist)
                if d < 0:
                    return out, -d
                if d > 29:
                    return out, 3
                if bits.cnt < _PNG_DEXT[d]:
                    return out, 1
                D = _PNG_DBASE[d] + bits.take(_PNG_DEXT[d])
                if D > len(out):
                    return out, 4
                if len(out) + L > expected:
                    return out, 5
                for _ in range(L):
                    out.append(out[-D])
        if last:
            break
    return out, 0 if len(out) == expected else 5


def _png_paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _png_unfilter(rows, bpp: int):
    """rows uint8 numpy (H, 1 + W bpp): the filter byte and the filtered bytes -> the reconstructed (H, W bpp), int arithmetic
    mod 256 (PNG specification, 9.2)"""
    import numpy as np
    H, n = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((H, n), dtype=np.uint8)
    zero = np.zeros(n, dtype=np.int64)
    for y in range(H):
        ft, x = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1].astype(np.int64) if y else zero
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = x + up
        elif ft == 1:
            cur = x.copy()
            for i in range(bpp, n):
                cur[i] = (cur[i] + cur[i - bpp]) & 255
        else:
            cur = x.copy()
            for i in range(n):
                a = int(cur[i - bpp]) if i >= bpp else 0
                b = int(up[i])
                c = int(up[i - bpp]) if i >= bpp else 0
                cur[i] = (cur[i] + ((a + b) >> 1 if ft == 3 else _png_paeth(a, b, c))) & 255
        out[y] = (cur & 255).astype(np.uint8)
    return out


def png_decode_host(data, return_status: bool = False):
    """The definition of ops.png_decode_u8, integers only: one file (bytes, or a PngHeader) -> uint8 (H, W, 3), with
    return_status=True (frame, status).  png_parse; the inflate; the row filters; grey replicated to three channels, alpha
    dropped.  status: 0 fine, else PNG_STATUS, and the frame is all zeros.  The status is _png_inflate's, always: zlib is more
    lenient than RFC 1951 in one place (it takes an incomplete literal/length set whose only code is one bit long, which the
    decoders here refuse with status 3), so it never decides.  Where _png_inflate decodes a stream, zlib.decompress(raw, -15)
    must give the same bytes, and this raises if it does not."""
    import zlib

    import numpy as np
    hd = data if isinstance(data, PngHeader) else png_parse(data)
    raw, status = _png_inflate(hd.data, hd.raw_bytes)
    if status == 0:
        z = zlib.decompressobj(-15)
        if z.decompress(hd.data) != bytes(raw) or not z.eof:
            raise RuntimeError('png_decode_host: zlib and _png_inflate disagree on a stream both decode')
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(hd.H, -1) if status == 0 else None
    if status == 0 and int(rows[:, 0].max()) > 4:
        status = 6
    if status:
        out = torch.zeros((hd.H, hd.W, 3), dtype=torch.uint8)
    else:
        px = torch.from_numpy(_png_unfilter(rows, hd.bpp)).reshape(hd.H, hd.W, hd.bpp)
        out = px.expand(hd.H, hd.W, 3).contiguous() if hd.bpp == 1 else px[:, :, :3].contiguous()
    return (out, status) if return_status else out


def png_band_table(hd: PngHeader, file: int = 0, base: int = 0) -> list:
    """The bands of one parsed file as rows of PngBatch.bands: [file, first byte, end byte, first output byte within the
    file's filtered rows, output bytes], the byte positions counted from `base` + the start of hd.data.  A file without a
    usable index is one band over its whole stream."""
    if hd.bands is None:
        return [[file, base, base + len(hd.data), 0, hd.raw_bytes]]
    R, off = hd.bands
    stride = 1 + hd.W * hd.bpp
    return [[file, base + off[k] - 2, base + off[k + 1] - 2, k * R * stride, (min(hd.H, (k + 1) * R) - k * R) * stride]
            for k in range(len(off) - 1)]


def png_inflate_bands_host(hd: PngHeader):
    """-> (the filtered rows as far as they were decoded, bytearray of hd.raw_bytes; [status of every band])"""
    rows = png_band_table(hd)
    raw, statuses = bytearray(hd.raw_bytes), []
    for k, (_, begin, end, at, nbytes) in enumerate(rows):
        out, status = _png_inflate(hd.data[begin:end], nbytes, middle=k < len(rows) - 1)
        raw[at:at + len(out)] = out
        statuses.append(status)
    return raw, statuses


def png_decode_bands_host(data, return_status: bool = False):
    """The definition of ops.png_decode_u8 on a batch that carries bands, integers only: one file (bytes, or a PngHeader) ->
    uint8 (H, W, 3), with return_status=True (frame, status).  Every band of the file's index (png_parse: .bands) is decoded
    alone, by _png_inflate's rules with two changes.
      The window starts at the band's first output byte: a distance beyond the bytes THIS band has produced is status 4.  The
        output is bounded by the band's rows (1 + W bpp) bytes and the input by the band's [begin, end).
      The stop rule.  A band that is not the file's last stops when a stored block ends with the byte position equal to `end`;
        the file's last band stops at its BFINAL block, whatever its type, as the sequential decoder does.
    The order of precedence, which the device follows: the faults of a block are _png_inflate's, in its order, and the first in
    stream order decides.  In a band that is not the last, BFINAL is looked at before the block's type: a set BFINAL is status
    7 (PNG_BAND_STATUS) even on a reserved type, and nothing of that block is decoded.  Bits or bytes wanted at or past `end` are
    status 1, wherever that happens -- so a band whose last block is not a stored one ending on `end` runs into status 1 at
    the next block header, and a stored block that reaches past `end` is 1 after its complement (2) and its room (5) were
    checked.  More bytes than the band's rows hold is status 5 where the symbol or the stored block that brings them stands;
    fewer is status 5 at the stop, so of a band that stops in the right place with the wrong count 5 is the status.
    The file's status is the status of its first failing band, in band order; then 6 for a filter byte above 4, as in
    png_decode_host.  A file whose bands is None is one last band over its whole stream: the sequential decoder, the same
    bytes and the same status as png_decode_host.
    Why a file whose bands all have status 0 decodes to png_decode_host's frame: by induction over the bands.  Say the
    sequential decoder stands at byte off[k] on a byte boundary in front of a block header, with exactly the rows in front of
    band k produced (true for k = 0).  The band decoder read non-final blocks from there to a stored block that ended at
    off[k + 1]; the sequential decoder reads the same bits, for every symbol the band decoder took had all of its bits inside
    the band; every distance lay inside the band's own output, so inside the sequential window, and copied the same bytes;
    no count check fires sooner, for the file's room is no smaller than the band's; no block has BFINAL, so it goes on; behind
    the stored block it stands at off[k + 1] on a byte boundary with band k's rows produced.  The last band ends with its
    BFINAL block in both, and the counts sum to H (1 + W bpp): status 0, the same filtered rows, the same frame."""
    import numpy as np
    hd = data if isinstance(data, PngHeader) else png_parse(data)
    raw, statuses = png_inflate_bands_host(hd)
    status = next((s for s in statuses if s), 0)
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(hd.H, -1) if status == 0 else None
    if status == 0 and int(rows[:, 0].max()) > 4:
        status = 6
    if status:
        out = torch.zeros((hd.H, hd.W, 3), dtype=torch.uint8)
    else:
        px = torch.from_numpy(_png_unfilter(rows, hd.bpp)).reshape(hd.H, hd.W, hd.bpp)
        out = px.expand(hd.H, hd.W, 3).contiguous() if hd.bpp == 1 else px[:, :, :3].contiguous()
    return (out, status) if return_status else out


def _png_alone_rows(raw, statuses, H: int, W: int, bpp: int, R: int):
    """The filtered rows of a file whose index says its bands of R rows stand alone, with its band statuses -> (frame uint8
    (H, W, 3), status) by the precedence of png_decode_alone_host.  The bands are unfiltered one by one, each from a zero row."""
    import numpy as np
    status = next((s for s in statuses if s), 0)
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(H, -1) if status == 0 else None
    if status == 0 and int(rows[:, 0].max()) > 4:
        status = 6
    if status == 0 and any(int(rows[r, 0]) >= 2 for r in range(R, H, R)):
        status = 10
    if status:
        return torch.zeros((H, W, 3), dtype=torch.uint8), status
    px = np.concatenate([_png_unfilter(rows[r0:r0 + R], bpp) for r0 in range(0, H, R)], axis=0)
    px = torch.from_numpy(px).reshape(H, W, bpp)
    return (px.expand(H, W, 3).contiguous() if bpp == 1 else px[:, :, :3].contiguous()), 0


def png_decode_alone_host(data, return_status: bool = False):
    """The definition of ops.png_decode_u8 on a batch packed with alone=True, integers only: one file (bytes, or a PngHeader)
    -> uint8 (H, W, 3), with return_status=True (frame, status).  A file whose header has alone == False is
    png_decode_bands_host, bytes and status.  A file with alone == True inflates every band as png_inflate_bands_host does and
    is then unfiltered band by band, each band on its own: rows [k R, min(H, (k + 1) R)) by _png_unfilter with a zero row above
    the band's first.  Status 10 (PNG_ALONE_STATUS): a row k R, k >= 1, has filter type 2, 3 or 4 -- the file lies; row 0 may
    have any type, PNG defines it with a zero row above.  Precedence for the whole file: the inflate status of the first
    failing band in band order; then 6, a filter byte above 4 anywhere; then 10.  Any status other than 0 gives a frame of
    zeros.
    Why status 0 gives png_decode_host's frame: by induction over the bands.  png_decode_bands_host's induction gives the
    same filtered rows as the sequential inflate.  Say rows [0, k R) are reconstructed as _png_unfilter of the whole file
    reconstructs them (nothing to show for k = 0).  Row k R has type 0 or 1 (status 10 is absent; for k = 0 the row above
    is zero in both), so its reconstruction reads the row's own bytes only and is the same with a zero row above as with row
    k R - 1 above.  Every later row of the band reads its own bytes and the row above, which lies in the band and is the same
    by the step before.  So band k's rows agree, and with them rows [0, (k + 1) R)."""
    hd = data if isinstance(data, PngHeader) else png_parse(data)
    if not hd.alone:
        return png_decode_bands_host(hd, return_status)
    raw, statuses = png_inflate_bands_host(hd)
    out, status = _png_alone_rows(raw, statuses, hd.H, hd.W, hd.bpp, hd.bands[0])
    return (out, status) if return_status else out


def png_encode_host(frame, filters=None, level: int = 6, strategy: int = 0, idat: Optional[int] = None) -> bytes:
    """A PNG file of `frame`, uint8 (H, W) grey, (H, W, 3) RGB or (H, W, 4) RGBA (a tensor or an array): host only, for tests
    and users.  filters: one filter type 0..4 per row (None: 0 on every row).  zlib.compressobj(level, DEFLATED, 15, 9,
    strategy): level 0 writes stored blocks, strategy 4 (Z_FIXED) fixed ones.  idat=k splits the stream into IDAT chunks of k
    bytes."""
    import zlib

    import numpy as np
    px = np.ascontiguousarray(frame.numpy() if torch.is_tensor(frame) else frame)
    if px.dtype != np.uint8 or px.ndim not in (2, 3) or (px.ndim == 3 and px.shape[2] not in (3, 4)) or 0 in px.shape:
        raise ValueError('png_encode_host: a uint8 (H, W), (H, W, 3) or (H, W, 4) frame, got %s %s' % (px.dtype, px.shape))
    H, W = px.shape[:2]
    bpp = 1 if px.ndim == 2 else px.shape[2]
    ct = {1: 0, 3: 2, 4: 6}[bpp]
    filters = [0] * H if filters is None else [int(v) for v in filters]
    if len(filters) != H or any(not 0 <= v <= 4 for v in filters):
        raise ValueError('png_encode_host: filters holds one type 0..4 per row (%d rows)' % H)
    cur = px.reshape(H, W * bpp).astype(np.int64)
    a = np.concatenate([np.zeros((H, bpp), np.int64), cur[:, :-bpp]], axis=1) if W > 1 else np.zeros_like(cur)
    b = np.concatenate([np.zeros((1, W * bpp), np.int64), cur[:-1]], axis=0)
    c = np.concatenate([np.zeros((H, bpp), np.int64), b[:, :-bpp]], axis=1) if W > 1 else np.zeros_like(cur)
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = np.stack([np.zeros_like(cur), a, b, (a + b) >> 1, paeth])
    ft = np.array(filters, dtype=np.int64)
    rows = np.empty((H, 1 + W * bpp), dtype=np.uint8)
    rows[:, 0] = ft
    rows[:, 1:] = ((cur - pred[ft, np.arange(H)]) & 255).astype(np.uint8)
    z = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    stream = z.compress(rows.tobytes()) + z.flush()
    return png_wrap(H, W, ct, stream, idat)


def png_wrap(H: int, W: int, colour_type: int, stream: bytes, idat: Optional[int] = None, extra: bytes = b'') -> bytes:
    """the file of a zlib stream (header, DEFLATE bytes, Adler-32): signature, IHDR, `extra` (whole chunks, as they are),
    IDAT chunks of `idat` bytes (None: one), IEND"""
    import zlib

    def chunk(kind, body):
        return len(body).to_bytes(4, 'big') + kind + body + zlib.crc32(kind + body).to_bytes(4, 'big')
    k = len(stream) if idat is None else int(idat)
    if k < 1:
        raise ValueError('png_wrap: idat is a chunk size of at least 1 byte')
    head = W.to_bytes(4, 'big') + H.to_bytes(4, 'big') + bytes([8, colour_type, 0, 0, 0])
    return (PNG_SIGNATURE + chunk(b'IHDR', head) + extra + b''.join(chunk(b'IDAT', stream[i:i + k]) for i in range(0, len(stream), k))
            + chunk(b'IEND', b''))


class PngBatch:
    """Files packed for one launch of ops.png_decode_u8 (png_batch makes it): host tensors, pinned where a device is there to
    take them.  data uint8: the raw DEFLATE streams end to end, each starting at a multiple of 16 bytes | images int32 (n, 8):
    H, W, colour type, bpp, begin, end, 0, 0 | sizes: [(H, W)] | raw_stride: the largest H (1 + W bpp) of the batch, rounded up
    to 16 | raw_bytes: the filtered bytes of all files.  bands: None, or with png_batch(bands='index') int32 (nband, 5), the
    bands of all files sorted by file, then by band: file, first byte in data, end byte, first output byte within the file's
    filtered rows, output bytes; images[:, 6:8] are then a file's first row of `bands` and its count of them.  alone: None, or
    with png_batch(bands='index', alone=True) int32 (n,): 1 where the file's header says its bands stand alone, else 0; such a
    batch is decoded by istvt_png_decode_alone_u8, the flagged files one wave per band in the unfilter too."""

    def __init__(self, **kw):
        self.bands = None
        self.alone = None
        self.__dict__.update(kw)
        self._on = {}

    @property
    def scratch_bytes(self) -> int:
        """what a launch needs: a row of raw_stride bytes per file for its filtered rows; with bands, behind them a status
        word per band"""
        return self.n * self.raw_stride + (0 if self.bands is None else 4 * int(self.bands.shape[0]))

    def on(self, device):
        """.data and .images (and .bands, where the batch has them) on `device`: uploaded once, without blocking, on the
        stream that is current at the first call"""
        key = str(device)
        if key not in self._on:
            names = ('data', 'images') + (() if self.bands is None else ('bands',)) + (() if self.alone is None else ('alone',))
            self._on[key] = SimpleNamespace(**{k: getattr(self, k).to(device, non_blocking=True) for k in names})
        return self._on[key]


def check_png_bands(bands, who: str = 'png_batch'):
    """None (the sequential decoder) or 'index' (one wave per band of every file's baND chunk); anything else is refused"""
    if bands is None or bands == 'index':
        return bands
    raise ValueError("%s: bands is None or 'index', got %r" % (who, bands))


def png_batch(files, bands=None, alone: bool = False) -> PngBatch:
    """A sequence of PNG files (bytes, or PngHeaders) -> the PngBatch of one launch.  Every file goes through png_parse, so a
    file the decoder does not take is refused here, before anything is uploaded.  bands='index': the batch carries the band
    table of the files' baND chunks (png_band_table), one band for a file without a usable chunk, and ops.png_decode_u8
    decodes it one wave per band; bands=None: the batch of the sequential decoder, whatever chunks the files have.
    alone=True (needs bands='index'): the batch carries .alone, every file's flag, and the files whose index says their bands
    stand alone are unfiltered one wave per band as well (png_decode_alone_host); a file without the flag is decoded as
    without the keyword.  Without alone=True the flag is not looked at: the serial unfilter gives the right pixels either way."""
    check_png_bands(bands)
    if not isinstance(alone, bool):
        raise ValueError('png_batch: alone is True or False, got %r' % (alone,))
    if alone and bands != 'index':
        raise ValueError("png_batch: alone=True needs bands='index' (the flag lives in the band index)")
    files = list(files)
    if not files:
        raise ValueError('png_batch: an empty batch')
    parts, images, sizes, nbytes, stride, raw, table, flags = [], [], [], 0, 16, 0, [], []
    for f in files:
        hd = f if isinstance(f, PngHeader) else png_parse(f)
        images.append([hd.H, hd.W, hd.colour_type, hd.bpp, nbytes, nbytes + len(hd.data), 0, 0])
        flags.append(int(bool(hd.alone)))
        if bands is not None:
            rows = png_band_table(hd, len(images) - 1, nbytes)
            images[-1][6:8] = [len(table), len(rows)]
            table += rows
        pad = -len(hd.data) % 16
        parts.append(hd.data + bytes(pad))
        nbytes += len(hd.data) + pad
        sizes.append((hd.H, hd.W))
        stride = max(stride, -(-hd.raw_bytes // 16) * 16)
        raw += hd.raw_bytes
    if nbytes > PNG_MAX_BYTES:
        raise ValueError('png_batch: the streams of a batch hold at most %d bytes, got %d' % (PNG_MAX_BYTES, nbytes))
    pin = torch.cuda.is_available()

    def host(t):
        return t.pin_memory() if pin and t.numel() else t
    data = torch.frombuffer(bytearray(b''.join(parts) or bytes(16)), dtype=torch.uint8)
    return PngBatch(data=host(data), nbytes=nbytes, images=host(torch.tensor(images, dtype=torch.int32)), sizes=sizes,
                    n=len(files), raw_stride=stride, raw_bytes=raw, alone=host(torch.tensor(flags, dtype=torch.int32)) if alone else None,
                    bands=None if bands is None else host(torch.tensor(table, dtype=torch.int32).reshape(-1, PNG_BAND_INTS)))


def check_png_status(status) -> None:
    """reads the status table of ops.png_decode_u8 back (this waits for the device) and raises for the first damaged file"""
    for i, s in enumerate(status.detach().cpu().tolist()):
        if s != 0:
            raise ValueError('png_decode: file %d is damaged (status %d: %s)'
                             % (i, s, PNG_STATUS.get(s) or PNG_BAND_STATUS.get(s) or PNG_BANK_STATUS.get(s)
                                or PNG_ALONE_STATUS.get(s) or PNG_WINDOW_STATUS.get(s, 'unknown')))


# ---- PNG bank (DESIGN.md "PNG bank") --------------------------------------------------------------------------------------------
# The files of a whole set packed once for ops.png_decode_bank_u8, which decodes those a device index names.  A file is
# addressed by a 64-bit base into the bank's bytes and everything inside it by 32-bit offsets from that base, so a bank is not
# bound by 2^31 bytes; csrc/png_bank.h is the same arithmetic in C++.  png_bank_decode_host is the definition, computed from
# the bank's own rows and bytes.
PNG_BANK_IMAGE_INTS = 10                    # a row of PngBank.images: ISTVT_PNG_BANK_IMAGE_INTS of include/istvt_hip.h
# the statuses only a bank's decode gives (png_bank_decode_host, ops.png_decode_bank_u8); check_png_status words them too
PNG_BANK_STATUS = {8: 'the index is outside the bank', 9: "the bank's row for this place, or one of its band rows, does not fit the call"}


class PngBank:
    """A set of PNG files ready for ops.png_decode_bank_u8 (png_bank makes it): host tensors, pinned where a device is there to
    take them.  data uint8: the raw DEFLATE streams end to end, each starting at a multiple of 16 bytes | images int32 (n, 10):
    H, W, colour type, bpp, base low word, base high word, stream bytes, first band row, band count, flags (bit 0 in a bank
    packed with alone=True: the file's bands stand alone; else 0); the base is the 64-bit
    byte offset of the file's stream on the device, first_byte included, and a multiple of 16 | bands int32 (nband, 5), rows
    of png_band_table sorted by file, then by band, with begin and end counted from the file's base | sizes: [(H, W)] | n,
    nband | nbytes: the streams' bytes with their padding, a Python int that may exceed 2^31 | Hmax, Wmax | raw_stride: the
    largest H (1 + W bpp), rounded up to 16 | band_max: the most bands of any file | first_byte: where the first stream
    starts on the device | headers: the parsed files | alone: True for png_bank(alone=True), whose decode unfilters the
    flagged files one wave per band (istvt_png_decode_bank_alone_u8)."""

    def __init__(self, **kw):
        self.device = None                                        # ops.png_decode_bank_u8 reads it as it does a JpegBank's
        self.alone = False
        self.__dict__.update(kw)
        self._on = {}

    def __len__(self) -> int:
        return self.n

    def on(self, device):
        """.data .images .bands on `device`, uploaded once without blocking: .data is torch.empty of first_byte + nbytes bytes
        with the streams copied behind first_byte; the bytes in front are never written and never read"""
        key = str(device)
        if key not in self._on:
            data = torch.empty((self.first_byte + self.nbytes,), dtype=torch.uint8, device=device)
            data[self.first_byte:].copy_(self.data, non_blocking=True)
            self._on[key] = SimpleNamespace(data=data, images=self.images.to(device, non_blocking=True),
                                            segments=self.bands.to(device, non_blocking=True))
            self._on[key].bands = self._on[key].segments           # the band table goes where segments do
        return self._on[key]


def png_bank(files, bands='index', first_byte: int = 0, alone: bool = False) -> PngBank:
    """A sequence of PNG files (bytes, or PngHeaders) -> the PngBank of the set, on the host.  Every file goes through
    png_parse, which refuses what the decoder does not take.  bands='index' (the default): a file's bands are those of its
    baND chunk where png_parse accepts it, and a file without a usable chunk is one band; bands=None: every file is one band.
    first_byte (a multiple of 16, for tests): the first stream starts there on the device, and the bytes in front are
    allocated and never read.  A single stream of PNG_MAX_BYTES or more is refused; the set as a whole has no such bound.
    alone=True (needs bands='index'): bit 0 of images[:, 9] is the file's flag (PngHeader.alone), and the bank's decode
    unfilters the flagged files one wave per band; a file without the flag is decoded as in any other bank."""
    check_png_bands(bands, 'png_bank')
    if not isinstance(alone, bool):
        raise ValueError('png_bank: alone is True or False, got %r' % (alone,))
    if alone and bands != 'index':
        raise ValueError("png_bank: alone=True needs bands='index' (the flag lives in the band index)")
    if isinstance(first_byte, bool) or not isinstance(first_byte, int) or first_byte < 0 or first_byte % 16:
        raise ValueError('png_bank: first_byte is a multiple of 16 and not negative, got %r' % (first_byte,))
    if isinstance(files, (bytes, bytearray)) or not hasattr(files, '__len__'):
        raise TypeError('png_bank expects a sequence of files (bytes), got %s' % type(files).__name__)
    if len(files) == 0:
        raise ValueError('png_bank: an empty bank')
    headers = [f if isinstance(f, PngHeader) else png_parse(f) for f in files]
    parts, images, table, nbytes, stride, band_max = [], [], [], 0, 16, 1
    for i, hd in enumerate(headers):
        if len(hd.data) >= PNG_MAX_BYTES:
            raise ValueError('png_bank: the stream of file %d holds %d bytes; one file holds fewer than %d (offsets inside a '
                             'file are int32)' % (i, len(hd.data), PNG_MAX_BYTES))
        one = hd if bands == 'index' or hd.bands is None else PngHeader(H=hd.H, W=hd.W, colour_type=hd.colour_type, bpp=hd.bpp,
                                                                         data=hd.data, bands=None)
        rows = png_band_table(one, i, 0)
        base = first_byte + nbytes
        images.append([hd.H, hd.W, hd.colour_type, hd.bpp, base & 0xffffffff, base >> 32, len(hd.data), len(table), len(rows),
                       int(alone and bool(hd.alone))])
        table += rows
        band_max = max(band_max, len(rows))
        pad = -len(hd.data) % 16
        parts.append(hd.data + bytes(pad))
        nbytes += len(hd.data) + pad
        stride = max(stride, -(-hd.raw_bytes // 16) * 16)
    pin = torch.cuda.is_available()

    def host(t):
        return t.pin_memory() if pin and t.numel() else t
    words = torch.tensor(images, dtype=torch.int64)
    words[:, 4:6] = (words[:, 4:6] + 2 ** 31) % 2 ** 32 - 2 ** 31   # the two words of the base as int32 holds them
    data = torch.frombuffer(bytearray(b''.join(parts) or bytes(16)), dtype=torch.uint8)
    return PngBank(data=host(data), nbytes=int(data.numel()), images=host(words.to(torch.int32)),
                   bands=host(torch.tensor(table, dtype=torch.int32).reshape(-1, PNG_BAND_INTS)),
                   sizes=[(hd.H, hd.W) for hd in headers], n=len(headers), nband=len(table), Hmax=max(hd.H for hd in headers),
                   Wmax=max(hd.W for hd in headers), raw_stride=stride, band_max=band_max, first_byte=first_byte, headers=headers,
                   alone=alone)


def png_bank_scratch_bytes(bank: PngBank, m: int) -> int:
    """The scratch of ops.png_decode_bank_u8 for m places: a row of raw_stride bytes per place for its filtered rows, then an
    int32 status per band, band_max of them per place"""
    m = int(m)
    return m * bank.raw_stride + 4 * m * bank.band_max


def _png_alone_band_rows(H: int, stride: int, rows) -> int:
    """The band rows of a file that says its bands stand alone -> R, the rows of a band, where they are the R-row bands of an
    index, else 0 (pa_alone_rows and pa_band_row_fits of csrc/png_alone.h): R = out_bytes of band row 0 / stride, a whole
    number of at least 1; count == ceil(H / R); band k writes out == k R stride and out_bytes == rows_k stride.  A row that
    is not inside the table (None) fails."""
    if not rows or rows[0] is None or rows[0][4] < stride or rows[0][4] % stride:
        return 0
    R = rows[0][4] // stride
    if len(rows) != -(-H // R):
        return 0
    for k, row in enumerate(rows):
        if row is None or row[3] != k * R * stride or row[4] != (min(H, (k + 1) * R) - k * R) * stride:
            return 0
    return R


def _png_bank_place(bank: PngBank, i: int, Hc: int, Wc: int):
    """Place i of the bank from its own rows and bytes, as csrc/png_bank.h reads them -> (frame uint8 (H, W, 3) or None, H, W,
    status).  Status 9 and no frame where the image row or a band row does not fit the bank."""
    import numpy as np
    im = bank.images[i].tolist()
    H, W, ct, bpp, lo, hi, nstream, first, count = im[:9]
    alone = bool(bank.alone and im[9] & 1)
    base = ((hi & 0xffffffff) << 32) | (lo & 0xffffffff)
    if base >= 2 ** 63:
        base -= 2 ** 64
    total = bank.first_byte + bank.nbytes
    if not (1 <= H <= PNG_MAX_SIDE and 1 <= W <= PNG_MAX_SIDE and H <= Hc and W <= Wc) or PNG_BPP.get(ct) != bpp \
            or H * (1 + W * bpp) > bank.raw_stride or not (1 <= count <= bank.band_max) or base < 0 or base % 16 or nstream < 0 \
            or base > total or nstream > total - base or base < bank.first_byte:
        return None, 0, 0, 9
    stream = bytes(bank.data[base - bank.first_byte:base - bank.first_byte + nstream].numpy())
    raw, statuses = bytearray(H * (1 + W * bpp)), []
    for k in range(count):
        if first < 0 or first + k >= bank.nband:
            statuses.append(9)
            continue
        f, begin, end, at, nout = bank.bands[first + k].tolist()
        if f != i or not (0 <= begin <= end <= nstream) or at < 0 or nout < 0 or at + nout > len(raw):
            statuses.append(9)
            continue
        out, status = _png_inflate(stream[begin:end], nout, middle=k < count - 1)
        raw[at:at + len(out)] = out
        statuses.append(status)
    if alone:
        R = _png_alone_band_rows(H, 1 + W * bpp, [bank.bands[first + k].tolist() if 0 <= first and first + k < bank.nband else None
                                                  for k in range(count)])
        if R == 0:
            return None, 0, 0, 9
        frame, status = _png_alone_rows(raw, statuses, H, W, bpp, R)
        return (None, 0, 0, 9) if status == 9 else (frame, H, W, status)
    status = next((s for s in statuses if s), 0)
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(H, -1) if status == 0 else None
    if status == 0 and int(rows[:, 0].max()) > 4:
        status = 6
    if status:
        return torch.zeros((H, W, 3), dtype=torch.uint8), H, W, status
    px = torch.from_numpy(_png_unfilter(rows, bpp)).reshape(H, W, bpp)
    return (px.expand(H, W, 3).contiguous() if bpp == 1 else px[:, :, :3].contiguous()), H, W, 0


def png_bank_decode_host(bank_or_files, index, canvas=None):
    """The definition of ops.png_decode_bank_u8, integers only: -> (frames, sizes, status), frames uint8 (m, Hc, Wc, 3) with
    place j holding png_decode_bands_host(files[index[j]]) in its top left corner and 0 elsewhere, sizes int32 (m, 2) =
    (H, W), status int32 (m,).  Computed from the bank's own rows and bytes (a sequence of files is packed by png_bank
    first), so it says what the tables mean: a file packed as one band gives png_decode_host's result.  Beside the statuses of
    png_decode_bands_host: 8 where index[j] is outside [0, n), 9 where the bank's row for the place or one of its band rows
    does not fit (PNG_BANK_STATUS); both with size (0, 0) and a frame of zeros.  canvas = (Hc, Wc) defaults to the bank's
    Hmax x Wmax, whatever is drawn.  A bank packed with alone=True places png_decode_alone_host for its flagged files: status
    10 (PNG_ALONE_STATUS) keeps the file's size and zeroes the frame, like statuses 1 to 7; a flagged file whose band rows
    are not the R-row bands of an index (_png_alone_band_rows) is status 9."""
    bank = bank_or_files if isinstance(bank_or_files, PngBank) else png_bank(bank_or_files)
    index = check_bank_index(index, 'png_bank_decode_host').tolist()
    Hc, Wc = (bank.Hmax, bank.Wmax) if canvas is None else (int(canvas[0]), int(canvas[1]))
    if Hc < bank.Hmax or Wc < bank.Wmax:
        raise ValueError('png_bank_decode_host: the canvas %d x %d does not hold every image of the bank' % (Hc, Wc))
    drawn = {i: _png_bank_place(bank, i, Hc, Wc) for i in set(index) if 0 <= i < bank.n}
    frames = torch.zeros((len(index), Hc, Wc, 3), dtype=torch.uint8)
    sizes = torch.zeros((len(index), 2), dtype=torch.int32)
    status = torch.zeros((len(index),), dtype=torch.int32)
    for j, i in enumerate(index):
        if i not in drawn:
            status[j] = 8
            continue
        f, H, W, s = drawn[i]
        status[j] = s
        if s != 9:
            frames[j, :H, :W] = f
            sizes[j, 0], sizes[j, 1] = H, W
    return frames, sizes, status


# ---- PNG windows (DESIGN.md "PNG windows") ------------------------------------------------------------------------------------
# A face box needs a fraction of a whole frame's rows.  Of a file whose bands stand alone, ops.png_decode_window_u8 inflates and
# unfilters only the bands the box touches, into a canvas that is a window of `rows` rows, and hands the crop the box moved into
# that window.  png_window_plan is the window, png_bank_window_host the definition; csrc/png_window.h is the same arithmetic in
# C++ for the device and for tools/png_window_check.cpp.
def png_window_plan(H: int, R: int, count: int, box, rows: int, win_bands: int, W: Optional[int] = None):
    """The window of box (y0, x0, h, w) in a file of H rows in `count` bands of R rows that stand alone -> (kfirst, klast, w0,
    w1), or status 12 (PNG_WINDOW_STATUS).  kfirst = y0 // R and klast = (y0 + h - 1) // R are the bands the box touches; w0 =
    kfirst R and w1 = min(H, (klast + 1) R) the rows they hold.  12: h < 1, w < 1, y0 < 0, x0 < 0, y0 + h > H, x0 + w > W
    (looked at where W is given), w1 - w0 > rows, or more than win_bands bands.  The one place these steps are written in
    Python; pw_window of csrc/png_window.h is the same in C++."""
    y0, x0, h, w = (int(v) for v in box)
    if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or (W is not None and x0 + w > W):
        return 12
    kfirst, klast = y0 // R, (y0 + h - 1) // R
    w0, w1 = kfirst * R, min(H, (klast + 1) * R)
    if klast >= count or w1 - w0 > rows or klast - kfirst + 1 > win_bands:
        return 12
    return kfirst, klast, w0, w1


def _png_window_files(src) -> list:
    """[(H, W, bpp, R, count, flagged)] of a PngBank's or a PngBatch's files from its own tables; R is 0 for a file without the
    flag.  Kept with the tensors it was read from, so that a decode step after step does not read the tables again and an
    object given other tables is read anew."""
    if not isinstance(src, (PngBank, PngBatch)):
        raise TypeError('a clips.PngBank or a clips.PngBatch is expected, got %s' % type(src).__name__)
    kept = src.__dict__.get('_window_files')
    if kept is None or kept[0] is not src.images or kept[1] is not src.bands or kept[2] is not src.alone:
        src._window_files = kept = (src.images, src.bands, src.alone, _png_window_files_read(src))
    return kept[3]


def _png_window_files_read(src) -> list:
    if src.bands is None:
        return [(r[0], r[1], r[3], 0, 1, False) for r in src.images.tolist()]
    bands, out = src.bands.tolist(), []
    bank = isinstance(src, PngBank)
    flags = src.images[:, 9].tolist() if bank else [0] * src.n if src.alone is None else src.alone.tolist()
    for r, flag in zip(src.images.tolist(), flags):
        first, count = (r[7], r[8]) if bank else (r[6], r[7])
        flagged = bool(flag & 1) and (not bank or bool(src.alone))
        out.append((r[0], r[1], r[3], bands[first][4] // (1 + r[1] * r[3]) if flagged else 0, count, flagged))
    return out


def png_window_rows(bank_or_batch, h_max: int) -> int:
    """The window height `rows` that fits any box of height at most h_max in any flagged file of a PngBank or a PngBatch: the
    largest of min(H_i, R_i (1 + (h_max + R_i - 2) // R_i)).  A box of height h at y0 = k R + a, 0 <= a < R, touches bands k to
    (k R + a + h - 1) // R = k + (a + h - 1) // R, so 1 + (a + h - 1) // R bands: most for a = R - 1, the box that starts in a
    band's last row, which touches 1 + (h + R - 2) // R bands, and for h = h_max.  Their rows are R each, and never more than
    the image has.  1 where no file is flagged."""
    h_max = int(h_max)
    if h_max < 1:
        raise ValueError('png_window_rows: h_max is at least 1, got %d' % h_max)
    return max([min(H, R * (1 + (h_max + R - 2) // R)) for H, _, _, R, _, flagged in _png_window_files(bank_or_batch) if flagged] or [1])


def png_window_bands(bank_or_batch, rows: int) -> int:
    """win_bands for a window of `rows` rows, the slots a place gets: the largest min(count_i, ceil(rows / R_i)) over the flagged
    files; 1 where none is"""
    rows = int(rows)
    return max([min(count, -(-rows // R)) for _, _, _, R, count, flagged in _png_window_files(bank_or_batch) if flagged] or [1])


def png_window_stride(bank_or_batch, rows: int) -> int:
    """win_stride, the bytes of a place's filtered rows in the scratch: rows * the largest 1 + W_i bpp_i, rounded up to 16"""
    return -(-int(rows) * max(1 + W * bpp for _, W, bpp, _, _, _ in _png_window_files(bank_or_batch)) // 16) * 16


def png_window_scratch_bytes(bank_or_batch, m: int, rows: int) -> int:
    """The scratch of ops.png_decode_window_u8 for m places: m * win_stride bytes of filtered rows, an int32 status per slot
    (m * win_bands), then from the next multiple of 16 the moved boxes int32 (m, 4) and the origins int32 (m,)"""
    return png_window_boxes_at(bank_or_batch, m, rows) + 4 * int(m) * 5


def png_window_boxes_at(bank_or_batch, m: int, rows: int) -> int:
    """Where the moved boxes stand in that scratch, in bytes (pw_boxes_at of csrc/png_window.h): behind the filtered rows and
    the status words, at the next multiple of 16; the m origins follow the 4 m words of the boxes"""
    m = int(m)
    at = m * png_window_stride(bank_or_batch, rows) + 4 * m * png_window_bands(bank_or_batch, rows)
    return -(-at // 16) * 16


def _png_window_place(bank: PngBank, i: int, box, rows: int, Wc: int, win_bands: int, win_stride: int, inflated: dict):
    """Place i of the bank through `box`, from the bank's own rows and bytes as csrc/png_window.h reads them -> (window uint8
    (w1 - w0, W, 3) or None, H, W, status, origin, moved box).  inflated: {(i, k): (bytes, status)}, the bands inflated so far."""
    import numpy as np
    none = lambda H, W, status: (None, H, W, status, 0, (0, 0, 1, 1))
    im = bank.images[i].tolist()
    H, W, ct, bpp, lo, hi, nstream, first, count = im[:9]
    base = ((hi & 0xffffffff) << 32) | (lo & 0xffffffff)
    if base >= 2 ** 63:
        base -= 2 ** 64
    total = bank.first_byte + bank.nbytes
    if not (1 <= H <= PNG_MAX_SIDE and 1 <= W <= PNG_MAX_SIDE and W <= Wc) or PNG_BPP.get(ct) != bpp \
            or H * (1 + W * bpp) > bank.raw_stride or not (1 <= count <= bank.band_max) or base < 0 or base % 16 or nstream < 0 \
            or base > total or nstream > total - base or base < bank.first_byte:
        return none(0, 0, 9)
    stride = 1 + W * bpp
    if min(H, rows) * stride > win_stride:
        return none(0, 0, 9)
    if not (bank.alone and im[9] & 1):
        return none(H, W, 11)
    if first < 0 or first + count > bank.nband:
        return none(0, 0, 9)
    table = [bank.bands[first + k].tolist() for k in range(count)]
    R = _png_alone_band_rows(H, stride, table)
    if R == 0:
        return none(0, 0, 9)
    plan = png_window_plan(H, R, count, box, rows, win_bands, W)
    if plan == 12:
        return none(H, W, 12)
    kfirst, klast, w0, w1 = plan
    raw, statuses = bytearray((w1 - w0) * stride), []
    for k in range(kfirst, klast + 1):
        f, begin, end, at, nout = table[k]
        if f != i or not (0 <= begin <= end <= nstream):
            statuses.append(9)
            continue
        if (i, k) not in inflated:
            stream = bytes(bank.data[base - bank.first_byte + begin:base - bank.first_byte + end].numpy())
            inflated[(i, k)] = _png_inflate(stream, nout, middle=k < count - 1)
        out, status = inflated[(i, k)]
        raw[at - w0 * stride:at - w0 * stride + len(out)] = out
        statuses.append(status)
    status = next((s for s in statuses if s), 0)
    if status == 9:
        return none(0, 0, 9)
    filt = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(w1 - w0, stride)
    if status == 0 and int(filt[:, 0].max()) > 4:
        status = 6
    if status == 0 and any(int(filt[r - w0, 0]) >= 2 for r in range(w0, w1) if r > 0 and r % R == 0):
        status = 10
    if status:
        return none(H, W, status)
    px = np.concatenate([_png_unfilter(filt[r0 - w0:min(r0 + R, w1) - w0], bpp) for r0 in range(w0, w1, R)], axis=0)
    px = torch.from_numpy(px).reshape(w1 - w0, W, bpp)
    y0, x0, h, w = (int(v) for v in box)
    return (px.expand(w1 - w0, W, 3).contiguous() if bpp == 1 else px[:, :, :3].contiguous()), H, W, 0, w0, (y0 - w0, x0, h, w)


def png_bank_window_host(bank_or_files, index, boxes, rows: int, Wc: Optional[int] = None):
    """The definition of ops.png_decode_window_u8, integers only: place j is files[index[j]] through boxes[j] = (y0, x0, h, w)
    -> (windows uint8 (m, rows, Wc, 3), sizes int32 (m, 2), status int32 (m,), origin int32 (m,), moved_boxes int32 (m, 4)).
    bank_or_files: a PngBank packed with alone=True, or a sequence of files, which png_bank(files, alone=True) packs.  Wc
    defaults to the bank's Wmax.  Of a file of H rows whose index says its count bands of R rows stand alone only the bands
    the box touches are inflated and unfiltered (png_window_plan): rows [w0, w1) of the image stand in rows [0, w1 - w0) and
    columns [0, W) of the place's window and everything else of it is zero; origin is w0 and the moved box (y0 - w0, x0, h, w).
    The status of a place, by precedence:
      8   index[j] is outside the bank;
      9   the bank's row does not fit the call (as png_bank_decode_host decides it, but that the file's H is not compared with
          `rows`: its W is compared with Wc, and min(H, rows) of its filtered rows with the bytes a place has in the scratch);
      11  the file's index does not say its bands stand alone (PNG_WINDOW_STATUS): such a file is decoded whole, not by a box;
      9   the band rows of a flagged file are not the R-row bands of an index (_png_alone_band_rows);
      12  the box does not lie in the image, or its bands do not fit the window (png_window_plan, with win_bands =
          png_window_bands(bank, rows));
      then the status of the first failing TOUCHED band in band order: its inflate's, or 9 for a band row that does not name the
          file or lies outside its stream;
      6   a filter byte above 4 in a touched row;
      10  a touched row k R, k >= 1, of type 2, 3 or 4 -- the first row of the window's own first band where kfirst >= 1.
    Any status but 0 leaves a window of zeros, origin 0 and the moved box (0, 0, 1, 1), so that the crop behind it is black;
    sizes are (H, W), or (0, 0) with 8 and 9.
    A deliberate difference from png_decode_alone_host: damage in a band the box does not touch is not seen.  A flipped bit, a
    filter byte 5 or a lying first row in a band outside [kfirst, klast] leaves status 0 and the right pixels here, where the
    whole decode gives the file's status and zeros.
    Why status 0 gives the crop of the whole frame.  The touched bands inflated to the filtered rows the sequential inflate has
    (png_decode_bands_host's induction, band by band).  No touched row k R, k >= 1, has type 2, 3 or 4 (status 10 is absent), and
    row 0 is defined with a zero row above: so no touched band's first row reads the row above it, and unfiltering each touched
    band from a zero row gives rows [w0, w1) of png_decode_host (png_decode_alone_host's induction, started at kfirst in place
    of 0).  The box lies inside rows [w0, w1) and columns [0, W), and crop_resize_host reads src[y0:y0 + h, x0:x0 + w] and
    nothing else: crop_resize_host(window, moved_box) is crop_resize_host(whole frame, box), byte for byte."""
    bank = bank_or_files if isinstance(bank_or_files, PngBank) else png_bank(bank_or_files, alone=True)
    index = check_bank_index(index, 'png_bank_window_host').tolist()
    boxes = [[int(v) for v in b] for b in (boxes.tolist() if torch.is_tensor(boxes) else boxes)]
    rows = int(rows)
    Wc = bank.Wmax if Wc is None else int(Wc)
    if len(boxes) != len(index) or any(len(b) != 4 for b in boxes):
        raise ValueError('png_bank_window_host: one box (y0, x0, h, w) per place, %d of them' % len(index))
    if not (1 <= rows <= PNG_MAX_SIDE and 1 <= Wc <= PNG_MAX_SIDE):
        raise ValueError('png_bank_window_host: rows and Wc lie in 1..%d, got %d and %d' % (PNG_MAX_SIDE, rows, Wc))
    win_bands, win_stride = png_window_bands(bank, rows), png_window_stride(bank, rows)
    m, inflated = len(index), {}
    windows = torch.zeros((m, rows, Wc, 3), dtype=torch.uint8)
    sizes, status = torch.zeros((m, 2), dtype=torch.int32), torch.zeros((m,), dtype=torch.int32)
    origin, moved = torch.zeros((m,), dtype=torch.int32), torch.tensor([[0, 0, 1, 1]] * m, dtype=torch.int32)
    for j, i in enumerate(index):
        if not 0 <= i < bank.n:
            status[j] = 8
            continue
        win, H, W, s, w0, box = _png_window_place(bank, i, boxes[j], rows, Wc, win_bands, win_stride, inflated)
        status[j], origin[j] = s, w0
        sizes[j, 0], sizes[j, 1] = H, W
        moved[j] = torch.tensor(box, dtype=torch.int32)
        if win is not None:
            windows[j, :win.shape[0], :W] = win
    return windows, sizes, status, origin, moved


def png_decode_window_host(data, box, rows: Optional[int] = None, Wc: Optional[int] = None, return_status: bool = False):
    """One file (bytes, or a PngHeader) through one box (y0, x0, h, w) -> (window uint8 (rows, Wc, 3), origin, moved_box), with
    return_status=True (window, origin, moved_box, status): png_bank_window_host of the file alone, which has the statuses,
    their precedence and the argument.  rows defaults to the window the box needs, w1 - w0 of png_window_plan (1 where the box
    has none), Wc to the file's W."""
    hd = data if isinstance(data, PngHeader) else png_parse(data)
    bank = png_bank([hd], alone=True)
    if rows is None:
        plan = png_window_plan(hd.H, hd.bands[0], len(hd.bands[1]) - 1, box, hd.H, PNG_MAX_SIDE, hd.W) if hd.alone else 12
        rows = 1 if plan == 12 else plan[3] - plan[2]
    windows, _, status, origin, moved = png_bank_window_host(bank, [0], [box], rows, Wc)
    out = (windows[0], int(origin[0]), tuple(moved[0].tolist()))
    return out + (int(status[0]),) if return_status else out


def check_png_window(src, boxes, index=None, rows: Optional[int] = None, canvas_w: Optional[int] = None,
                     who: str = 'png_decode_window_u8'):
    """What ops.png_decode_window_u8 refuses by name before a device is asked for -> (boxes, rows, Wc).  src: a PngBatch packed
    with png_batch(bands='index', alone=True) whose files all carry the flag, or a PngBank packed with png_bank(alone=True).
    boxes: int32 (m, 4) = (y0, x0, h, w), one per place (a list is made one).  Where the boxes and, for a bank, the index are
    on the host, every box of a flagged file is looked at: it lies in its image, and its window (png_window_plan) has at most
    `rows` rows, or with rows=None `rows` becomes the smallest that fits them all.  Boxes or an index on the device are not
    read: a bank then needs `rows`, and a batch takes its tallest image.  rows and canvas_w (default: the widest image) lie
    in 1..16384."""
    if isinstance(src, PngBatch):
        if src.alone is None:
            raise ValueError("%s: the batch was not packed with alone=True (clips.png_batch(files, bands='index', alone=True)): only "
                             'bands that stand alone are decoded by a box' % who)
        flags = src.alone.tolist()
        if 0 in flags:
            raise ValueError("%s: file %d of the batch does not say its bands stand alone (ops.png_encode_u8(alone=True) and "
                             'clips.png_encode_banded_host(index=True, alone=True) write files that do)' % (who, flags.index(0)))
        if index is not None:
            raise ValueError('%s: index= goes with a clips.PngBank' % who)
        which, Wmax = list(range(src.n)), max(w for _, w in src.sizes)
    elif isinstance(src, PngBank):
        if not src.alone:
            raise ValueError('%s: the bank was not packed with alone=True (clips.png_bank(files, alone=True)): only bands that '
                             'stand alone are decoded by a box' % who)
        if index is None:
            raise ValueError('%s: a clips.PngBank is decoded through index=' % who)
        index = check_bank_index(index, who)
        which, Wmax = None if index.is_cuda else index.tolist(), src.Wmax
    else:
        raise TypeError('%s expects a clips.PngBatch or a clips.PngBank packed with alone=True, got %s' % (who, type(src).__name__))
    m = src.n if index is None else int(index.numel())
    if not torch.is_tensor(boxes):
        boxes = torch.tensor(boxes, dtype=torch.int32).reshape(-1, 4)
    if boxes.dtype != torch.int32 or tuple(boxes.shape) != (m, 4):
        raise ValueError('%s: boxes are int32 (%d, 4) = (y0, x0, h, w), one per place, got %s %s' % (who, m, boxes.dtype, tuple(boxes.shape)))
    for name, v in (('rows', rows), ('canvas_w', canvas_w)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= PNG_MAX_SIDE):
            raise ValueError('%s: %s lies in 1..%d, got %r' % (who, name, PNG_MAX_SIDE, v))
    Wc = Wmax if canvas_w is None else canvas_w
    if Wc < Wmax:
        raise ValueError('%s: canvas_w holds the widest image (%d), got %d' % (who, Wmax, Wc))
    if boxes.is_cuda or which is None:
        if rows is None and isinstance(src, PngBank):
            raise ValueError('%s: boxes or an index on the device are not read here: say rows= (clips.png_window_rows(bank, h_max) '
                             'fits any box of height at most h_max)' % who)
        return boxes, (max(h for h, _ in src.sizes) if rows is None else rows), Wc
    files, need = _png_window_files(src), 1
    for j, (i, box) in enumerate(zip(which, boxes.tolist())):
        if not 0 <= i < src.n or not files[i][5]:
            continue
        H, W, _, R, count, _ = files[i]
        plan = png_window_plan(H, R, count, box, H, count, W)
        if plan == 12:
            raise IndexError('%s: box %d, (y0, x0, h, w) = %s, does not lie in its image of %d x %d' % (who, j, tuple(box), H, W))
        if rows is not None and plan[3] - plan[2] > rows:
            raise ValueError('%s: box %d, (y0, x0, h, w) = %s, needs a window of %d rows (its bands of %d rows), rows is %d'
                             % (who, j, tuple(box), plan[3] - plan[2], R, rows))
        need = max(need, plan[3] - plan[2])
    return boxes, (need if rows is None else rows), Wc


# ---- PNG files out (DESIGN.md "PNG files out") ---------------------------------------------------------------------------------
# png_encode_banded_host is the definition of ops.png_encode_u8, byte for byte: row filters chosen from the source pixels, bands
# of band_rows rows coded on their own (one dynamic-Huffman block and an empty stored block each, so every band starts and ends
# on a byte), literals and matches at distance 1 only.  csrc/png_deflate.h is the same steps in C++ for the device and for
# tools/png_deflate_check.cpp.
PNG_ENCODE_STATUS = {1: 'the file does not fit in data: offsets[n] is the capacity a retry needs'}
PNG_BAND_HEADER_BITS = 17 + 3 * 19 + 7 * 287    # BFINAL, BTYPE, HLIT, HDIST, HCLEN; 19 lengths of 3 bits; 286 + 1 lengths of <= 7 bits
PNG_CONTAINER_BYTES = 57 + 6                # signature 8, IHDR 25, IDAT 12, IEND 12; the zlib header 2 and the Adler-32 4


def _png_code_lengths(counts, limit: int) -> list:
    """Counts -> the code length of every symbol (0 where the count is 0), at most `limit` bits, a complete set where two or
    more symbols have a count.  The rule, fixed so that two programs make the same table:
      1. merge the two smallest live counts until one is left; of equal counts the larger symbol is the smaller one; the
         first pick c1 keeps the sum and c2's chain of symbols is hung behind c1's; every symbol of both chains gets one bit
         more (libjpeg's jpeg_gen_optimal_table without its reserved symbol);
      2. bits[l] = how many symbols have length l; for i from the longest length down to limit + 1, while bits[i] > 0: take
         the largest j < i - 1 with bits[j] > 0 and do bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1 (ITU T.81
         K.2, which keeps the Kraft sum at 1);
      3. the symbols sorted by (length of step 1, symbol) take the lengths of bits[] in ascending order.
    One live symbol gets length 1 (an incomplete code; no band makes one)."""
    n = len(counts)
    live = [s for s in range(n) if counts[s]]
    lens = [0] * n
    if len(live) < 2:
        for s in live:
            lens[s] = 1
        return lens
    freq, others, size = list(counts), [-1] * n, [0] * n
    while True:
        c1, v = -1, None
        for s in live:
            if freq[s] and (v is None or freq[s] <= v):
                v, c1 = freq[s], s
        c2, v = -1, None
        for s in live:
            if freq[s] and s != c1 and (v is None or freq[s] <= v):
                v, c2 = freq[s], s
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        for c in (c1, c2):
            size[c] += 1
            while others[c] >= 0:
                c = others[c]
                size[c] += 1
        c = c1                                 # the chain of c2 goes behind the chain of c1
        while others[c] >= 0:
            c = others[c]
        others[c] = c2
    bits = [0] * (n + 2)
    for s in live:
        bits[size[s]] += 1
    for i in range(n, limit, -1):
        while bits[i] > 0:
            j = i - 2
            while j > 0 and bits[j] == 0:
                j -= 1
            if j == 0:
                raise ValueError('_png_code_lengths: %d symbols do not fit in %d bits' % (len(live), limit))
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    order = sorted(live, key=lambda s: (size[s], s))
    at = 0
    for l in range(1, min(limit, n) + 1):
        for _ in range(bits[l]):
            lens[order[at]] = l
            at += 1
    return lens


def _png_canonical(lens) -> list:
    """RFC 1951 3.2.2: lengths -> the code of every symbol, most significant bit first"""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    codes = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            codes[s] = nxt[v]
            nxt[v] += 1
    return codes


def _png_band_tokens(band) -> list:
    """The tokens of one band's bytes (rows with their filter bytes, one sequence): a literal is its byte 0..255, a match of
    length L at distance 1 is -L.  Per maximal run of n equal bytes: its first byte is a literal; of the other m = n - 1, m //
    258 matches of 258, then one match of m % 258 where that is at least 3, else that many literals."""
    out, i, n = [], 0, len(band)
    while i < n:
        j = i
        while j < n and band[j] == band[i]:
            j += 1
        m = j - i - 1
        out.append(band[i])
        out += [-258] * (m // 258)
        r = m % 258
        out += [-r] if r >= 3 else [band[i]] * r
        i = j
    return out


def _png_length_symbol(L: int):
    """a match length 3..258 -> (symbol 257..285, extra bits, their count); 258 is symbol 285"""
    k = 28
    while _PNG_LBASE[k] > L:
        k -= 1
    return 257 + k, L - _PNG_LBASE[k], _PNG_LEXT[k]


def _png_length_tokens(lens) -> list:
    """The lengths of a block's two codes, one sequence, as code-length symbols [(symbol, extra, extra bits)], greedy from the
    left.  A run of r zeros: 18 with min(r, 138) while r >= 11, then 17 with r where r >= 3, else r times 0.  A run of r equal
    lengths v > 0: v once, then 16 with min(rest, 6) while the rest is >= 3, then the rest (0..2) as v."""
    out, i, n = [], 0, len(lens)
    while i < n:
        j = i
        while j < n and lens[j] == lens[i]:
            j += 1
        v, r = lens[i], j - i
        if v == 0:
            while r >= 11:
                k = min(r, 138)
                out.append((18, k - 11, 7))
                r -= k
            if r >= 3:
                out.append((17, r - 3, 3))
                r = 0
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3, 2))
                r -= k
        out += [(v, 0, 0)] * r
        i = j
    return out


class _PngBitsOut:
    """bits of a DEFLATE stream, least significant first; a Huffman code goes in most significant bit first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v: int, k: int):
        self.acc |= v << self.n
        self.n += k

    def code(self, c: int, k: int):
        self.put(int('{:0{}b}'.format(c, k)[::-1], 2) if k else 0, k)

    def bytes(self) -> bytes:
        return self.acc.to_bytes(-(-self.n // 8), 'little')


def _png_band_tables(tokens):
    """tokens -> (literal/length lengths [286], HLIT, code-length tokens, code-length code's lengths [19], HCLEN)"""
    counts = [0] * 286
    for t in tokens:
        counts[t if t >= 0 else _png_length_symbol(-t)[0]] += 1
    counts[256] = 1
    lit = _png_code_lengths(counts, 15)
    hlit = max(i for i in range(286) if lit[i]) + 1             # >= 257: the end-of-block has a code
    cltok = _png_length_tokens(lit[:hlit] + [1])                # and the distance code: symbol 0, one bit
    clcounts = [0] * 19
    for s, _, _ in cltok:
        clcounts[s] += 1
    cl = _png_code_lengths(clcounts, 7)
    hclen = max(4, max(i for i in range(19) if cl[_PNG_CL_ORDER[i]]) + 1)
    return lit, hlit, cltok, cl, hclen


def _png_encode_band(band, final: bool) -> bytes:
    """one band: a dynamic-Huffman block (BFINAL = 0) and an empty stored block, which carries BFINAL on the last band"""
    tokens = _png_band_tokens(band)
    lit, hlit, cltok, cl, hclen = _png_band_tables(tokens)
    if _png_code(lit) is None or _png_code(cl) is None:
        raise RuntimeError('png_encode_banded_host: an incomplete code')
    w = _PngBitsOut()
    w.put(0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl[_PNG_CL_ORDER[i]], 3)
    clcode, litcode = _png_canonical(cl), _png_canonical(lit)
    for s, extra, k in cltok:
        w.code(clcode[s], cl[s])
        w.put(extra, k)
    for t in tokens:
        if t >= 0:
            w.code(litcode[t], lit[t])
        else:
            s, extra, k = _png_length_symbol(-t)
            w.code(litcode[s], lit[s])
            w.put(extra, k)
            w.put(0, 1)                                           # distance 1: code 0 of one bit
    w.code(litcode[256], lit[256])
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.put(0, -w.n % 8)
    return w.bytes() + b'\x00\x00\xff\xff'


def _png_frame(frame, who: str):
    import numpy as np
    px = np.ascontiguousarray(frame.detach().cpu().numpy() if torch.is_tensor(frame) else frame)
    if px.ndim == 3 and px.shape[2] == 1:
        px = px[:, :, 0]
    if px.dtype != np.uint8 or px.ndim not in (2, 3) or (px.ndim == 3 and px.shape[2] not in (3, 4)) or 0 in px.shape:
        raise ValueError('%s: a uint8 (H, W), (H, W, 1), (H, W, 3) or (H, W, 4) frame, got %s %s' % (who, px.dtype, px.shape))
    if px.shape[0] > PNG_MAX_SIDE or px.shape[1] > PNG_MAX_SIDE:
        raise ValueError('%s: sides of at most %d, got %d x %d' % (who, PNG_MAX_SIDE, px.shape[0], px.shape[1]))
    return px, (1 if px.ndim == 2 else px.shape[2])


def check_png_filters(filters, who: str = 'png_encode_banded_host') -> int:
    """'adaptive' -> 5, a fixed type 0..4 -> itself; anything else is refused"""
    if filters == 'adaptive':
        return 5
    if isinstance(filters, int) and not isinstance(filters, bool) and 0 <= filters <= 4:
        return int(filters)
    raise ValueError("%s: filters is 'adaptive' or one type 0..4 for every row, got %r" % (who, filters))


def check_png_band_rows(band_rows, who: str = 'png_encode_banded_host') -> int:
    if isinstance(band_rows, bool) or not isinstance(band_rows, int) or band_rows < 1:
        raise ValueError('%s: band_rows is a count of rows of at least 1, got %r' % (who, band_rows))
    return min(int(band_rows), PNG_MAX_SIDE)


def png_filter_rows_host(frame, filters='adaptive', alone_rows=None):
    """frame -> the filtered rows uint8 (H, 1 + W bpp) with their filter bytes.  The predictors are png_encode_host's: a and c
    are zero at the row's start, b and c on the image's first row, and the row above is the source's.  'adaptive': per row the
    type whose residuals r have the smallest sum of min(r, 256 - r); of equal sums the lowest type.
    alone_rows = R: every row r with r % R == 0, row 0 included, is restricted to the types that do not read the row above.
    'adaptive' takes the cheaper of 0 and 1 by the same cost, of equal sums 0; a fixed 0 or 1 stays; a fixed 2 becomes 0 (Up
    against a zero row is None); a fixed 3 or 4 becomes 1 (Paeth with b = c = 0 is Sub; Average has no equal, Sub is the
    choice).  Every other row is byte for byte what it is without alone_rows: a row's filtered bytes depend on the source
    rows only."""
    import numpy as np
    px, bpp = _png_frame(frame, 'png_encode_banded_host')
    mode = check_png_filters(filters)
    if alone_rows is not None:
        alone_rows = check_png_band_rows(alone_rows)
    H, W = px.shape[:2]
    cur = px.reshape(H, W * bpp).astype(np.int64)
    a = np.concatenate([np.zeros((H, bpp), np.int64), cur[:, :-bpp]], axis=1) if W > 1 else np.zeros_like(cur)
    b = np.concatenate([np.zeros((1, W * bpp), np.int64), cur[:-1]], axis=0)
    c = np.concatenate([np.zeros((H, bpp), np.int64), b[:, :-bpp]], axis=1) if W > 1 else np.zeros_like(cur)
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = (cur[None] - np.stack([np.zeros_like(cur), a, b, (a + b) >> 1, paeth])) & 255
    if mode == 5:
        ft = np.argmin(np.minimum(res, 256 - res).sum(axis=2), axis=0)
    else:
        ft = np.full(H, mode, dtype=np.int64)
    if alone_rows is not None:
        first = np.arange(0, H, alone_rows)
        if mode == 5:
            ft[first] = np.argmin(np.minimum(res[:2, first], 256 - res[:2, first]).sum(axis=2), axis=0)
        else:
            ft[first] = (0, 1, 0, 1, 1)[mode]
    rows = np.empty((H, 1 + W * bpp), dtype=np.uint8)
    rows[:, 0] = ft
    rows[:, 1:] = res[ft, np.arange(H)].astype(np.uint8)
    return rows


def _check_png_alone(alone, index, who: str) -> bool:
    if not isinstance(alone, bool):
        raise ValueError('%s: alone is True or False, got %r' % (who, alone))
    if alone and not index:
        raise ValueError('%s: alone=True needs index=True (the flag lives in the band index)' % who)
    return alone


def png_encode_banded_host(frame, band_rows: int = 16, filters='adaptive', return_bands: bool = False, index: bool = False,
                           alone: bool = False):
    """The definition of ops.png_encode_u8, integers only: frame uint8 (H, W) / (H, W, 1) grey, (H, W, 3) RGB or (H, W, 4) RGBA
    -> a complete PNG file: signature, IHDR, one IDAT, IEND.  Rows [k R, min(H, (k + 1) R)) with their filter bytes
    (png_filter_rows_host) are band k, R = band_rows, coded on its own by _png_encode_band: tokens by _png_band_tokens, both
    code tables by _png_code_lengths (15 and 7 bits), the lengths sent by _png_length_tokens, HLIT and HCLEN trimmed of
    trailing zeros, HDIST = 0 with one distance code of one bit, canonical codes, then an empty stored block (000 or, on the
    last band, 100; zeros to the byte; 00 00 FF FF).  So every band starts and ends on a byte and refers to no byte outside
    itself.  The stream is 78 01, the bands, the Adler-32 of the filtered rows.  return_bands=True: (file, [(begin, end)] of
    every band in the stream, whose first band begins at 2, the filter type of every row).  index=True (the definition of
    ops.png_encode_u8(index=True)): the file carries the bands' offsets in a baND chunk (_png_band_chunk, with R =
    min(band_rows, H)) between IHDR and IDAT, for a decoder that takes the bands apart; every other byte is the same.
    alone=True (the definition of ops.png_encode_u8(alone=True); needs index=True): every band's first row is filtered without
    the row above (png_filter_rows_host(alone_rows=R)) and the chunk's R word carries PNG_BAND_ALONE, so a band decodes to
    pixels with no other band (png_decode_alone_host)."""
    import zlib
    if not isinstance(index, bool):
        raise ValueError('png_encode_banded_host: index is True or False, got %r' % (index,))
    _check_png_alone(alone, index, 'png_encode_banded_host')
    R = check_png_band_rows(band_rows)
    rows = png_filter_rows_host(frame, filters, R if alone else None)
    H, bpp = rows.shape[0], _png_frame(frame, 'png_encode_banded_host')[1]
    W = (rows.shape[1] - 1) // bpp
    stream, bands = bytearray(b'\x78\x01'), []
    for r0 in range(0, H, R):
        part = _png_encode_band(rows[r0:r0 + R].tobytes(), r0 + R >= H)
        bands.append((len(stream), len(stream) + len(part)))
        stream += part
    stream += zlib.adler32(rows.tobytes()).to_bytes(4, 'big')
    extra = _png_band_chunk(min(R, H), [b for b, _ in bands] + [bands[-1][1]], alone) if index else b''
    data = png_wrap(H, W, {1: 0, 3: 2, 4: 6}[bpp], bytes(stream), extra=extra)
    return (data, bands, rows[:, 0].tolist()) if return_bands else data


def png_encode_files_host(frames, band_rows: int = 16, filters='adaptive', index: bool = False, alone: bool = False) -> list:
    """the files of a batch: frames uint8 (n, H, W), (n, H, W, 1 | 3 | 4) or clips (B, T, H, W, C) -> [bytes], one
    png_encode_banded_host each"""
    import numpy as np
    px = np.asarray(frames.detach().cpu().numpy() if torch.is_tensor(frames) else frames)
    if px.ndim == 5:
        px = px.reshape((-1,) + px.shape[2:])
    if px.ndim not in (3, 4):
        raise ValueError('png_encode_files_host: frames (n, H, W), (n, H, W, C) or (B, T, H, W, C), got %s' % (px.shape,))
    return [png_encode_banded_host(f, band_rows, filters, index=index, alone=alone) for f in px]


def png_encoded_bound(H: int, W: int, bpp: int, band_rows: int = 16, index: bool = False, alone: bool = False) -> int:
    """The bytes one file of png_encode_banded_host needs at the most.  A band of nb bytes (rows (1 + W bpp)) is at most nb
    tokens and the end-of-block.  The code `256 literals of 9 bits, the end-of-block and the 29 length symbols of 6` is a
    prefix code (256 / 512 + 30 / 64 < 1), and under it a literal costs 9 bits and a match 6 + 5 extra + 1 distance = 12 for
    at least 3 bytes, so a band's tokens cost at most 9 nb bits and the end-of-block at most 15; a Huffman code costs no more
    than any prefix code.  (The covering code is not the issue's sketch, 255 literals of 8 bits and two symbols of 9, which
    has no room for the length symbols the tokens use.)  The limit of 15 bits only acts where a code would be longer, which
    takes counts that grow like 1, 1, 2, 3, 5, ... (2584 bytes at least); the adjustment that shortens such a code is not
    an optimal one, so for those bands the 9 bits are measured (tests/test_png_encode_cpu.py: far inside), not proven.
    Nothing rests on it but the default capacity: the kernels check the capacity themselves and report status 1.  The block
    header is at most PNG_BAND_HEADER_BITS = 17
    + 19 * 3 + 287 * 7 bits.  The empty stored block is 3 bits, the pad to the byte and 4 bytes.  Bands of a file: ceil(H /
    R).  The container is 57 + 6 bytes; index=True adds the baND chunk's png_band_chunk_bytes(H, R).  alone=True (needs
    index=True) changes filter types only: the indexed bound, unchanged."""
    _check_png_alone(alone, index, 'png_encoded_bound')
    H, W, bpp, R = int(H), int(W), int(bpp), check_png_band_rows(band_rows, 'png_encoded_bound')
    stride, total = 1 + W * bpp, PNG_CONTAINER_BYTES + (png_band_chunk_bytes(H, R) if index else 0)
    for r0 in range(0, H, R):
        nb = (min(H, r0 + R) - r0) * stride
        total += -(-(PNG_BAND_HEADER_BITS + 9 * nb + 15 + 3) // 8) + 4
    return total


class PngFiles(_EncodedFiles):
    """What ops.png_encode_u8 hands back, on the device, with JpegFiles' semantics: data uint8 (capacity,): the files end to
    end | offsets int64 (n + 1,): file i is data[offsets[i]:offsets[i + 1]] | status int32 (n,): 0 fine, 1 as
    PNG_ENCODE_STATUS words it (files() hands b'' over for it with check=False).  geometry: H, W, bpp, band_rows, filters,
    index, alone."""
    _name, _who, _status, _empty = 'PngFiles', 'png_encode', PNG_ENCODE_STATUS, (1,)
