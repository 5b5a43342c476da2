"""Relevance maps of ISTVT: gradient-weighted attention rollout (Chefer, Gur, Wolf, ICCV 2021, "Generic Attention-model
Explainability"), the interpretable half of the reference (visualize_rel.py:206-294) on the HIP path.

    res = istvt_amd.explain.relevance(model, clips, index=0)      # or model.relevance(clips)
    maps = istvt_amd.explain.heatmaps(res.cam_s, scale=16)        # (B, T, g*16, g*16), min-max normalised per map
    ex = model.explain_video(frames)                              # a whole video: video.VideoScorer.explain
    shown = istvt_amd.explain.overlay(frames, ex.frame_s)         # (N, g*16, g*16, 3) uint8, the maps on the frames

Definition (DESIGN.md "Relevance maps"): y = sum_b logits[b, index]; per layer and head A = softmax output, G = dy/dA;
Abar_l = (1/H) sum_h max(0, A_{l,h} * G_{l,h}); r = e_0, r <- r + r Abar_l for l = L-1 .. 0, one spatial rollout per
(clip, frame) over tokens and one temporal rollout per (clip, position) over frames.  No row normalisation (the 2021b
"generic" rule, not the LRP rules of the reference's `tfe` package).

The call leaves the model as it found it: eval mode for the call (BatchNorm statistics do not move), the stem under
no_grad, a backward pass to the token input only, no parameter gradient computed (p.grad, the fused bucket and any
data-parallel hook see nothing), eager even when step graphs are on (the graph cache is not touched), fp8 attention
operands off (the recomputed probabilities must match the forward's statistics), and every flag restored in a
``finally``.
"""
from __future__ import annotations

import contextlib

import torch

from . import frames as byte_frames
from . import functional as Fn
from . import ops


class Relevance:
    """cam_s, cam_t (B, T, P-1): the per-frame spatial and temporal maps (the reference's cam_s and cam_t after its
    transpose(0, 1), visualize_rel.py:259); r_s (B, F, P), r_t (B, P, F): the raw rollouts; logits (B, num_classes)."""
    __slots__ = ('cam_s', 'cam_t', 'r_s', 'r_t', 'logits')

    def __init__(self, r_s, r_t, logits):
        self.r_s, self.r_t, self.logits = r_s, r_t, logits
        self.cam_s = r_s[:, 1:, 1:]                           # cam_s[b, t, n-1] = r_s[b, t+1, n]
        self.cam_t = r_t[:, 1:, 1:].transpose(1, 2)           # cam_t[b, t, n-1] = r_t[b, n, t+1]

    def __repr__(self):
        return 'Relevance(cam_s=%s, cam_t=%s)' % (tuple(self.cam_s.shape), tuple(self.cam_t.shape))


def _attention_modules(model):
    from .network.vivit.module import SpatialOnlyAttention
    return [m for m in model.modules() if isinstance(m, SpatialOnlyAttention)]


@contextlib.contextmanager
def _explaining(model):
    """eval mode, fp8 attention operands off and every parameter frozen for the call; all restored afterwards"""
    modes = [(m, m.training) for m in model.modules()]
    fp8 = [(m, m.attn_fp8) for m in _attention_modules(model)]
    req = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for m, _ in modes:
            m.training = False
        for m, _ in fp8:
            m.attn_fp8 = False
        for p, _ in req:
            p.requires_grad_(False)
        yield
    finally:
        for p, on in req:
            p.requires_grad_(on)
        for m, on in fp8:
            m.attn_fp8 = on
        for m, on in modes:
            m.training = on


def _rollouts_tokens(dsttr, x, b, f, p, index):
    """x: the assembled tokens (b, f*p, dim) of b clips -> Relevance; the caller has put the model in _explaining"""
    x = x.detach().requires_grad_(True)                       # the backward pass ends at the tokens
    rel = Fn.RelevanceContext(b, f, p, x.device)
    with torch.enable_grad(), Fn.relevance_mode(rel):
        logits = dsttr.forward_tokens(x, b, f, p)
        if not 0 <= index < logits.shape[1]:
            raise IndexError('relevance: index %d out of range for %d outputs' % (index, logits.shape[1]))
        y = logits[:, index].sum()                            # inside enable_grad: VideoScorer.explain calls under no_grad
    torch.autograd.grad(y, x)
    return Relevance(rel.r_s.view(b, f, p), rel.r_t.view(b, p, f), logits.detach())


def _rollouts(dsttr, feats, index):
    """feats (b, t, hw, c) -> Relevance; the caller has put the model in _explaining"""
    if feats.dim() != 4:
        raise RuntimeError('relevance: features must be (b, t, h*w, c), got %s' % (tuple(feats.shape),))
    b, t, hw, _ = feats.shape
    with torch.no_grad():
        x = Fn.TokensFn.apply(ops.cast(feats, dsttr.compute_dtype), dsttr.space_token, dsttr.temporal_token,
                              dsttr.pos_embedding)
    return _rollouts_tokens(dsttr, x, b, t + 1, hw + 1, index)


def relevance_features(dsttr, feats, index=0) -> Relevance:
    """Relevance maps of a DSTTr from its input features (b, t, h*w, c)."""
    with _explaining(dsttr):
        return _rollouts(dsttr, feats, index)


def relevance(model, x, index=0) -> Relevance:
    """Relevance maps of an XceptionVidTr for the clips x (b, t, 3, S, S) and output `index` (a DSTTr takes its features
    (b, t, h*w, c) instead, as relevance_features)."""
    from .network.vivit.vivit import DSTTr, XceptionVidTr
    if isinstance(model, DSTTr):
        return relevance_features(model, x, index)
    if not isinstance(model, XceptionVidTr):
        raise TypeError('relevance: expected an XceptionVidTr or a DSTTr, got %s' % type(model).__name__)
    with _explaining(model):
        b, t = x.shape[:2]
        with torch.no_grad():
            feats = model.xcep.model.low_level_features_nhwc(x.flatten(0, 1), model.compute_dtype)
        n, h, w, c = feats.shape
        return _rollouts(model.vit, feats.view(b, t, h * w, c), index)


def heatmaps(cam, scale: int = 16):
    """The reference's post-processing of one map (visualize_rel.py:262-265) for every map at once: bilinear upsampling
    by `scale` (align_corners=False) and (x - min) / (max - min) per map.  cam: (B, T, g, g), or (B, T, g*g) as
    Relevance.cam_s / cam_t hold it -> (B, T, g*scale, g*scale) float32."""
    if cam.dim() == 3:
        g = _grid(cam, 'heatmaps')
        cam = cam.reshape(*cam.shape[:-1], g, g)
    return ops.relevance_heatmap(cam, scale)


def _grid(cam, what):
    g = int(round(cam.shape[-1] ** 0.5))
    if g * g != cam.shape[-1]:
        raise RuntimeError('%s: %d tokens per map is not a square grid' % (what, cam.shape[-1]))
    return g


def jet_lut(device=None):
    """The default colour table of overlay(): (256, 3) uint8, a closed-form piecewise-linear jet.  Entry i of the channel
    with centre c is round(255 * clip(1.5 - |4 i / 255 - 4 c|, 0, 1)), c = 0.75, 0.5, 0.25 for red, green, blue (columns
    0, 1, 2).  It is NOT pinned to OpenCV's COLORMAP_JET (a sampled table that differs from this formula by a few levels
    in places), and its channel order is RGB where the reference's cv2 frames are BGR: the order of `lut`'s columns and
    of the frames' channels is the caller's."""
    i = torch.arange(256, dtype=torch.float64).view(256, 1)
    c = torch.tensor([0.75, 0.5, 0.25], dtype=torch.float64).view(1, 3)
    lut = torch.round(255 * (1.5 - (4 * i / 255 - 4 * c).abs()).clamp(0, 1)).to(torch.uint8)
    return lut if device is None else lut.to(device)


def overlay(frames_u8, maps, scale: int = 16, lut=None):
    """The reference's show_cam_on_image (visualize_rel.py:39-44) for a batch of frames, decoder bytes in and displayable
    bytes out: frames_u8 (N, S, S, 3) uint8, maps (N, g, g) or (N, g*g) float32 (VideoExplanation.frame_s, say), lut
    (256, 3) uint8 (default jet_lut()) -> (N, g*scale, g*scale, 3) uint8.  Per frame: the map upsampled and min-max
    normalised as heatmaps() does, coloured through the table, added to the frame (resampled bilinearly to g*scale when
    S differs: 300 -> 304 at the native geometry), and the sum divided by its maximum over the frame."""
    if maps.dim() == 2:
        g = _grid(maps, 'overlay')
        maps = maps.reshape(maps.shape[0], g, g)
    if lut is None:
        lut = jet_lut(frames_u8.device)
    return ops.relevance_overlay_u8(frames_u8, maps, lut, scale)


def _paste_setup(n, Hs, Ws, side, boxes, transforms, lut, pixel_format, yuv_matrix):
    """the host half of a paste: geometry from the table that cut the crops and the colour table in the frames' space, ->
    (A, rect, lut) on the host, for one upload each.  Every argument error is raised here, before the device is touched."""
    from . import clips
    nv = pixel_format == 'nv12'
    A, rect = clips.paste_geometry(n, Hs, Ws, side, boxes=boxes, transforms=transforms, even=nv)
    if lut is None:
        lut = jet_lut()
    if not torch.is_tensor(lut) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError('lut must be uint8 (256, 3), got %s' % (tuple(lut.shape) if torch.is_tensor(lut) else type(lut).__name__,))
    if nv:
        lut = clips.lut_to_ycc(lut.cpu(), yuv_matrix)
    return A, rect, lut.cpu().contiguous()


def overlay_frames(frames, maps, boxes=None, transforms=None, side=None, alpha=0.5, lut=None, pixel_format: str = 'rgb24',
                   yuv_matrix: str = 'bt709', inplace: bool = False):
    """Relevance maps pasted back onto the whole frames their crops were cut from (DESIGN.md "Pasting maps onto frames"):
    frames uint8 (N, Hs, Ws, 3) -- pixel_format 'nv12': (N, 3 * Hs / 2, Ws) -- on the device, maps (N, g, g) or (N, g * g)
    float32 in crop coordinates (VideoExplanation.frame_s, say), exactly one of boxes int32 (N, 4) and transforms float32
    (N, 2, 3): the table that cut the crops of side `side`; alpha a float or float32 (N,); lut uint8 (256, 3) of RGB colours
    (default jet_lut()) -> frames of the input's format with every map normalised over its cells, coloured through the
    table and blended over its face (clips.paste_maps_host is the definition).  inplace=True writes into `frames` and costs
    the faces' area; several faces per frame are several calls in place."""
    from . import video
    if pixel_format not in ('rgb24', 'nv12'):
        raise ValueError("overlay_frames: pixel_format must be 'rgb24' or 'nv12', got %r" % (pixel_format,))
    if (boxes is None) == (transforms is None):
        raise ValueError('overlay_frames: boxes and transforms are two ways to cut the same crop: pass exactly one of them')
    n, Hs, Ws = video._whole_frames(frames, side, pixel_format, 'boxes' if boxes is not None else 'transforms')
    A, rect, table = (t.to(frames.device) for t in _paste_setup(n, Hs, Ws, int(side), boxes, transforms, lut, pixel_format,
                                                                yuv_matrix))
    return byte_frames.paste_maps(pixel_format, frames, maps, A, rect, table, alpha, int(side), inplace=inplace, checked=True)
