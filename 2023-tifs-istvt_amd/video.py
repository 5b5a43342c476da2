"""Scoring whole videos (DESIGN.md "Video scoring"): decoded frames in, one logit per sliding window and one score per
video out.

    scorer = VideoScorer(model, stride=1)
    res = scorer.score(frames)                       # uint8 (N, S, S, 3), host or device; or float32 (N, 3, S, S)
    ex = scorer.explain(frames)                      # the same windows through the relevance rollout, fused per frame
    res = scorer.score(full, boxes=boxes)            # whole frames uint8 (N, Hs, Ws, 3) and one face box per frame, int32
                                                     # (N, 4) = (y0, x0, h, w): cropped and resized on the device
    res = scorer.score(full, transforms=M)           # or one similarity per frame, float32 (N, 2, 3): aligned crops
                                                     # (ops.warp_similarity_u8), e.g. clips.similarity_from_landmarks
    scorer.reset()
    for chunk in stream:                             # the same windows, as the frames arrive
        logits, starts = scorer.push(chunk)
    logits, starts = scorer.flush()                  # the window that covers the tail, if one is due
    res = scorer.score_videos(videos, labels=labels)  # a test set: stem and window batches assembled across the videos, one
                                                     # synchronisation, per-video means and accuracy / AUC on the device

What `model(clips)` would pay for this and the scorer does not: the Xception stem runs once per frame instead of once per
(window, frame) -- in eval mode a frame's feature map does not depend on the clip around it --, conv1 reads the decoder's
bytes (istvt_conv1_fwd_u8) instead of a host-normalised float32 copy four times the size, and overlapping windows are
never copied out as clips: the per-frame features sit in a device ring and istvt_tokens_gather_fwd assembles each
window's tokens from its slots.

The schedule (which frames go through the stem when, which windows run when, which ring slot holds which frame) is host
logic with no tensor in it: RingPlan for one stream, SetPlan for a set of videos that share one bank, both testable
without a device.
"""
from __future__ import annotations

import contextlib
import heapq
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import frames as byte_frames      # (`frames` is every method's argument here)
from . import ops

Tensor = torch.Tensor
# the reference's preprocessing (network/xception.py:12 of the reference: Normalize([0.5] * 3, [0.5] * 3))
DEFAULT_MEAN = (0.5, 0.5, 0.5)
DEFAULT_STD = (0.5, 0.5, 0.5)


def window_starts(n: int, T: int, stride: int = 1, cover_tail: bool = True) -> List[int]:
    """First frames of the T-frame windows over an n-frame video: 0, stride, 2 stride, ... while the window fits, and with
    cover_tail one more at n - T when the last of those does not end at the last frame."""
    if T < 1 or stride < 1:
        raise ValueError('window_starts: T and stride must be positive, got T=%d stride=%d' % (T, stride))
    if n < T:
        raise ValueError('a video of %d frames is shorter than one window of %d' % (n, T))
    starts = list(range(0, n - T + 1, stride))
    if cover_tail and starts[-1] != n - T:
        starts.append(n - T)
    return starts


def check_frames(frames) -> str:
    """'u8' for decoded frames uint8 (N, S, S, 3), 'f32' for normalised float32 (N, 3, S, S); ValueError otherwise."""
    if not torch.is_tensor(frames):
        raise ValueError('frames must be a torch tensor, got %s' % type(frames).__name__)
    if frames.dim() != 4:
        raise ValueError('frames must be uint8 (N, S, S, 3) or float32 (N, 3, S, S), got rank %d: %s'
                         % (frames.dim(), tuple(frames.shape)))
    if frames.dtype == torch.uint8:
        if frames.shape[3] != 3 or frames.shape[1] != frames.shape[2]:
            raise ValueError('uint8 frames must be channels-last (N, S, S, 3) as a decoder delivers them, got %s'
                             % (tuple(frames.shape),))
        return 'u8'
    if frames.dtype == torch.float32:
        if frames.shape[1] != 3 or frames.shape[2] != frames.shape[3]:
            raise ValueError('float frames must be normalised (N, 3, S, S), got %s' % (tuple(frames.shape),))
        return 'f32'
    raise ValueError('frames must be uint8 or float32, got %s' % frames.dtype)


def _whole_frames(frames, side: Optional[int], pixel_format: str, word: str):
    """(N, Hs, Ws) of whole frames that a table of `word` ('boxes' or 'transforms') cuts crops of side `side` from: uint8
    (N, Hs, Ws, 3), or NV12 uint8 (N, 3 * Hs / 2, Ws); ValueError otherwise"""
    from . import clips
    if side is None:
        raise ValueError('%s need the side of the crops: VideoScorer(model, side=S) or model.set_crop_side(S)' % word)
    if not torch.is_tensor(frames):
        raise ValueError('frames must be a torch tensor, got %s' % type(frames).__name__)
    if pixel_format == 'nv12':
        if frames.dtype != torch.uint8 or frames.dim() != 3:
            raise ValueError('NV12 frames must be uint8 (N, 3 * Hs / 2, Ws) as a decoder delivers them, got %s %s'
                             % (frames.dtype, tuple(frames.shape)))
        return (int(frames.shape[0]),) + clips.check_nv12(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError('with %s, frames must be uint8 channels-last (N, Hs, Ws, 3) as a decoder delivers them, got %s %s'
                         % (word, frames.dtype, tuple(frames.shape)))
    return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])


def check_boxed_frames(frames, boxes, side: Optional[int], pixel_format: str = 'rgb24'):
    """Whole frames with one face box each (DESIGN.md "Frames and boxes"): frames uint8 (N, Hs, Ws, 3) of any size, boxes
    int32 (N, 4) = (y0, x0, h, w) inside the frame with 1 <= h, w <= 8 side.  pixel_format 'nv12' (DESIGN.md "NV12 frames"):
    frames uint8 (N, 3 * Hs / 2, Ws), the boxes in pixels of the Hs x Ws picture.  -> the validated box table on the host."""
    from . import clips
    n, Hs, Ws = _whole_frames(frames, side, pixel_format, 'boxes')
    return clips.check_boxes(boxes, n, Hs, Ws, int(side))


def check_aligned_frames(frames, transforms, side: Optional[int], pixel_format: str = 'rgb24'):
    """Whole frames with one similarity each (DESIGN.md "Aligned crops"): frames as check_boxed_frames takes them, transforms
    float32 (N, 2, 3) as clips.check_similarities validates them.  -> the validated table on the host."""
    from . import clips
    n, Hs, Ws = _whole_frames(frames, side, pixel_format, 'transforms')
    return clips.check_similarities(transforms, n, Hs, Ws, int(side))


class Step(NamedTuple):
    """One unit of work of a RingPlan.  kind 'frames': frames [first, first + count) go through the stem into ring slots
    `slots` (one per frame).  kind 'windows': the windows starting at `starts` run; idx[w][t] is the slot of frame
    starts[w] + t."""
    kind: str
    first: int
    count: int
    slots: Tuple[int, ...]
    starts: Tuple[int, ...]
    idx: Optional[Tensor]


class RingPlan:
    """The order of work for a stream of frames whose features live in a ring of `capacity` slots (frame i in slot
    i mod capacity).  push(k) plans k more frames, flush() the tail window.  Frames go through the stem at most
    frame_batch at a time, windows run window_batch at a time as they complete, and every window completed by the frames
    of a push has run when the push returns.

    The invariant: a slot is overwritten only when no window that is pending or still to come, the tail window of a later
    flush() included, reads the frame in it.  Everything still to come reads only the last T frames, so a batch of k new
    frames -- which overwrites frames up to seen + k - 1 - capacity -- is cut to k <= capacity - T (no cut while the ring
    has never been full), and windows that are complete but still queued for a full batch run first when they read a
    slot the batch is about to take."""

    def __init__(self, T: int, stride: int, capacity: int, frame_batch: int, window_batch: int):
        if T < 1 or stride < 1 or frame_batch < 1 or window_batch < 1:
            raise ValueError('RingPlan: T, stride, frame_batch and window_batch must be positive')
        if capacity < T:
            raise ValueError('a ring of %d frames cannot hold one window of %d' % (capacity, T))
        self.T, self.stride, self.capacity = T, stride, capacity
        self.frame_batch, self.window_batch = frame_batch, window_batch
        self.seen = 0                      # frames planned so far (absolute index of the next one)
        self.next_start = 0                # first regular window that is not complete yet
        self.last_start = -1               # start of the last window planned
        self.pending: List[int] = []       # complete, not yet planned into a 'windows' step
        self.flushed = False

    def _windows(self, steps: List[Step], count: int):
        starts, self.pending = self.pending[:count], self.pending[count:]
        idx = torch.tensor([[(s + t) % self.capacity for t in range(self.T)] for s in starts], dtype=torch.int32)
        steps.append(Step('windows', starts[0], len(starts), (), tuple(starts), idx))
        self.last_start = starts[-1]

    def _drain(self, steps: List[Step]):
        while self.pending:
            self._windows(steps, min(len(self.pending), self.window_batch))

    def push(self, k: int, drain: bool = True) -> List[Step]:
        """drain=False leaves the last, partial batch of complete windows queued (for a flush() that follows at once)."""
        if self.flushed:
            raise RuntimeError('this stream has been flushed: reset() starts a new one')
        steps: List[Step] = []
        C, T = self.capacity, self.T
        while k > 0:
            room = max(C - self.seen, C - T)
            if room < 1:
                raise ValueError('a ring of %d frames holds one window of %d and nothing more: streaming needs capacity > T'
                                 % (C, T))
            kb = min(k, self.frame_batch, room)
            if self.pending and self.pending[0] <= self.seen + kb - 1 - C:
                self._drain(steps)         # they read slots this batch overwrites
            steps.append(Step('frames', self.seen, kb, tuple((self.seen + i) % C for i in range(kb)), (), None))
            self.seen += kb
            k -= kb
            while self.next_start + T <= self.seen:
                self.pending.append(self.next_start)
                self.next_start += self.stride
            while len(self.pending) >= self.window_batch:
                self._windows(steps, self.window_batch)
        if drain:
            self._drain(steps)
        return steps

    def flush(self, cover_tail: bool = True) -> List[Step]:
        """The end of the stream: the window at seen - T when cover_tail asks for it and no window ends at the last frame."""
        if self.flushed:
            return []
        if self.seen < self.T:
            raise ValueError('a video of %d frames is shorter than one window of %d' % (self.seen, self.T))
        self.flushed = True
        steps: List[Step] = []
        last = self.pending[-1] if self.pending else self.last_start
        if cover_tail and last != self.seen - self.T:
            self.pending.append(self.seen - self.T)
        self._drain(steps)
        return steps


class SetPlan:
    """The order of work for a set of V videos of n_0 ... n_{V-1} frames whose features share one bank of `capacity` slots
    (DESIGN.md "Scoring a set of videos").  The frames of all videos form one sequence (video after video; frame i of video v
    is number frame_offsets[v] + i) and so do the windows (those of video v are window_starts(n_v, T, stride, cover_tail), in
    that order; video v owns the windows [offsets[v], offsets[v + 1])).

    steps           the Steps VideoScorer runs, in order.  'frames': frames [first, first + count) of the sequence go through
                    the stem into the bank slots `slots`; a batch may cross a video boundary.  'windows': the windows
                    [first, first + count) of the window sequence run; `starts` are their first frames inside their own
                    videos and idx[w][t] is the slot that holds frame t of window first + w.  Windows of several videos share a
                    batch: every batch is full except the last one of the plan.
    window_video    the video of every window;  starts: its first frame inside that video.
    capacity        slots of the bank (default: frame_batch + window_batch * T rounded up to a multiple of 8, where no batch is
                    ever cut); slots_used: the highest slot named, plus one -- what has to be allocated.
    full_batches, partial_batches   window batches of window_batch windows, and of fewer.

    The bank is a pool: a frame takes the lowest free slot, and the slot returns to the pool when the last window that reads
    the frame has been planned into a step (a frame no window reads returns its slot with its own stem batch).  The device
    runs the steps in order, so a slot handed out again is written only after every window that read its previous frame.
    When the next frame batch would find too few free slots, the complete windows that are still queued for a full batch
    are issued first, as a partial batch: they then hold nothing, and what remains held are the at most T - 1 frames of the
    one window that is not complete yet.  Hence the smallest capacity, frame_batch + T."""

    def __init__(self, counts: Sequence[int], T: int, stride: int = 1, cover_tail: bool = True, frame_batch: int = 64,
                 window_batch: int = 32, capacity: Optional[int] = None):
        if T < 1 or stride < 1 or frame_batch < 1 or window_batch < 1:
            raise ValueError('SetPlan: T, stride, frame_batch and window_batch must be positive')
        counts = [int(n) for n in counts]
        if not counts:
            raise ValueError('SetPlan: no videos')
        for v, n in enumerate(counts):
            if n < T:
                raise ValueError('video %d has %d frames: shorter than one window of %d' % (v, n, T))
        if capacity is None:
            capacity = self.default_capacity(T, frame_batch, window_batch)
        if capacity < frame_batch + T:
            raise ValueError('a bank of %d slots is too small for a frame batch of %d and one window of %d: %d at least'
                             % (capacity, frame_batch, T, frame_batch + T))
        self.T, self.stride, self.cover_tail = T, stride, bool(cover_tail)
        self.frame_batch, self.window_batch, self.capacity = frame_batch, window_batch, int(capacity)
        self.counts = counts
        self.frame_offsets, self.offsets = [0], [0]
        self.window_video: List[int] = []
        self.starts: List[int] = []
        for v, n in enumerate(counts):
            st = window_starts(n, T, stride, cover_tail)
            self.window_video += [v] * len(st)
            self.starts += st
            self.frame_offsets.append(self.frame_offsets[-1] + n)
            self.offsets.append(self.offsets[-1] + len(st))
        self.steps: List[Step] = []
        self.full_batches = self.partial_batches = 0
        self.slots_used = 0
        self._build()

    @staticmethod
    def default_capacity(T: int, frame_batch: int, window_batch: int) -> int:
        return -(-(frame_batch + window_batch * T) // 8) * 8

    def _build(self):
        T, G, W = self.T, self.frame_offsets[-1], len(self.starts)
        first = [self.frame_offsets[v] + s for v, s in zip(self.window_video, self.starts)]   # first frame, in the sequence
        readers = [0] * G                  # windows not yet planned that read the frame
        for f in first:
            for t in range(T):
                readers[f + t] += 1
        slot_of = [-1] * G
        free = list(range(self.capacity))  # a heap: the lowest free slot first
        pending: List[int] = []            # windows whose frames are all in the bank, not yet planned
        done = 0                           # windows [0, done) are complete (all their frames planned); they complete in order

        def windows(count):
            ws, pending[:] = pending[:count], pending[count:]
            idx = torch.tensor([[slot_of[first[w] + t] for t in range(T)] for w in ws], dtype=torch.int32)
            self.steps.append(Step('windows', ws[0], len(ws), (), tuple(self.starts[w] for w in ws), idx))
            if len(ws) == self.window_batch:
                self.full_batches += 1
            else:
                self.partial_batches += 1
            for w in ws:
                for t in range(T):
                    f = first[w] + t
                    readers[f] -= 1
                    if readers[f] == 0:
                        heapq.heappush(free, slot_of[f])

        g = 0
        while g < G:
            kb = min(self.frame_batch, G - g)
            if len(free) < kb and pending:
                windows(len(pending))      # early and partial: the bank has no room for the next frame batch otherwise
            assert len(free) >= kb, 'SetPlan: the bank ran out of slots'          # capacity >= frame_batch + T rules it out
            slots = tuple(heapq.heappop(free) for _ in range(kb))
            self.slots_used = max(self.slots_used, max(slots) + 1)
            self.steps.append(Step('frames', g, kb, slots, (), None))
            for i, sl in enumerate(slots):
                slot_of[g + i] = sl
                if readers[g + i] == 0:    # a frame between two windows (stride > T) or past the last one (no cover_tail)
                    heapq.heappush(free, sl)
            g += kb
            while done < W and first[done] + T <= g:
                pending.append(done)
                done += 1
            while len(pending) >= self.window_batch:
                windows(self.window_batch)
        while pending:
            windows(min(len(pending), self.window_batch))

    def pieces(self, first: int, count: int) -> List[Tuple[int, int, int]]:
        """the frames [first, first + count) of the sequence as (video, lo, hi) pieces, frames [lo, hi) of that video"""
        out = []
        v = 0
        while self.frame_offsets[v + 1] <= first:
            v += 1
        end = first + count
        while first < end:
            hi = min(end, self.frame_offsets[v + 1])
            out.append((v, first - self.frame_offsets[v], hi - self.frame_offsets[v]))
            first = hi
            v += 1
        return out


class VideoScore(NamedTuple):
    """Result of VideoScorer.score: device tensors, complete when score() returns."""
    window_logits: Tensor      # (W, num_classes) float32
    starts: Tensor             # (W,) int64: first frame of every window
    logit_mean: Tensor         # (num_classes,) mean of the window logits
    prob_mean: Tensor          # (num_classes,) mean of the windows' sigmoids


class VideoExplanation(NamedTuple):
    """Result of VideoScorer.explain: device tensors, complete when explain() returns.  P - 1 = g * g map positions."""
    score: VideoScore          # as score(frames) returns it, for the same windows
    windows: object            # explain.Relevance: every window's own maps, cam_s / cam_t (W, T, P-1), in window order
    frame_s: Tensor            # (N, P-1) float32: mean over the covering windows of cam_s[w, n - start_w]
    frame_t: Tensor            # (N, P-1) float32: the same of cam_t
    frame_weight: Tensor       # (N,) float32: mean of r_t[w, 0, n - start_w + 1], how much the verdict rests on the frame
    frame_logit: Tensor        # (N,) float32: mean of logits[w, index] over the covering windows
    count: Tensor              # (N,) int32: number of windows that cover the frame (0: zeros in the other fields)


class SetMetrics(NamedTuple):
    """Result of set_metrics: 0-dim device tensors; nothing has been synchronised."""
    correct: Tensor            # int64: videos with a finite score and (score > threshold) == (label == 1)
    positives: Tensor          # int64: videos labelled 1
    negatives: Tensor          # int64: videos labelled 0
    nonfinite: Tensor          # int64: videos whose score is NaN or infinite (in no pair, never correct)
    auc: Tensor                # float64: (greater + equal / 2) / (positives * negatives); NaN when a class is empty
    greater: Tensor            # int64: (positive, negative) pairs with s_p > s_n
    equal: Tensor              # int64: pairs with s_p == s_n


class VideoSetScore(NamedTuple):
    """Result of VideoScorer.score_videos: device tensors, complete when score_videos() returns.  The windows of video v are
    the rows [offsets[v], offsets[v + 1])."""
    window_logits: Tensor      # (W, num_classes) float32, video after video
    window_video: Tensor       # (W,) int32: the video of every window
    starts: Tensor             # (W,) int64: first frame of every window inside its video
    offsets: Tensor            # (V + 1,) int32
    logit_mean: Tensor         # (V, num_classes) mean of each video's window logits
    prob_mean: Tensor          # (V, num_classes) mean of each video's windows' sigmoids
    metrics: Optional[SetMetrics]      # set_metrics(logit_mean[:, 0], labels) when labels were given


def _validate_labels(labels, V: int) -> Tensor:
    """labels of 0 / 1, one per video, checked on the host -> the tensor.  A host tensor or a list is validated; a device
    tensor is taken as it is (checking it would synchronise): anything but 0 counts as 1."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.shape[0] != V:
        raise ValueError('labels: one 0 / 1 per video expected, (%d,), got %s' % (V, tuple(labels.shape)))
    if not labels.is_cuda and not bool(((labels == 0) | (labels == 1)).all()):
        raise ValueError('labels must be 0 or 1')
    return labels


def _upload_labels(labels: Tensor, dev) -> Tensor:
    """validated labels -> int32 (V,) on dev"""
    if not labels.is_cuda:
        return labels.to(torch.int32).to(dev, non_blocking=True)
    return labels.to(device=dev, dtype=torch.int32)


def set_metrics(scores: Tensor, labels, threshold: float = 0.0) -> SetMetrics:
    """Accuracy counts and the pairwise AUC of V video scores on the device (ops.auc_pairs), without a synchronisation.
    scores (V,) float32 on the device, labels (V,) of 0 / 1 (host or device)."""
    if not torch.is_tensor(scores) or scores.dim() != 1 or scores.shape[0] < 1:
        raise ValueError('scores: one per video expected, (V,), got %s'
                         % (tuple(scores.shape) if torch.is_tensor(scores) else type(scores).__name__,))
    ops._req(scores, 'scores')
    lab = _upload_labels(_validate_labels(labels, int(scores.shape[0])), scores.device)
    counts, auc = ops.auc_pairs(scores.float(), lab, threshold)
    c = dict(zip(ops.AUC_COUNTS, counts.unbind(0)))
    return SetMetrics(c['correct'], c['positives'], c['negatives'], c['nonfinite'], auc[0], c['greater'], c['equal'])


def windows_reduce_ref(logits: Tensor, offsets) -> Tuple[Tensor, Tensor]:
    """ops.windows_reduce restated in float64 on the host: (logit_mean, prob_mean), float64 (V, nc)"""
    x = logits.detach().cpu().double()
    off = [int(v) for v in (offsets.tolist() if torch.is_tensor(offsets) else offsets)]
    lm = torch.stack([x[a:b].sum(0) / (b - a) for a, b in zip(off, off[1:])])
    pm = torch.stack([(1.0 / (1.0 + torch.exp(-x[a:b]))).sum(0) / (b - a) for a, b in zip(off, off[1:])])
    return lm, pm


def set_metrics_ref(scores, labels, threshold: float = 0.0) -> dict:
    """set_metrics restated on the host with sorted ranks instead of pairs: Python ints and a Python float (auc)"""
    s = torch.as_tensor(scores).detach().cpu().float()
    lab = torch.as_tensor(labels).detach().cpu() != 0
    fin = torch.isfinite(s)
    neg = torch.sort(s[~lab & fin].double()).values
    pos = s[lab & fin].double()
    below = torch.searchsorted(neg, pos, right=False)      # negatives strictly below every positive
    upto = torch.searchsorted(neg, pos, right=True)
    greater, equal = int(below.sum()), int((upto - below).sum())
    P, N = int(lab.sum()), int((~lab).sum())
    auc = (float(greater) + 0.5 * float(equal)) / (float(P) * float(N)) if P and N else float('nan')
    correct = int((fin & ((s > threshold) == lab)).sum())
    return dict(correct=correct, positives=P, negatives=N, nonfinite=int((~fin).sum()), auc=auc, greater=greater, equal=equal)


class VideoInput(NamedTuple):
    """What a call hands over for one video (VideoScorer._input)."""
    reads: str                 # what the stem reads: 'u8' decoded bytes, 'f32' normalised floats
    boxed: bool                # whole frames with one box or one similarity each: every stem batch is cropped to side x
                               # side first
    side: Optional[int]        # the side of those crops (None without boxes)
    table: Optional[Tensor]    # the validated table on the host: boxes int32 (N, 4), or similarities float32 (N, 2, 3) when
                               # `aligned` (None without either)
    aligned: bool = False      # the crops are cut through similarities (ops.warp_similarity_*), not boxes


def slot_runs(slots: Sequence[int]) -> List[Tuple[int, int]]:
    """The slots of a frame batch as (first slot, count) runs of consecutive slots, in order: one run for a batch that lies
    in the bank as it is, two where a ring wraps, more for slots scattered over a pool."""
    runs = [[slots[0], 1]]
    for s in slots[1:]:
        if s == runs[-1][0] + runs[-1][1]:
            runs[-1][1] += 1
        else:
            runs.append([s, 1])
    return [(s0, k) for s0, k in runs]


def _store(bank: Tensor, feats: Tensor, slots: Tuple[int, ...], dslots: Optional[Tensor] = None):
    """feats[i] -> bank[slots[i]]: slice copies run by run, or one index_copy_ when the slots are scattered and the caller
    has them on the device (dslots, int64)"""
    runs = slot_runs(slots)
    if len(runs) > 1 and dslots is not None:
        bank.index_copy_(0, dslots, feats)
        return
    at = 0
    for s0, k in runs:
        bank[s0:s0 + k].copy_(feats[at:at + k])
        at += k


@contextlib.contextmanager
def _eval_mode(model):
    """eval mode for the call; every module's own train / eval flag comes back afterwards (as explain.relevance does)"""
    on = [m for m in model.modules() if m.training]         # one walk; a model already in eval mode costs nothing more
    try:
        for m in on:
            m.training = False
        yield
    finally:
        for m in on:
            m.training = True


class VideoScorer:
    """Sliding-window scores of an XceptionVidTr over decoded video frames.

    model         the XceptionVidTr; its compute_dtype, attn_fp8 and dead_row_elimination settings are used as they are.
                  It is put in eval mode for each call and handed back with its train / eval flags as they were; running
                  statistics and num_batches_tracked are not touched.
    stride        frames between window starts.
    frame_batch   frames per stem pass.        window_batch   windows per transformer pass.
    capacity      frames of features the device ring holds (default: the whole video for score(), T + frame_batch
                  rounded up to a multiple of 8 for push()).
    mean, std     per-channel normalisation of uint8 frames, (u / 255 - mean) / std; float input is taken as normalised.
    cover_tail    score() / flush() add the window at N - T when the strided windows leave the last frames uncovered.
    side          the side of the crops made of whole frames when a call passes `boxes` (default: the model's crop_side).
    jpeg_quality  None, or an int in 1..100: every uint8 stem batch goes through ops.jpeg_roundtrip_u8 at that quality (4:2:0)
                  just before the stem, after the crop when a call passes `boxes` -- the S x S crops the stem reads are
                  recompressed, not the whole frames.  score(), push(), score_videos() and explain() then give the bits they
                  give on ops.jpeg_roundtrip_u8(crops, jpeg_quality); float frames raise TypeError.
    perturb       None, or a (kind_name, value) pair as clips.perturbation takes it -- ('blur', 2.0), ('noise', 10.0),
                  ('saturation', 0.4), ('pixelate', 4), ...: every uint8 stem batch goes through ops.perturb_u8, after the crop
                  when a call passes `boxes` or `transforms` and before the JPEG round trip when jpeg_quality is set too (a
                  perturbed video is then compressed).  A frame's row is (kind, param, its index in its video -- counted since
                  reset() for push() --, its video's index in the call -- 0 for score(), push() and explain()), so with tab,
                  taps = clips.perturbation_table(N, *perturb) the scorer gives the bits it gives on ops.perturb_u8(crops,
                  tab, taps, perturb_seed), whatever the batches; float frames raise TypeError.
    perturb_seed  the 64-bit key of the noise.
    pixel_format  'rgb24' (packed RGB, the default) or 'nv12': every call then takes NV12 frames uint8 (N, 3 * Hs / 2, Ws) and
                  needs `boxes` (ValueError without; frames that already are the crops take identity boxes).  The crop reads
                  the NV12 bytes itself (ops.crop_resize_nv12): the bits of the 'rgb24' scorer on
                  ops.crop_resize_nv12(frames, boxes, side, yuv_matrix), and everything after the crop is the same code.
    yuv_matrix    'bt601', 'bt709' (limited range) or 'jfif' (full range): how 'nv12' frames become RGB.

    Every call that takes `boxes` takes `transforms` in their place (never both: ValueError): one similarity per frame,
    float32 (N, 2, 3), output pixel centres to source coordinates (clips.check_similarities).  The crops are then
    ops.warp_similarity_u8(frames, transforms, side) -- ops.warp_similarity_nv12 for 'nv12' frames -- and everything after the
    crop is the same code; explain() gives its maps in crop coordinates.
    """

    def __init__(self, model, stride: int = 1, frame_batch: int = 64, window_batch: int = 32,
                 capacity: Optional[int] = None, mean: Sequence[float] = DEFAULT_MEAN, std: Sequence[float] = DEFAULT_STD,
                 cover_tail: bool = True, side: Optional[int] = None, jpeg_quality: Optional[int] = None,
                 pixel_format: str = 'rgb24', yuv_matrix: str = 'bt709', perturb=None, perturb_seed: int = 0):
        vit = getattr(model, 'vit', None)
        if vit is None or not hasattr(model, 'xcep') or not hasattr(vit, 'forward_tokens'):
            raise TypeError('VideoScorer: expected an XceptionVidTr, got %s' % type(model).__name__)
        if stride < 1 or frame_batch < 1 or window_batch < 1:
            raise ValueError('VideoScorer: stride, frame_batch and window_batch must be positive')
        self.model = model
        self.T = int(vit.pos_embedding.shape[1])
        if capacity is not None and capacity <= self.T:
            raise ValueError('VideoScorer: capacity %d must exceed the window length %d' % (capacity, self.T))
        if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
            raise ValueError('VideoScorer: mean and std take 3 values each, std non-zero')
        self.stride, self.frame_batch, self.window_batch = int(stride), int(frame_batch), int(window_batch)
        self.capacity = capacity
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.cover_tail = bool(cover_tail)
        if side is not None and int(side) < 3:
            raise ValueError('VideoScorer: side must be at least 3, got %r' % (side,))
        self.side = None if side is None else int(side)
        if jpeg_quality is not None and (isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, int)
                                         or not 1 <= jpeg_quality <= 100):
            raise ValueError('VideoScorer: jpeg_quality must be None or an int in [1, 100], got %r' % (jpeg_quality,))
        self.jpeg_quality = jpeg_quality
        if pixel_format not in ('rgb24', 'nv12'):
            raise ValueError("VideoScorer: pixel_format must be 'rgb24' or 'nv12', got %r" % (pixel_format,))
        from . import clips
        if yuv_matrix not in clips.YUV_MATRICES:
            raise ValueError("VideoScorer: yuv_matrix must be 'bt601', 'bt709' or 'jfif', got %r" % (yuv_matrix,))
        self.pixel_format, self.yuv_matrix = pixel_format, yuv_matrix
        self.perturb = None                # (kind, param, host taps or None) of clips.perturbation
        if perturb is not None:
            if not isinstance(perturb, (tuple, list)) or len(perturb) != 2:
                raise ValueError('VideoScorer: perturb must be None or a (kind_name, value) pair, got %r' % (perturb,))
            self.perturb = clips.perturbation(*perturb)
        self.perturb_seed = int(perturb_seed)
        if not 0 <= self.perturb_seed < 2 ** 64:
            raise ValueError('VideoScorer: perturb_seed must lie in [0, 2^64), got %r' % (perturb_seed,))
        self._taps = None                  # the perturbation's taps on the device
        self._norm = None                  # (device, mean tensor, std tensor)
        self._jpeg = None                  # the device quality table of a stem batch: jpeg_quality, frame_batch times
        self.reset()

    # ---------------------------------------------------------------------------------------- what a call hands over
    def _device(self):
        dev = next(self.model.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('VideoScorer: the model must be on a ROCm device (no CPU fallback exists for the ISTVT hot path)')
        return dev

    def _input(self, frames, boxes, transforms=None) -> VideoInput:
        """The frames (and boxes or transforms) of one video, checked: every argument error of a call, before anything is
        launched."""
        if boxes is not None and transforms is not None:
            raise ValueError('VideoScorer: boxes and transforms are two ways to cut the same crop: pass one of them')
        if transforms is not None:
            side = self.side if self.side is not None else getattr(self.model, 'crop_side', None)
            return VideoInput('u8', True, side, check_aligned_frames(frames, transforms, side, self.pixel_format), True)
        if boxes is None and self.pixel_format == 'rgb24':
            reads = check_frames(frames)
            if self.jpeg_quality is not None and reads == 'f32':
                raise TypeError('VideoScorer: jpeg_quality recompresses decoded uint8 frames; normalised float frames cannot '
                                'take it')
            if self.perturb is not None and reads == 'f32':
                raise TypeError('VideoScorer: perturb degrades decoded uint8 frames; normalised float frames cannot take it')
            return VideoInput(reads, False, None, None)
        if boxes is None:
            raise ValueError("VideoScorer: pixel_format='nv12' needs boxes or transforms with every call (one (y0, x0, h, w) or "
                             'one similarity per frame; frames that already are the crops take identity boxes)')
        side = self.side if self.side is not None else getattr(self.model, 'crop_side', None)
        return VideoInput('u8', True, side, check_boxed_frames(frames, boxes, side, self.pixel_format))

    def _fetcher(self, videos, inputs: Sequence[VideoInput], pieces, dev, frame0: int = 0):
        """-> fetch(first, count), the stem batch of frames [first, first + count) of the executor's steps;
        pieces(first, count) names them as (video, lo, hi).  The tables are uploaded here, once.  The inputs of one call are
        all of one kind (_check_set and _input see to it: boxes for every video, transforms for every video, or neither), so
        the first one speaks for the set.  frame0: the index in its video of frame 0 of `videos[0]` (push(): the frames the
        stream has seen), which only a perturbation reads."""
        bdev = [i.table.contiguous().to(dev, non_blocking=True) for i in inputs] if inputs[0].boxed else None
        if self.perturb is None:
            return lambda first, count: self._frame_batch(videos, pieces(first, count), bdev, inputs[0].side, dev,
                                                          inputs[0].aligned)

        def fetch(first, count):
            ps = pieces(first, count)
            return self._perturbed(self._frame_batch(videos, ps, bdev, inputs[0].side, dev, inputs[0].aligned), ps, dev, frame0)
        return fetch

    def _perturbed(self, x: Tensor, pieces, dev, frame0: int) -> Tensor:
        """the stem batch of (video, lo, hi) pieces through ops.perturb_u8: frame i of video v is (kind, param, frame0 + i, v)"""
        kind, param, taps = self.perturb
        if not x.is_cuda:                  # host frames: pinned, then copied on the current stream
            x = x.contiguous().pin_memory().to(dev, non_blocking=True)
        table = torch.tensor([(kind, param, frame0 + i, v) for v, lo, hi in pieces for i in range(lo, hi)], dtype=torch.int32)
        if taps is not None and (self._taps is None or self._taps.device != dev):
            self._taps = taps.to(dev)
        return ops.perturb_u8(x.contiguous(), table.pin_memory().to(dev, non_blocking=True),
                              None if taps is None else self._taps, self.perturb_seed, checked=True)

    def _frame_batch(self, videos, pieces, bdev, side, dev, aligned: bool = False) -> Tensor:
        """One stem batch from (video, lo, hi) pieces.  Without boxes a single piece is used where it lies (_stem uploads a
        host batch); several are copied into one staging batch on the device (host pieces pinned first).  With boxes (bdev:
        one validated device table per video) every piece is cropped into its slice of one batch of side x side crops, from
        NV12 or packed RGB as the scorer's pixel_format says; `aligned`: the tables hold similarities and the crops are warps."""
        if bdev is None and len(pieces) == 1:
            v, lo, hi = pieces[0]
            return videos[v][lo:hi]
        n = sum(hi - lo for _, lo, hi in pieces)
        first = videos[pieces[0][0]]
        shape = (n, side, side, 3) if bdev is not None else (n,) + tuple(first.shape[1:])
        batch = torch.empty(shape, dtype=first.dtype, device=dev)
        at = 0
        for v, lo, hi in pieces:
            x, out = videos[v][lo:hi], batch[at:at + hi - lo]
            if not x.is_cuda:
                x = x.contiguous().pin_memory()
            if bdev is None:
                out.copy_(x, non_blocking=True)
            else:
                byte_frames.crop_frames(self.pixel_format, aligned, x.to(dev, non_blocking=True), bdev[v][lo:hi], side,
                                        self.yuv_matrix, out=out, checked=True)
            at += hi - lo
        return batch

    # ---------------------------------------------------------------------------------------- the executor
    def _stem(self, x: Tensor, kind: str, dev) -> Tensor:
        """a stem batch ('u8' bytes or 'f32' normalised floats) -> its features (n, h * w, C)"""
        if not x.is_cuda:                  # host frames: pinned, then copied on the current stream
            x = x.contiguous().pin_memory().to(dev, non_blocking=True)
        if self.jpeg_quality is not None:  # the bytes the stem reads, as a JPEG codec would hand them back
            n = int(x.shape[0])
            if self._jpeg is None or self._jpeg.device != dev or self._jpeg.shape[0] < n:
                self._jpeg = torch.full((max(n, self.frame_batch),), self.jpeg_quality, dtype=torch.int32, device=dev)
            x = ops.jpeg_roundtrip_u8(x.contiguous(), self._jpeg[:n], checked=True)
        xcep = self.model.xcep.model
        if kind == 'u8':
            if self._norm is None or self._norm[0] != dev:
                self._norm = (dev, torch.tensor(self.mean, dtype=torch.float32, device=dev),
                              torch.tensor(self.std, dtype=torch.float32, device=dev))
            feats = xcep.low_level_features_nhwc(x, self.model.compute_dtype, self._norm[1], self._norm[2])
        else:
            feats = xcep.low_level_features_nhwc(x, self.model.compute_dtype, inference=True)
        n, h, w, c = feats.shape
        return feats.view(n, h * w, c)

    def _execute(self, steps: Sequence[Step], bank: Optional[Tensor], slots: int, dev, fetch=None, reads: Optional[str] = None,
                 rollout=None, dslots: Optional[Tensor] = None):
        """Runs the steps, in order, against the feature bank it is given -> (bank, logits (W, num_classes) float32 on the
        device, list of starts) of the windows that ran.  A 'frames' step sends fetch(first, count) through the stem (`reads`
        as VideoInput has it) into its slots; a 'windows' step assembles the tokens of its windows from the bank and runs
        the transformer on them.  bank None: allocated with `slots` slots from the shape of the first stem batch.  idx of a
        'windows' step: a host table, validated and uploaded by ops.tokens_gather_fwd, or a device table the caller has
        validated.  rollout: what runs a batch of windows instead of the plain forward, (tokens, windows, h*w) -> logits
        (explain()).  dslots: the slots of all 'frames' steps, one after the other, int64 on the device."""
        vit = self.model.vit
        outs, starts, fpos = [], [], 0
        with _eval_mode(self.model), torch.no_grad():
            for st in steps:
                if st.kind == 'frames':
                    feats = self._stem(fetch(st.first, st.count), reads, dev)
                    if bank is None:
                        bank = torch.empty((slots,) + tuple(feats.shape[1:]), dtype=feats.dtype, device=dev)
                    elif tuple(bank.shape[1:]) != tuple(feats.shape[1:]) or bank.dtype != feats.dtype:
                        raise RuntimeError('VideoScorer: the frames of one stream must share one size and compute dtype '
                                           '(reset() starts a new stream)')
                    _store(bank, feats, st.slots, None if dslots is None else dslots[fpos:fpos + st.count])
                    fpos += st.count
                else:
                    hw = bank.shape[1]
                    x = ops.tokens_gather_fwd(bank, st.idx, vit.space_token, vit.temporal_token, vit.pos_embedding, pad=True,
                                              checked=st.idx.is_cuda)
                    outs.append(vit.forward_tokens(x, st.count, self.T + 1, hw + 1) if rollout is None
                                else rollout(x, st.count, hw))
                    starts.extend(st.starts)
        if len(outs) == 1:
            return bank, outs[0], starts
        nc = vit.mlp_head[1].out_features
        return bank, torch.cat(outs) if outs else torch.empty((0, nc), dtype=torch.float32, device=dev), starts

    # ---------------------------------------------------------------------------------------- a stream
    def reset(self):
        """Forget the stream: the next push() is frame 0 of a new video."""
        self._plan: Optional[RingPlan] = None
        self._ring: Optional[Tensor] = None
        self._kind: Optional[VideoInput] = None            # what the stream's first push handed over
        return self

    def push(self, frames: Tensor, boxes=None, transforms=None):
        """The next frames of the stream -> (logits (W, num_classes) float32 on the device, starts (W,) int64 on the host)
        of the windows these frames complete, in stream order: with flush(), the windows of score() on the concatenation.
        boxes: one (y0, x0, h, w) per frame of this push, for whole frames uint8 (k, Hs, Ws, 3); transforms: one similarity per
        frame in their place; a stream keeps one mode."""
        inp = self._input(frames, boxes, transforms)
        if self._kind is not None and (inp.boxed != self._kind.boxed or inp.aligned != self._kind.aligned):
            raise ValueError('VideoScorer: a stream takes boxes with every push, transforms with every push, or neither '
                             '(reset() starts a new one)')
        if self._kind is not None and inp.reads != self._kind.reads:
            raise ValueError('VideoScorer: a stream is either uint8 or float frames, not both (reset() starts a new one)')
        dev = self._device()
        if self._plan is None:
            cap = self.capacity if self.capacity is not None else -(-(self.T + self.frame_batch) // 8) * 8
            self._plan = RingPlan(self.T, self.stride, cap, self.frame_batch, self.window_batch)
        self._kind = inp._replace(table=None)
        base = self._plan.seen
        fetch = self._fetcher([frames], [inp], lambda first, count: [(0, first - base, first - base + count)], dev, base)
        self._ring, logits, starts = self._execute(self._plan.push(int(frames.shape[0])), self._ring, self._plan.capacity, dev,
                                                   fetch, inp.reads)
        return logits, torch.tensor(starts, dtype=torch.int64)

    def flush(self):
        """End of the stream -> (logits, starts) of the tail window (empty when none is due).  ValueError if the stream
        was shorter than one window."""
        if self._plan is None:
            raise ValueError('a video of 0 frames is shorter than one window of %d' % self.T)
        _, logits, starts = self._execute(self._plan.flush(self.cover_tail), self._ring, self._plan.capacity, self._device())
        return logits, torch.tensor(starts, dtype=torch.int64)

    # ---------------------------------------------------------------------------------------- whole video
    def _whole_video(self, frames: Tensor, rollout=None, boxes=None, transforms=None):
        """every window of one video, on a plan and a bank of its own -> (logits, list of starts, device)"""
        inp = self._input(frames, boxes, transforms)
        n = int(frames.shape[0])
        if n < self.T:
            raise ValueError('a video of %d frames is shorter than one window of %d' % (n, self.T))
        dev = self._device()
        plan = RingPlan(self.T, self.stride, self.capacity if self.capacity is not None else n, self.frame_batch,
                        self.window_batch)
        steps = plan.push(n, drain=False) + plan.flush(self.cover_tail)
        fetch = self._fetcher([frames], [inp], lambda first, count: [(0, first, first + count)], dev)
        _, logits, starts = self._execute(steps, None, plan.capacity, dev, fetch, inp.reads, rollout)
        return logits, starts, dev

    @staticmethod
    def _video_score(logits: Tensor, starts: List[int], dev) -> VideoScore:
        return VideoScore(logits, torch.tensor(starts, dtype=torch.int64).to(dev, non_blocking=True), logits.mean(0),
                          torch.sigmoid(logits).mean(0))

    def score(self, frames: Tensor, boxes=None, transforms=None) -> VideoScore:
        """All windows of one video.  Does not disturb a stream in progress (it never touches the stream's state).  boxes: one
        (y0, x0, h, w) per frame, int32 (N, 4), for whole frames uint8 (N, Hs, Ws, 3): each stem batch is cropped and resized
        to side x side on the device (ops.crop_resize_u8) just before the stem -- the bits of score() on those crops.  transforms: one similarity per
        frame, float32 (N, 2, 3), in the boxes' place: the crops are ops.warp_similarity_u8(frames, transforms, side)."""
        logits, starts, dev = self._whole_video(frames, boxes=boxes, transforms=transforms)
        res = self._video_score(logits, starts, dev)
        torch.cuda.current_stream(dev).synchronize()
        return res

    def explain(self, frames: Tensor, index: int = 0, boxes=None, transforms=None) -> VideoExplanation:
        """Relevance maps of one video for output `index` (DESIGN.md "Explaining whole videos"): the windows, frames and
        stem pass of score(), every window batch through the gradient-weighted attention rollout of explain.relevance
        instead of the plain forward, and the windows' maps fused per frame (ops.relevance_fuse_windows).  The model is in
        explain.relevance's state for the call and comes back as it was; a stream in progress is not disturbed.  With
        boxes or transforms (as score() takes them) the maps are in crop coordinates."""
        from . import explain as _explain
        vit = self.model.vit
        rels = []

        def rollout(x, count, hw):
            rels.append(_explain._rollouts_tokens(vit, x, count, self.T + 1, hw + 1, index))
            return rels[-1].logits

        with _explain._explaining(self.model):
            logits, starts, dev = self._whole_video(frames, rollout, boxes, transforms)
            windows = _explain.Relevance(torch.cat([r.r_s for r in rels]), torch.cat([r.r_t for r in rels]), logits)
            fused = ops.relevance_fuse_windows(windows.r_s, windows.r_t, logits, starts, int(frames.shape[0]), index)
        res = VideoExplanation(self._video_score(logits, starts, dev), windows, *fused)
        torch.cuda.current_stream(dev).synchronize()
        return res

    def render_explanation(self, frames: Tensor, explanation: VideoExplanation, boxes=None, transforms=None, which: str = 's',
                           alpha: float = 0.5, weight_frames: bool = True, lut=None, jpeg_quality: Optional[int] = None):
        """The video an analyst was given, with the heat where the face is (DESIGN.md "Pasting maps onto frames"): the frames
        of explain() -- with the same boxes or transforms -- and its result -> the frames in their own format (packed RGB or
        NV12, as the scorer's pixel_format says), uint8 on the device, with explanation.frame_s (which='s') or frame_t ('t')
        pasted onto every frame through the table that cut its crop (explain.overlay_frames, clips.paste_maps_host).  Without
        boxes or transforms the frames are the crops themselves, (N, S, S, 3), and the maps cover them.  weight_frames: frame n
        is blended with alpha_n = (frame_weight[n] / max frame_weight).clamp(0, 1) * alpha (float32, on the device, no
        synchronisation), so frames the verdict did not rest on stay nearly clean; frames no window covers have zero maps and
        come back untouched.  lut: uint8 (256, 3) RGB colours (default explain.jet_lut()).  Host frames are pinned, uploaded
        and pasted frame_batch at a time; device frames are pasted out of place.  The model is not touched.  jpeg_quality
        (1..100): the rendered RGB frames leave as JPEG files instead, a clips.JpegFiles on the device (ops.jpeg_encode_u8,
        4:2:0, a restart marker every MCU row) -- a tenth of the bytes across the host boundary; not for NV12 frames."""
        from . import clips, explain as _explain, ops
        if which not in ('s', 't'):
            raise ValueError("render_explanation: which must be 's' or 't', got %r" % (which,))
        if jpeg_quality is not None:
            if self.pixel_format == 'nv12':
                raise ValueError("render_explanation: jpeg_quality encodes packed RGB frames; pixel_format='nv12' with "
                                 'jpeg_quality is not supported')
            if isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, int) or not 1 <= jpeg_quality <= 100:
                raise ValueError('render_explanation: jpeg_quality must be an int in [1, 100], got %r' % (jpeg_quality,))
        if boxes is not None and transforms is not None:
            raise ValueError('VideoScorer: boxes and transforms are two ways to cut the same crop: pass one of them')
        nv = self.pixel_format == 'nv12'
        if boxes is None and transforms is None:
            if nv:
                raise ValueError("VideoScorer: pixel_format='nv12' needs boxes or transforms with every call")
            if check_frames(frames) != 'u8':
                raise TypeError('render_explanation pastes onto decoded uint8 frames; normalised float frames cannot take it')
            side = int(frames.shape[1])
            boxes = torch.tensor([[0, 0, side, side]] * int(frames.shape[0]), dtype=torch.int32)
        else:
            side = self.side if self.side is not None else getattr(self.model, 'crop_side', None)
        n, Hs, Ws = _whole_frames(frames, side, self.pixel_format, 'boxes' if boxes is not None else 'transforms')
        maps = explanation.frame_s if which == 's' else explanation.frame_t
        if maps.shape[0] != n or explanation.frame_weight.shape[0] != n:
            raise ValueError('render_explanation: the explanation covers %d frames, got %d' % (maps.shape[0], n))
        alpha = float(alpha)
        if not math.isfinite(alpha):
            raise ValueError('render_explanation: alpha must be finite, got %r' % (alpha,))
        tables = _explain._paste_setup(n, Hs, Ws, int(side), boxes, transforms, lut, self.pixel_format, self.yuv_matrix)
        dev = self._device()
        A, rect, table = (t.to(dev) for t in tables)
        if weight_frames:
            fw = explanation.frame_weight.to(dev)
            al = (fw / fw.max()).clamp(0, 1) * alpha
        else:
            al = torch.full((n,), alpha, dtype=torch.float32, device=dev)
        maps = maps.to(dev)
        out = torch.empty(tuple(frames.shape), dtype=torch.uint8, device=dev)
        for lo in range(0, n, self.frame_batch):
            hi = min(lo + self.frame_batch, n)
            x = frames[lo:hi]
            if not x.is_cuda:              # host frames: pinned, then copied on the current stream
                x = x.contiguous().pin_memory()
            out[lo:hi].copy_(x, non_blocking=True)
            byte_frames.paste_maps(self.pixel_format, out[lo:hi], maps[lo:hi], A[lo:hi], rect[lo:hi], table, al[lo:hi],
                                   int(side), inplace=True, checked=True)
        if jpeg_quality is not None:
            out = byte_frames.jpeg_encode_u8(out, jpeg_quality, '420', 'row')
        torch.cuda.current_stream(dev).synchronize()
        return out

    # ---------------------------------------------------------------------------------------- a set of videos
    def _check_set(self, videos, boxes, transforms=None) -> List[VideoInput]:
        """-> every video's VideoInput; every ValueError of a call about its videos and boxes (or transforms), before anything
        is launched"""
        if torch.is_tensor(videos) or not isinstance(videos, (list, tuple)) or len(videos) == 0:
            raise ValueError('videos: a non-empty list of frame tensors expected, got %s' % type(videos).__name__)
        if boxes is not None and transforms is not None:
            raise ValueError('VideoScorer: boxes and transforms are two ways to cut the same crop: pass one of them')
        if transforms is not None:
            if not isinstance(transforms, (list, tuple)) or len(transforms) != len(videos) or any(t is None for t in transforms):
                raise ValueError('transforms: one table per video expected (%d)' % len(videos))
            return [self._input(v, None, t) for v, t in zip(videos, transforms)]
        if boxes is None:
            inputs = [self._input(v, None) for v in videos]
            if len({i.reads for i in inputs}) != 1:
                raise ValueError('the videos of one call are all uint8 or all float, not both (video %d differs from video 0)'
                                 % next(v for v, i in enumerate(inputs) if i.reads != inputs[0].reads))
            sides = sorted({int(v.shape[2]) for v in videos})
            if len(sides) != 1:
                raise ValueError('the videos of one call share one crop side, got %s' % sides)
            return inputs
        if not isinstance(boxes, (list, tuple)) or len(boxes) != len(videos) or any(b is None for b in boxes):
            raise ValueError('boxes: one table per video expected (%d)' % len(videos))
        return [self._input(v, b) for v, b in zip(videos, boxes)]

    def score_videos(self, videos, boxes=None, labels=None, transforms=None) -> VideoSetScore:
        """All windows of a set of videos in one pass (DESIGN.md "Scoring a set of videos"): the windows of score(video) for
        every video, but stem batches and window batches are assembled across the videos (SetPlan), the per-video means are
        one kernel (ops.windows_reduce), and the call synchronises once.  videos: a list of tensors as score() takes them --
        all uint8 or all float, one crop side, host or device in any mix.  boxes: one table per video, for whole uint8
        frames; each video may have its own frame size.  transforms: one table of similarities per video in the boxes' place.  labels: one 0 / 1 per video -> metrics = set_metrics(logit_mean[:, 0],
        labels).  A stream in progress is not disturbed."""
        inputs = self._check_set(videos, boxes, transforms)
        plan = SetPlan([int(v.shape[0]) for v in videos], self.T, self.stride, self.cover_tail, self.frame_batch,
                       self.window_batch, self.capacity)
        V = len(videos)
        if labels is not None:
            labels = _validate_labels(labels, V)
        dev = self._device()
        # every table of the call in two uploads: the slots of the frame batches (int64, for index_copy_) and the windows' idx,
        # whose slices take the place of the steps' host tables (SetPlan names slots < capacity: they are checked)
        dslots = torch.tensor([s for st in plan.steps for s in st.slots], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        idx = torch.cat([st.idx for st in plan.steps if st.kind == 'windows']).pin_memory().to(dev, non_blocking=True)
        steps = [st if st.kind == 'frames' else st._replace(idx=idx[st.first:st.first + st.count]) for st in plan.steps]
        fetch = self._fetcher(videos, inputs, plan.pieces, dev)
        _, logits, _ = self._execute(steps, None, plan.slots_used, dev, fetch, inputs[0].reads, dslots=dslots)
        tab = torch.tensor(plan.offsets + plan.window_video, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        offsets, window_video = tab[:V + 1], tab[V + 1:]
        starts = torch.tensor(plan.starts, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        ops.check_window_offsets(plan.offsets, int(logits.shape[0]))
        logit_mean, prob_mean = ops.windows_reduce(logits, offsets, checked=True)
        metrics = None if labels is None else set_metrics(logit_mean[:, 0].contiguous(), labels)
        res = VideoSetScore(logits, window_video, starts, offsets, logit_mean, prob_mean, metrics)
        torch.cuda.current_stream(dev).synchronize()
        return res
