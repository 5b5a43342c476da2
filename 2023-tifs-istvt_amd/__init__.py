"""istvt_amd — MI355X-native (gfx950) implementation of the ISTVT video-clip hot path.

The directory name (``2023-tifs-istvt_amd``) is not a valid Python identifier; load the
package through ``istvt_pkg.load()`` at the repo root, which registers it as ``istvt_amd``.

Layout
    csrc/          hand-written HIP kernels + the C ABI (libistvt_hip.so, see include/istvt_hip.h)
    _lib.py        ctypes binding of the C ABI (fails loudly when the library is missing)
    _common.py     dtype codes, stream handle, row-strided layout, cast: what ops.py and weights.py both stand on
    weights.py     the one cache of every copy derived from a parameter (operands, transposes, stem layouts)
    ops.py         tensor-level launch wrappers (shape checks, stream, dtype codes)
    frames.py      the launch wrappers of the routines on decoded uint8 frames (crops, warps, NV12, JPEG, perturbations, the
                   relevance paste) behind one argument front end; ops re-exports them
    functional.py  torch.autograd.Function glue (autograd plumbing only)
    network/       nn.Modules mirroring the reference's constructor/forward signatures
    parallel.py    data-parallel gradient bucket (one RCCL all-reduce per step)
    explain.py     relevance maps (gradient-weighted attention rollout)
    video.py       whole-video scoring: uint8 frames, sliding windows, the stem once per frame
    loss.py        the criterion: BCE with logits, accuracy and epoch meters in one launch
"""
__all__ = ['ops', 'functional', 'network', 'parallel', 'explain', 'video', 'loss']
