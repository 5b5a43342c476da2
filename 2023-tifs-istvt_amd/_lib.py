"""ctypes binding of libistvt_hip.so (C ABI declared in include/istvt_hip.h).

There is no fallback: if the library is missing or a symbol is absent, importing the ops
raises.  Build with ``python 2023-tifs-istvt_amd/build.py`` (or ``__graft_entry__.build()``).
"""
import ctypes
import os
from ctypes import c_float, c_int, c_long, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# ISTVT_LIB: another build of the same library (same-box A/B of a kernel change); it must export the same entry points
LIB_PATH = os.environ.get('ISTVT_LIB') or os.path.join(_HERE, 'libistvt_hip.so')

P, I, L, F = c_void_p, c_int, c_long, c_float


class JpegDecodeArgs(ctypes.Structure):
    """istvt_jpeg_decode_args of include/istvt_hip.h"""
    _fields_ = [('bytes', P), ('nbytes', L), ('images', P), ('images_host', P), ('segments', P), ('segments_host', P),
                ('qtabs', P), ('htabs', P), ('scratch', P), ('scratch_bytes', L), ('out', P), ('sizes', P), ('status', P),
                ('stream', P), ('n', I), ('nseg', I), ('nq', I), ('nh', I), ('Hc', I), ('Wc', I)]


class JpegEncodeArgs(ctypes.Structure):
    """istvt_jpeg_encode_args of include/istvt_hip.h"""
    _fields_ = [('frames', P), ('total', L), ('quality', P), ('header', P), ('header_bytes', L), ('scratch', P),
                ('scratch_bytes', L), ('data', P), ('capacity', L), ('offsets', P), ('status', P), ('stream', P), ('n', I),
                ('H', I), ('W', I), ('subsampling', I), ('restart_interval', I), ('dqt0', I), ('dqt1', I)]


# name -> argtypes (all return int).  Written by hand, one line per prototype of include/istvt_hip.h;
# tests/test_abi_cpu.py parses the header and compares the two type by type.
SIGNATURES = {
    'istvt_gemm': [P, L, I, P, L, I, P, L, I, I, I, P, P, L, P, I, I, I, F, P, P, I, I, P],
    'istvt_layernorm_fwd': [P, L, P, P, P, L, P, P, L, I, F, I, P],
    'istvt_layernorm_fwd_diff': [P, L, P, P, P, L, P, L, P, P, I, I, I, I, F, I, P],
    'istvt_layernorm_bwd': [P, L, P, L, P, P, P, P, L, P, L, P, P, P, P, L, L, I, I, P],
    'istvt_layernorm_bwd_ws_elems': [L, I],
    'istvt_layernorm_bwd_partial': [P, L, P, L, P, P, P, P, L, P, L, I, P, L, L, I, I, P],
    'istvt_layernorm_bwd_reduce': [P, L, L, I, P, P, P, P],
    'istvt_attn_spatial_fwd': [P, L, P, L, P, I, I, I, I, F, I, P],
    'istvt_attn_spatial_bwd': [P, L, P, P, L, P, P, P, I, I, I, I, F, I, P],
    'istvt_attn_spatial_fwd_fp8': [P, L, P, L, P, I, I, I, I, F, I, P],
    'istvt_attn_spatial_bwd_fp8': [P, L, P, P, L, P, P, P, I, I, I, I, F, I, P],
    'istvt_attn_temporal_fwd': [P, L, P, L, P, L, I, I, I, I, I, F, I, I, P],
    'istvt_attn_temporal_bwd': [P, L, P, L, P, L, P, P, I, I, I, I, I, F, I, I, P],
    'istvt_attn_spatial_relevance': [P, L, P, L, P, P, P, I, I, I, I, F, I, P],
    'istvt_attn_temporal_relevance': [P, L, P, L, P, P, I, I, I, I, I, F, I, I, P],
    'istvt_relevance_heatmap': [P, P, I, I, I, P],
    'istvt_relevance_fuse_windows': [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P],
    'istvt_relevance_overlay_u8': [P, P, P, P, P, I, I, I, I, P],
    'istvt_windows_reduce': [P, P, P, P, I, I, I, P],
    'istvt_auc_pairs': [P, P, F, P, L, P, P, I, P],
    'istvt_tokens_fwd': [P, P, P, P, P, L, I, I, I, I, I, I, P],
    'istvt_tokens_gather_fwd': [P, P, P, P, P, P, L, I, I, I, I, I, I, I, P],
    'istvt_tokens_bwd': [P, L, P, P, P, P, P, I, I, I, I, I, I, P],
    'istvt_frame_diff': [P, P, I, I, I, I, I, I, P],
    'istvt_stats_replicas': [],
    'istvt_stats_reduce': [P, I, P],
    'istvt_stats_reduce_add': [P, I, P, P],
    'istvt_bn_stats': [P, P, P, L, I, I, P],
    'istvt_bn_finalize': [P, P, ctypes.c_double, P, P, P, P, F, F, P, I, I, I, P],
    'istvt_bn_apply': [P, P, P, L, I, I, I, P],
    'istvt_bn_bwd_stats': [P, P, P, P, P, L, I, I, P],
    'istvt_bn_bwd_apply': [P, P, P, P, P, P, P, P, P, L, I, I, I, P],
    'istvt_bn_add_fwd': [P, P, P, P, P, L, I, I, P],
    'istvt_pw_bwd': [P, P, P, P, P, P, P, L, P, L, P, P, P, P, P, L, I, I, I, I, P],
    'istvt_pw_bwd_grid': [L],
    'istvt_pw_bwd_rows': [],
    'istvt_im2col_conv1': [P, P, I, I, I, P],
    'istvt_conv1_fwd': [P, P, P, I, I, I, P],
    'istvt_conv1_fwd_u8': [P, P, P, P, P, I, I, I, P],
    'istvt_conv1_wgrad': [P, P, P, P, I, I, I, P],
    'istvt_conv1_wgrad_slabs': [],
    'istvt_conv1_fwd_u8_view': [P, L, I, I, P, P, P, P, P, I, I, I, P],
    'istvt_conv1_wgrad_u8': [P, P, L, I, I, P, P, P, P, P, I, I, I, P],
    'istvt_im2col_conv1_u8': [P, L, I, I, P, P, P, P, I, I, I, P],
    'istvt_crop_resize_u8': [P, L, I, I, P, P, I, I, P],
    'istvt_crop_resize_nv12': [P, L, I, I, L, L, P, P, P, I, I, P],
    'istvt_nv12_to_rgb_u8': [P, L, I, I, L, L, P, P, I, P],
    'istvt_warp_similarity_u8': [P, L, I, I, P, P, I, I, P],
    'istvt_warp_similarity_nv12': [P, L, I, I, L, L, P, P, P, I, I, P],
    'istvt_relevance_paste_u8': [P, L, I, I, P, I, P, P, P, P, I, I, P],
    'istvt_relevance_paste_nv12': [P, L, I, I, L, L, P, I, P, P, P, P, I, I, P],
    'istvt_jpeg_roundtrip_u8': [P, L, I, I, I, P, I, P, L, P, P],
    'istvt_jpeg_decode_u8': [ctypes.POINTER(JpegDecodeArgs)],
    'istvt_jpeg_decode_split_u8': [ctypes.POINTER(JpegDecodeArgs), I],
    'istvt_jpeg_decode_indexed_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I],
    'istvt_jpeg_decode_indexed_split_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I, I, I, I],
    'istvt_batch_draw': [ctypes.POINTER(JpegDecodeArgs), I, I, I],
    'istvt_jpeg_decode_drawn_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I, I, I],
    'istvt_jpeg_decode_drawn_split_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I, I, I, I, I, I],
    'istvt_png_decode_u8': [ctypes.POINTER(JpegDecodeArgs), I],
    'istvt_png_decode_bands_u8': [ctypes.POINTER(JpegDecodeArgs), I],
    'istvt_png_decode_bank_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I],
    'istvt_png_decode_bank_drawn_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I],
    'istvt_png_decode_alone_u8': [ctypes.POINTER(JpegDecodeArgs), I],
    'istvt_png_decode_bank_alone_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I],
    'istvt_png_decode_bank_alone_drawn_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I],
    'istvt_png_decode_window_u8': [ctypes.POINTER(JpegDecodeArgs), I, I],
    'istvt_png_decode_bank_window_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I],
    'istvt_png_decode_bank_window_drawn_u8': [ctypes.POINTER(JpegDecodeArgs), I, I, I, I, I, I, I],
    'istvt_png_encode_u8': [ctypes.POINTER(JpegEncodeArgs), I, I, I, I],
    'istvt_png_encode_indexed_u8': [ctypes.POINTER(JpegEncodeArgs), I, I, I, I],
    'istvt_png_encode_alone_u8': [ctypes.POINTER(JpegEncodeArgs), I, I, I, I],
    'istvt_jpeg_bank_ingest': [ctypes.POINTER(JpegEncodeArgs), I],
    'istvt_jpeg_encode_u8': [ctypes.POINTER(JpegEncodeArgs)],
    'istvt_jpeg_encode_opt_u8': [ctypes.POINTER(JpegEncodeArgs), I, I],
    'istvt_jpeg_encode_layout_u8': [ctypes.POINTER(JpegEncodeArgs), I, I, I],
    'istvt_perturb_u8': [P, L, I, I, I, P, I, P, I, ctypes.c_ulonglong, P, L, P, P],
    'istvt_conv2_fwd': [P, P, P, P, I, I, I, P],
    'istvt_conv2_dgrad': [P, P, P, P, P, I, I, I, P],
    'istvt_conv2_wgrad': [P, P, P, P, P, I, I, I, P],
    'istvt_conv2_wgrad_slabs': [],
    'istvt_col2im_conv1': [P, P, I, I, I, P],
    'istvt_im2col3x3': [P, P, I, P, I, I, I, I, I, P],
    'istvt_col2im3x3': [P, P, P, P, I, I, I, I, I, P],
    'istvt_dwconv3x3': [P, P, P, I, I, I, I, P, I, I, P, P, I, I, P, I, I, P, P, I, P],
    'istvt_dwconv3x3_wgrad': [P, P, I, P, P, P, L, I, I, I, I, I, P],
    'istvt_dwconv3x3_wgrad_ws_elems': [I, I, I, I],
    'istvt_pool_add_fwd': [P, P, P, P, P, P, I, I, I, I, I, P],
    'istvt_pool_bwd': [P, P, P, I, I, I, I, P, P, P, P, I, P],
    'istvt_subsample2': [P, P, I, I, I, I, I, P],
    'istvt_splitk_reduce': [P, I, L, P, P],
    'istvt_wgrad_group': [I, P, P, P, P, P, P, P, I, I, P, L, P],
    'istvt_wgrad_group_splits': [I, P, P, I],
    'istvt_colsum': [P, P, L, I, L, P, L, I, P],
    'istvt_colsum_ws_elems': [L, I],
    'istvt_rows_reduce': [P, I, L, P, P],
    'istvt_cast': [P, I, P, I, L, P],
    'istvt_cast2d': [P, I, L, P, I, L, L, I, P],
    'istvt_cast_transpose': [P, L, P, L, P, L, I, I, P],
    'istvt_cast_transpose_group': [I, P, P, P, P, P, P, P, P, P],
    'istvt_relu_avgpool_fwd': [P, P, I, I, I, I, I, P],
    'istvt_relu_avgpool_bwd': [P, P, P, I, I, I, I, I, P],
    'istvt_prepend_fwd': [P, P, P, P, L, L, I, I, I, I, I, P],
    'istvt_prepend_bwd': [P, L, P, P, P, P, L, I, I, I, I, I, P],
    'istvt_prepend_bwd_ws_rows': [L, I, I],
    'istvt_seq_mean_fwd': [P, L, P, L, I, I, I, P],
    'istvt_seq_mean_bwd': [P, P, L, L, I, I, I, P],
    'istvt_dropout_fwd': [P, L, P, L, P, L, I, F, ctypes.c_ulonglong, I, P],
    'istvt_dropout_bwd': [P, L, P, P, L, L, I, F, I, P],
    'istvt_add': [P, L, P, L, P, L, L, I, I, P],
    'istvt_sgd_momentum': [P, P, P, L, F, F, F, F, I, I, I, F, P],
    'istvt_adamw': [P, P, P, P, L, F, F, F, F, F, L, I, F, P],
    'istvt_grad_norm': [P, L, F, F, I, P, L, P, P],
    'istvt_grad_norm_ws_elems': [L],
    'istvt_sgd_momentum_groups': [P, P, P, L, P, P, I, P, P, I, F, F, I, I, I, F, P, I, P],
    'istvt_adamw_groups': [P, P, P, P, L, P, P, I, P, P, I, F, F, F, L, I, F, P, I, P],
    'istvt_bce_logits': [P, L, P, I, P, F, F, I, F, L, P, P, P, P, P],
    'istvt_bce_logits_bwd': [P, P, I, P, L, P],
}

_lib = None


class IstvtLibraryError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IstvtLibraryError(
                'libistvt_hip.so not found at %s: build it with `python 2023-tifs-istvt_amd/build.py`; '
                'there is no CPU or PyTorch fallback for the ISTVT hot path' % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError as e:
                raise IstvtLibraryError('libistvt_hip.so lacks symbol %s (stale build?)' % name) from e
            fn.argtypes = argtypes
            fn.restype = c_int
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc == -2:
        msg = 'unsupported dtype'
    elif rc == -3:
        msg = 'invalid shape/argument'
    elif rc <= -1000:
        msg = 'hipError_t %d at launch' % (-rc - 1000)
    else:
        msg = 'error %d' % rc
    raise RuntimeError('%s failed: %s' % (what, msg))
