// The checks and the inflate launch of the two band-wise PNG decoders (csrc/png_bands.hip, csrc/png_bank.hip), for
// csrc/png_alone.hip: its entries refuse what those refuse and launch the same inflate kernels, which stay where they compile
// as they did.  Host functions of the library, not of its C ABI.
#pragma once
#include "istvt_hip.h"
#include "png_bank.h"

// istvt_png_decode_bands_u8: every check of the block and of its host tables, the scratch included
bool png_bands_args_ok(const istvt_jpeg_decode_args* a, int raw_stride);
// ... and of them those that ask nothing of the canvas or the scratch: the pointers, counts and alignment of the block, every
// image row against the bytes, the band rows against the image rows (csrc/png_window.hip decodes into a canvas of its own)
bool png_bands_tables_ok(const istvt_jpeg_decode_args* a);
// ... and png_inflate_bands_kernel, one wave per band row; the band statuses are nseg ints behind n * raw_stride bytes of scratch
int png_bands_inflate_launch(const istvt_jpeg_decode_args* a, int raw_stride);

// istvt_png_decode_bank_u8: every check of the scalars and pointers -> *call, what the kernels compare the rows with
bool png_bank_args_ok(const istvt_jpeg_decode_args* a, int m, int band_max, int raw_stride, PkCall* call);
// ... and png_bank_inflate_kernel, m * band_max waves; the band statuses are m * band_max ints behind m * raw_stride bytes
int png_bank_inflate_launch(const istvt_jpeg_decode_args* a, int m, const PkCall& call);
