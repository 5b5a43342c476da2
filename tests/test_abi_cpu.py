"""The C ABI has one declaration, include/istvt_hip.h.  The kernels are compiled against it (a definition that disagrees does
not build); this file ties the third copy to it, the ctypes table and structures of istvt_amd._lib, type by type, and the
Python constants that restate a #define.  tests/abi_header.py reads the header."""
import ctypes
import os
import re
import subprocess

import pytest

import abi_header as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'istvt_hip.h')
BLOCK_NAMES = {'istvt_jpeg_decode_args': 'JpegDecodeArgs', 'istvt_jpeg_encode_args': 'JpegEncodeArgs'}


@pytest.fixture(scope='module')
def lib_module():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


@pytest.fixture(scope='module')
def text():
    with open(HEADER) as fh:
        return fh.read()


@pytest.fixture(scope='module')
def blocks(lib_module):
    return {c_name: getattr(lib_module, py_name) for c_name, py_name in BLOCK_NAMES.items()}


def _llvm_tool(name):
    from istvt_amd import build
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC))), 'llvm', 'bin', name)
    assert os.path.exists(path), '%s: the ROCm toolchain that built the library has no %s' % (path, name)
    return path


def test_every_prototype_equals_the_table(lib_module, text, blocks):
    declared = H.prototypes(text)
    assert len(declared) >= 96, len(declared)                   # a pattern that matches nothing cannot pass
    # every `int istvt_` of the header is one of them: none is left out because the pattern could not read it
    assert len(declared) == len(re.findall(r'\bint\s+istvt_\w+\s*\(', H.strip_comments(text)))
    assert H.signature_mismatches(text, lib_module.SIGNATURES, blocks) == []
    for name, params in declared.items():                       # (what the comparison above compared, spelled out)
        assert lib_module.SIGNATURES[name] == [H.ctype_of(t, blocks, name) for t, _ in params], name
    r = subprocess.run([_llvm_tool('llvm-objdump'), '-T', lib_module.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if re.search(r'\sistvt_\w+$', ln) and '*UND*' not in ln}
    assert set(lib_module.SIGNATURES) == set(declared) == exported
    lib = lib_module.lib()                                      # binds every name of the table or raises
    assert all(getattr(lib, name).argtypes == argtypes for name, argtypes in lib_module.SIGNATURES.items())


def test_every_ctypes_structure_equals_its_struct(lib_module, text, blocks):
    bound = {name: cls for name, cls in vars(lib_module).items()
             if isinstance(cls, type) and issubclass(cls, ctypes.Structure) and cls is not ctypes.Structure}
    assert set(bound) == set(BLOCK_NAMES.values())              # a new Structure gets its line in BLOCK_NAMES
    for c_name, cls in blocks.items():
        assert H.struct_mismatches(text, c_name, cls, blocks) == [], c_name
        # the prototype that takes the block takes a pointer to exactly this struct
        entry = c_name.replace('_args', '_u8')
        assert H.prototypes(text)[entry] == [('const %s*' % c_name, 'a')]
        assert lib_module.SIGNATURES[entry] == [ctypes.POINTER(cls)]


def test_layout_as_a_c_compiler_sees_it(lib_module, text, blocks, tmp_path):
    """The header compiles as plain C99 without a warning, and its structs lie where ctypes and the Python side put them."""
    from istvt_amd import loss, ops
    names = list(BLOCK_NAMES) + ['istvt_loss_meter', 'istvt_step_info']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text(H.layout_program(text, names))
    r = subprocess.run([_llvm_tool('clang'), '-std=c99', '-Wall', '-Wpedantic', '-Werror', '-I', os.path.dirname(HEADER),
                        str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = {key: int(value) for key, value in (ln.split() for ln in r.stdout.splitlines())}
    want = {}
    for c_name, cls in blocks.items():
        want[c_name] = ctypes.sizeof(cls)
        want.update({'%s.%s' % (c_name, f[0]): getattr(cls, f[0]).offset for f in cls._fields_})
    # the meter: ten 8-byte words (loss.py reads it as ten int64 / float64 words), the counts in words 2..8
    meter = [field for _, field, _ in H.structs(text)['istvt_loss_meter']]
    assert len(meter) == ops.METER_WORDS == 10 and tuple(meter[2:9]) == loss.METER_COUNTS
    assert meter[:2] == ['loss_sum', 'batch_loss_sum']
    want['istvt_loss_meter'] = 80
    want.update({'istvt_loss_meter.' + field: 8 * i for i, field in enumerate(meter)})
    # the step-info block: eight 32-bit words (parallel.py allocates 8 int32 and reads words 0, 3 and 4)
    want['istvt_step_info'] = 32
    want.update({'istvt_step_info.' + field: 4 * i for i, field in
                 enumerate(('total_norm', 'scale', 'finite', 'applied_steps', 'skipped_steps', 'reserved'))})
    assert got == want


def test_python_constants_equal_the_defines(lib_module, text):
    import torch
    from istvt_amd import _common, clips, ops
    d = H.defines(text)
    assert d['ISTVT_JPEG_IMAGE_INTS'] == clips.JPEG_IMAGE_INTS == 20
    assert d['ISTVT_JPEG_HUFF_INTS'] == clips.JPEG_HUFF_INTS == 288
    assert d['ISTVT_JPEG_IDCT_BLOCKS'] == clips.JPEG_IDCT_BLOCKS == 24
    assert d['ISTVT_JPEG_SEGMENT_INTS'] == 5
    assert d['ISTVT_G256_MIN'] == _common.G256_MIN == 64
    # the tables clips.jpeg_batch really packs have rows of those widths
    x = torch.arange(24 * 40 * 3, dtype=torch.int64).mul(37).remainder(256).to(torch.uint8).reshape(24, 40, 3)
    batch = clips.jpeg_batch([clips.jpeg_encode_host(x, 75, '420', 'row')])
    assert batch.images.shape[1] == d['ISTVT_JPEG_IMAGE_INTS'] and batch.segments.shape[1] == d['ISTVT_JPEG_SEGMENT_INTS']
    assert batch.htabs.shape[1] == d['ISTVT_JPEG_HUFF_INTS'] and batch.segments.shape[0] > 1
    assert batch.groups == -(-batch.blocks // d['ISTVT_JPEG_IDCT_BLOCKS'])
    # the codes loss.py passes through ops.bce_logits
    assert ops.BCE_TARGET_KINDS == {torch.float32: d['ISTVT_TARGET_F32'], torch.int64: d['ISTVT_TARGET_I64'],
                                    torch.int32: d['ISTVT_TARGET_I32'], torch.uint8: d['ISTVT_TARGET_U8']}
    assert ops.BCE_REDUCTIONS == {'none': d['ISTVT_REDUCE_NONE'], 'mean': d['ISTVT_REDUCE_MEAN'], 'sum': d['ISTVT_REDUCE_SUM']}
    assert (d['ISTVT_F32'], d['ISTVT_BF16']) == (_common._DT[torch.float32], _common._DT[torch.bfloat16])
    # the return codes _lib.check words
    assert (d['ISTVT_OK'], d['ISTVT_ERR_DTYPE'], d['ISTVT_ERR_SHAPE'], d['ISTVT_ERR_LAUNCH']) == (0, -2, -3, -4)
    lib_module.check(d['ISTVT_OK'], 'x')
    for code, words in ((d['ISTVT_ERR_DTYPE'], 'unsupported dtype'), (d['ISTVT_ERR_SHAPE'], 'invalid shape/argument'),
                        (-1003, 'hipError_t 3 at launch'), (d['ISTVT_ERR_LAUNCH'], 'error -4')):
        with pytest.raises(RuntimeError, match='x failed: ' + words):
            lib_module.check(code, 'x')


def _replace(text, old, new):
    """the header with `old`, which must stand in it exactly once, replaced"""
    assert text.count(old) == 1, old
    return text.replace(old, new)


def test_the_check_can_fail(lib_module, text, blocks):
    table = lib_module.SIGNATURES
    # a long and an int parameter exchanged
    doctored = _replace(text, 'int istvt_splitk_reduce(const float* ws, int splits, long n,',
                        'int istvt_splitk_reduce(const float* ws, long n, int splits,')
    assert H.signature_mismatches(doctored, table, blocks) == [
        'istvt_splitk_reduce: argument 1 (n) is declared long = c_long, the table has c_int',
        'istvt_splitk_reduce: argument 2 (splits) is declared int = c_int, the table has c_long']
    # a pointer turned into a long
    doctored = _replace(text, 'int istvt_stats_reduce(double* acc,', 'int istvt_stats_reduce(long acc,')
    assert H.signature_mismatches(doctored, table, blocks) == [
        'istvt_stats_reduce: argument 0 (acc) is declared long = c_long, the table has c_void_p']
    # two fields of a struct exchanged
    doctored = _replace(_replace(_replace(text, 'long total;', '\0'), 'const int* quality;', 'long total;'), '\0',
                        'const int* quality;')
    assert H.signature_mismatches(doctored, table, blocks) == []
    assert H.struct_mismatches(doctored, 'istvt_jpeg_encode_args', blocks['istvt_jpeg_encode_args'], blocks) == [
        'istvt_jpeg_encode_args: field 1 is declared c_void_p quality, JpegEncodeArgs has c_long total',
        'istvt_jpeg_encode_args: field 2 is declared c_long total, JpegEncodeArgs has c_void_p quality']
    assert H.struct_mismatches(doctored, 'istvt_jpeg_decode_args', blocks['istvt_jpeg_decode_args'], blocks) == []
    # a dropped parameter, a dropped entry point and a type outside the table are reported too
    doctored = _replace(text, 'int istvt_stats_reduce(double* acc, int C,', 'int istvt_stats_reduce(double* acc,')
    assert H.signature_mismatches(doctored, table, blocks) == ['istvt_stats_reduce: 2 parameters declared, 3 in the table']
    doctored = _replace(text, 'int istvt_stats_replicas(void);', '')
    assert H.signature_mismatches(doctored, table, blocks) == ['istvt_stats_replicas: in the table, not declared']
    with pytest.raises(H.AbiError, match='istvt_pw_bwd_grid.*short'):
        H.signature_mismatches(_replace(text, 'int istvt_pw_bwd_grid(long M);', 'int istvt_pw_bwd_grid(short M);'), table, blocks)
