"""What the six JPEG decode entries of the library refuse before any launch (csrc/jpeg.hip, csrc/batch_draw.hip), without a
device: a valid argument block on host memory, exactly one thing made wrong per case, and -3 (ISTVT_ERR_SHAPE) back.  Nothing
was launched then, which is why host memory will do; a case an entry let through would launch on host pointers, so every case
here is one the entries refuse by their own reading of the block.

The inputs are the smallest that reach every check: a 17 x 33 file in 4:2:0 with a restart marker per MCU row (2 x 3 MCUs: 36
blocks, 2 segments) and an 8 x 8 file in 4:4:4 without markers (3 blocks, 1 segment); the bank of the two with m = 3 places;
a draw of B = 1, T = 2.  The smallest scratch each entry takes is written out below from the entry's own arithmetic -- blocks,
segments, places, seg_max, chunk_rows -- and not asked of clips.JpegBatch.scratch_bytes, clips.jpeg_split_plan or
clips.jpeg_bank_scratch_bytes, which may round up further."""
import ctypes

import pytest
import torch

ERR_SHAPE = -3
BLOCKS, NSEG, N = 36 + 3, 3, 2                      # of the batch: 8 x 8 blocks, segment rows, files
HC, WC = 17, 33
CHUNK = 16
M, SEG_MAX, BLOCK_STRIDE = 3, 2, 48                 # of the bank's call: places; most segments of a file; 36 blocks -> 2 x 24
CHUNK_ROWS = 4
B, T, DRAW_HEADER = 1, 2, 36
# column of an images row / of a segment row
SUB, MCUX, QUANT, HUFF, BLOCK0, NSEG_COL, NBLOCKS, LAYOUT = 2, 3, 5, 8, 14, 17, 18, 19
POINTERS = ('bytes', 'images', 'images_host', 'segments', 'segments_host', 'qtabs', 'htabs', 'scratch', 'out', 'sizes', 'status')


def _up16(v):
    return (v + 15) & ~15


@pytest.fixture(scope='module')
def env():
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import _lib, clips
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 256, (17, 33, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (8, 8, 3), generator=g, dtype=torch.uint8)
    files = [clips.jpeg_encode_host(a, 60, '420', 'row'), clips.jpeg_encode_host(b, 85, '444', 0)]
    batch = clips.jpeg_batch(files)
    assert batch.n == N and batch.blocks == BLOCKS and tuple(batch.segments.shape) == (NSEG, 5)
    assert batch.images[:, NSEG_COL].tolist() == [2, 1] and batch.images[:, NBLOCKS].tolist() == [36, 3]
    assert batch.sizes == [(17, 33), (8, 8)] and batch.nbytes >= 3 * CHUNK
    bank = clips.jpeg_bank(files)
    assert (bank.n, bank.nseg, bank.seg_max, bank.block_stride, bank.Hmax, bank.Wmax) == (N, NSEG, SEG_MAX, BLOCK_STRIDE, HC, WC)
    return _lib, clips, batch, bank


# ---- the smallest scratch of each entry, from its own arithmetic ---------------------------------------------------------------
def direct_min(nbytes, chunk=None):
    front = BLOCKS * 192 + 4 * NSEG                 # int16 coefficients and planes of every block | a status per segment
    if chunk is None:
        return front
    return _up16(front) + (nbytes // chunk + NSEG) * 8 * 4     # | from the next multiple of 16, the state rows


def bank_min(chunk_rows=None):
    nseg = M * SEG_MAX
    tables = _up16(M * BLOCK_STRIDE * 192 + 4 * (nseg + M))    # ... | a status per planned segment row and one per place
    need = tables + 4 * M * 20 + 4 * nseg * 5                  # | the planned images and segments
    if chunk_rows is None:
        return need
    return _up16(need) + 4 * 8 * nseg * chunk_rows            # | from the next multiple of 16, chunk_rows state rows per segment


def test_the_written_minimum_is_not_above_what_the_helpers_hand_out(env):
    """the helpers may round up, never down: a caller who takes their number is never refused"""
    _, clips, batch, bank = env
    assert direct_min(batch.nbytes) == 7500 <= batch.scratch_bytes
    assert direct_min(batch.nbytes, CHUNK) == 7504 + 32 * (batch.nbytes // 16 + 3) <= clips.jpeg_split_plan(batch, CHUNK).scratch_bytes
    assert bank_min() == 28056 <= clips.jpeg_bank_scratch_bytes(bank, M)
    split = bank.with_split(CHUNK)
    assert bank_min(split.chunk_rows) == 28064 + 192 * split.chunk_rows <= clips.jpeg_bank_scratch_bytes(split, M)


# ---- a valid block on host memory ----------------------------------------------------------------------------------------------
class Block:
    """the argument block of one call and what it points at; fields are edited in place, tables through clones"""

    def __init__(self, env, kind, scratch_bytes):
        _lib, _, batch, bank = env
        src = batch if kind == 'direct' else bank
        n_out = N if kind == 'direct' else M
        room = torch.zeros(scratch_bytes + 48, dtype=torch.uint8)
        self.scratch = room[(-room.data_ptr()) % 16:]
        self.out = torch.zeros(n_out * HC * WC * 3, dtype=torch.uint8)
        self.sizes = torch.zeros((n_out, 2), dtype=torch.int32)
        self.status = torch.zeros(n_out, dtype=torch.int32)
        self.images, self.segments = src.images.clone(), src.segments.clone()
        self.index = torch.tensor([1, 0, 1], dtype=torch.int32)
        self.draw = torch.zeros(DRAW_HEADER + B * T, dtype=torch.int32)
        self.data = src.data
        second = {'direct': self.images, 'bank': self.index, 'drawn': self.draw}[kind]
        assert self.scratch.data_ptr() % 16 == 0
        self.args = _lib.JpegDecodeArgs(
            bytes=src.data.data_ptr(), nbytes=src.nbytes, images=self.images.data_ptr(), images_host=second.data_ptr(),
            segments=self.segments.data_ptr(), segments_host=self.segments.data_ptr() if kind == 'direct' else None,
            qtabs=src.qtabs.data_ptr(), htabs=src.htabs.data_ptr(), scratch=self.scratch.data_ptr(), scratch_bytes=scratch_bytes,
            out=self.out.data_ptr(), sizes=self.sizes.data_ptr(), status=self.status.data_ptr(), stream=None, n=src.n,
            nseg=int(src.segments.shape[0]), nq=int(src.qtabs.shape[0]), nh=int(src.htabs.shape[0]), Hc=HC, Wc=WC)


def _field(name, value):
    return lambda blk, extra: setattr(blk.args, name, value(blk) if callable(value) else value)


def _cell(table, row, col, value):
    def fn(blk, extra):
        t = getattr(blk, table)
        t[row, col] = value(t) if callable(value) else value
    return fn


def _extra(name, value):
    return lambda blk, extra: extra.__setitem__(name, value)


def _misalign(blk, extra):
    blk.args.scratch = blk.scratch.data_ptr() + 8


def _swap_byte_ranges(blk, extra):
    """segments 0 and 1 keep their image and MCUs and trade their bytes: each row is fine, their order is not"""
    s = blk.segments
    s[0, 1], s[0, 2], s[1, 1], s[1, 2] = int(s[1, 1]), int(s[1, 2]), int(s[0, 1]), int(s[0, 2])
    assert int(s[1, 1]) < int(s[0, 2])


def _direct_cases(split):
    c = [('%s = NULL' % p, _field(p, None)) for p in POINTERS]
    c += [('n = 0', _field('n', 0)), ('nseg = n - 1', _field('nseg', N - 1)), ('nq = 0', _field('nq', 0)),
          ('nh = 0', _field('nh', 0)), ('nbytes = -1', _field('nbytes', -1)),
          ('Hc = 0', _field('Hc', 0)), ('Hc = 16385', _field('Hc', 16385)), ('Wc = 0', _field('Wc', 0)),
          ('Wc = 16385', _field('Wc', 16385)), ('Hc one below the tallest image', _field('Hc', HC - 1)),
          ('images: sub = 3', _cell('images', 0, SUB, 3)),
          ('images: layout code 1 (4:2:2) with sub = 1', _cell('images', 1, LAYOUT, 1)),
          ('images: mcux + 1', _cell('images', 0, MCUX, lambda t: int(t[0, MCUX]) + 1)),
          ('images: a quant index = nq', lambda blk, extra: blk.images.__setitem__((0, QUANT), blk.args.nq)),
          ('images: a Huffman index = nh', lambda blk, extra: blk.images.__setitem__((0, HUFF), blk.args.nh)),
          ('images: block0 + 1', _cell('images', 1, BLOCK0, 37)),
          ('images: nseg = 0 for an image', _cell('images', 1, NSEG_COL, 0)),
          ('images: nblocks + 1', _cell('images', 0, NBLOCKS, 37)),
          ('segments: wrong file index', _cell('segments', 0, 0, 1)),
          ('segments: begin > end', _cell('segments', 0, 1, lambda t: int(t[0, 2]) + 1)),
          ('segments: end = nbytes + 1', lambda blk, extra: blk.segments.__setitem__((2, 2), blk.args.nbytes + 1)),
          ('segments: wrong first MCU', _cell('segments', 1, 3, 4)),
          ('segments: mcus = 0', _cell('segments', 2, 4, 0)),
          ('segments: MCU counts that do not sum', _cell('segments', 1, 4, 4)),
          ('nseg one more than the rows used', _field('nseg', NSEG + 1)),
          ('scratch misaligned by 8', _misalign),
          ('out overlapping bytes', _field('out', lambda blk: blk.data.data_ptr()))]
    if split:
        c += [('chunk_bytes = 15', _extra('chunk_bytes', 15)), ('segment rows whose bytes are out of order', _swap_byte_ranges)]
    return c


def test_direct_entries_refuse_before_any_launch(env):
    _lib, _, batch, _ = env
    lib = _lib.lib()
    assert batch.segments[1, 3:].tolist() == [3, 3] and batch.images[1, BLOCK0] == 36
    for split in (False, True):
        need = direct_min(batch.nbytes, CHUNK if split else None)

        def call(blk, extra):
            if split:
                return lib.istvt_jpeg_decode_split_u8(ctypes.byref(blk.args), extra['chunk_bytes'])
            return lib.istvt_jpeg_decode_u8(ctypes.byref(blk.args))
        which = 'istvt_jpeg_decode_split_u8' if split else 'istvt_jpeg_decode_u8'
        assert (lib.istvt_jpeg_decode_split_u8(None, CHUNK) if split else lib.istvt_jpeg_decode_u8(None)) == ERR_SHAPE, which
        for name, fault in _direct_cases(split):
            blk, extra = Block(env, 'direct', need), {'chunk_bytes': CHUNK}
            fault(blk, extra)
            assert call(blk, extra) == ERR_SHAPE, '%s: %s' % (which, name)
        short = [need - 1] + ([direct_min(batch.nbytes)] if split else [])     # split: the plain entry's scratch is short too
        for scratch_bytes in short:
            blk = Block(env, 'direct', need)
            blk.args.scratch_bytes = scratch_bytes
            assert call(blk, {'chunk_bytes': CHUNK}) == ERR_SHAPE, '%s: scratch_bytes = %d' % (which, scratch_bytes)


def _bank_cases(split):
    c = [('%s = NULL' % p, _field(p, None)) for p in POINTERS if p != 'segments_host']
    c += [('m = 0', _extra('m', 0)), ('seg_max = 0', _extra('seg_max', 0)),
          ('block_stride = 0', _extra('block_stride', 0)), ('block_stride = 23', _extra('block_stride', 23)),
          ('block_stride = 25', _extra('block_stride', 25)),
          ('nbytes = 2^31', _field('nbytes', 2 ** 31)),
          ('Hmax = 0', _extra('Hmax', 0)), ('Hmax = Hc + 1', _extra('Hmax', HC + 1)), ('Wmax = Wc + 1', _extra('Wmax', WC + 1)),
          ('Hc = 16385', _field('Hc', 16385)),
          ('scratch misaligned by 8', _misalign),
          ('out overlapping bytes', _field('out', lambda blk: blk.data.data_ptr()))]
    if split:
        c += [('chunk_bytes = 15', _extra('chunk_bytes', 15)), ('chunk_rows = 0', _extra('chunk_rows', 0)),
              ('chunk_rows = 257', _extra('chunk_rows', 257))]
    return c


def test_indexed_entries_refuse_before_any_launch(env):
    _lib, _, _, bank = env
    lib = _lib.lib()
    for split in (False, True):
        need = bank_min(CHUNK_ROWS if split else None)
        scalars = {'m': M, 'seg_max': SEG_MAX, 'block_stride': BLOCK_STRIDE, 'Hmax': HC, 'Wmax': WC, 'chunk_bytes': CHUNK,
                   'chunk_rows': CHUNK_ROWS, 'seg_bytes_max': -1}

        def call(a, e):
            head = (e['m'], e['seg_max'], e['block_stride'], e['Hmax'], e['Wmax'])
            if split:
                return lib.istvt_jpeg_decode_indexed_split_u8(a, *head, e['chunk_bytes'], e['chunk_rows'], e['seg_bytes_max'])
            return lib.istvt_jpeg_decode_indexed_u8(a, *head)
        which = 'istvt_jpeg_decode_indexed_split_u8' if split else 'istvt_jpeg_decode_indexed_u8'
        assert call(None, scalars) == ERR_SHAPE, which
        for name, fault in _bank_cases(split):
            blk, extra = Block(env, 'bank', need), dict(scalars)
            fault(blk, extra)
            assert call(ctypes.byref(blk.args), extra) == ERR_SHAPE, '%s: %s' % (which, name)
        short = [need - 1] + ([bank_min()] if split else [])
        for scratch_bytes in short:
            blk = Block(env, 'bank', need)
            blk.args.scratch_bytes = scratch_bytes
            assert call(ctypes.byref(blk.args), scalars) == ERR_SHAPE, '%s: scratch_bytes = %d' % (which, scratch_bytes)


def test_drawn_entries_refuse_before_the_draw(env):
    """only what is refused before the draw is launched: the draw's own scalars"""
    _lib, _, _, _ = env
    lib = _lib.lib()
    need = bank_min(CHUNK_ROWS)
    tail = (SEG_MAX, BLOCK_STRIDE, HC, WC)
    cases = [('a null block', None, B, T, DRAW_HEADER + B * T), ('B = 0', 1, 0, T, DRAW_HEADER + B * T),
             ('T = 0', 1, B, 0, DRAW_HEADER + B * T), ('block_ints = BD_HEADER_INTS + B * T - 1', 1, B, T, DRAW_HEADER + B * T - 1)]
    assert lib.istvt_jpeg_decode_drawn_u8(None, B, T, DRAW_HEADER + B * T, *tail) == ERR_SHAPE
    assert lib.istvt_jpeg_decode_drawn_split_u8(None, B, T, DRAW_HEADER + B * T, *tail, CHUNK, CHUNK_ROWS, -1) == ERR_SHAPE
    for name, block, b, t, ints in cases:
        blk = Block(env, 'drawn', need)
        if block is None:
            blk.args.images_host = None
        a = ctypes.byref(blk.args)
        assert lib.istvt_jpeg_decode_drawn_u8(a, b, t, ints, *tail) == ERR_SHAPE, name
        assert lib.istvt_jpeg_decode_drawn_split_u8(a, b, t, ints, *tail, CHUNK, CHUNK_ROWS, -1) == ERR_SHAPE, name
