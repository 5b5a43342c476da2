"""A small DEFLATE emitter for the PNG tests (no tests in here): a bit writer, stored blocks, fixed-Huffman blocks and dynamic
blocks from caller-given code lengths, with explicit (length, distance) matches -- so that tests reach what zlib never writes.
And the shared cases of tests/test_png_cpu.py and tests/test_png_gpu.py: the images of the filter test, the special streams
and the damaged streams on a 100 x 111 RGB image (33 400 filtered bytes, just past one 32 KiB window).

A block's items: an int is a literal; (L, D) is a match; ('sym', s) a bare literal/length symbol."""
import zlib

import numpy as np

LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_LENS = [4] * 13 + [5] * 6                 # a complete code over all 19 code-length symbols
FLAT_LIT = [8] * 226 + [9] * 60              # a complete code over the 286 literal/length symbols
FLAT_DIST = [4] * 2 + [5] * 28               # ... over the 30 distance symbols

H, W = 100, 111                              # the image of the special and the damaged streams
STRIDE = 1 + 3 * W
TOTAL = H * STRIDE


class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, n):                 # n bits, least significant first (header fields, extra bits)
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):                 # a Huffman code, its first bit first
        for i in range(n - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        assert self.n < 8
        return bytes(self.out) + (bytes([self.acc]) if self.n else b'')


def canonical(lens):
    """{symbol: (code, length)} by RFC 1951 3.2.2; for an over-subscribed set the codes mean nothing (only headers use them)"""
    count = [0] * 16
    for v in lens:
        count[v] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, v in enumerate(lens):
        if v:
            out[s] = (nxt[v], v)
            nxt[v] += 1
    return out


def length_symbol(L):
    s = max(i for i in range(29) if LBASE[i] <= L) if L < 258 else 28
    return 257 + s, LEXT[s], L - LBASE[s]


def distance_symbol(D):
    s = max(i for i in range(30) if DBASE[i] <= D)
    return s, DEXT[s], D - DBASE[s]


def stored(w: Bits, data, last, nlen=None):
    w.put(1 if last else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    w.out += bytes(data)


def _rle(lens):
    """the code-length symbols of a run of lengths, greedy: 18 / 17 for zeros, 16 for repeats, wherever the run lies"""
    items, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            k = min(run, 138)
            items.append((18, 7, k - 11) if k >= 11 else (17, 3, k - 3))
            i += k
        elif v != 0 and run >= 4:
            k = min(run - 1, 6)
            items += [(v, 0, 0), (16, 2, k - 3)]
            i += 1 + k
        else:
            items.append((v, 0, 0))
            i += 1
    return items


def coded(w: Bits, items, last, lit_lens=None, dist_lens=None, rle=False, eob=True):
    """a fixed block (no lengths given) or a dynamic one from lit_lens (257..286 lengths) and dist_lens (1..30)"""
    w.put(1 if last else 0, 1)
    if lit_lens is None:
        w.put(1, 2)
        lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
    else:
        w.put(2, 2)
        w.put(len(lit_lens) - 257, 5)
        w.put(len(dist_lens) - 1, 5)
        w.put(19 - 4, 4)
        for s in CL_ORDER:
            w.put(CL_LENS[s], 3)
        cl = canonical(CL_LENS)
        both = list(lit_lens) + list(dist_lens)
        for s, n, extra in (_rle(both) if rle else [(v, 0, 0) for v in both]):
            w.code(*cl[s])
            w.put(extra, n)
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for it in list(items) + ([('sym', 256)] if eob else []):
        if isinstance(it, int):
            w.code(*lit[it])
        elif it[0] == 'sym':
            w.code(*lit[it[1]])
        else:
            s, n, extra = length_symbol(it[0])
            w.code(*lit[s])
            w.put(extra, n)
            s, n, extra = distance_symbol(it[1])
            w.code(*dist[s])
            w.put(extra, n)


def play(items, out=None):
    """what a decoder makes of the items"""
    out = bytearray() if out is None else out
    for it in items:
        if isinstance(it, int):
            out.append(it)
        elif it[0] != 'sym':
            for _ in range(it[0]):
                out.append(out[-it[1]])
    return out


def lit(i):
    """byte i of the base image's filtered rows: filter type 0 in front of every row"""
    return 0 if i % STRIDE == 0 else (i * 7 + (i >> 5) * 13 + (i * i >> 9)) & 255


def lits(a, b):
    return [lit(i) for i in range(a, b)]


def zlib_wrap(raw, data=b''):
    return b'\x78\x9c' + raw + zlib.adler32(bytes(data)).to_bytes(4, 'big')


def special_streams():
    """[(name, raw DEFLATE bytes, the TOTAL bytes they inflate to)]: valid streams zlib would not write"""
    cases = []

    def add(name, w, parts):
        data = bytes(play([it for p in parts for it in p]))
        assert len(data) == TOTAL and all(data[r * STRIDE] <= 4 for r in range(H)), name
        cases.append((name, w.bytes(), data))

    # a match of length 258 at distance 32768, then at distance 1, then (3, 2): one fixed block
    items = lits(0, 32768) + [(258, 32768)] + lits(33026, 33066 + 1) + [(258, 1), (3, 2)]
    items += lits(len(play(items)), TOTAL)
    w = Bits()
    coded(w, items, True)
    add('len258_dist32768', w, [items])
    # distance 1, length 258 right behind a filter byte
    items = lits(0, 3 * STRIDE + 1) + [(258, 1)] + lits(3 * STRIDE + 259, TOTAL)
    w = Bits()
    coded(w, items, True)
    add('dist1_len258', w, [items])
    # a match that reaches back across a block boundary (and across a stored block)
    a, b, c = lits(0, 5000), lits(5000, 5100), [(200, 5100), (17, 90)]
    c += lits(5100 + 217, TOTAL)
    w = Bits()
    coded(w, a, False)
    stored(w, b, False)
    coded(w, c, True)
    add('match_across_blocks', w, [a, b, c])
    # an empty stored block between two coded blocks, entered at a bit position that is not a byte's first
    a, c = lits(0, 777), lits(777, TOTAL)
    w = Bits()
    coded(w, a, False)
    assert w.n != 0
    stored(w, b'', False)
    coded(w, c, True)
    add('empty_stored_unaligned', w, [a, c])
    # an empty final fixed block
    a = lits(0, TOTAL)
    w = Bits()
    coded(w, a, False, FLAT_LIT, FLAT_DIST)
    coded(w, [], True)
    add('empty_final_fixed', w, [a])
    # a dynamic block with 15-bit codes: length symbols 261 and 262 (L = 7, 8) have them
    deep = [8] * 255 + [9, 10, 11, 12, 13, 14, 15, 15]
    items = lits(0, 400) + [(7, 334), (8, 5), (7, 1)]
    items += [min(v, 255) for v in lits(len(play(items)), TOTAL)]
    w = Bits()
    coded(w, items, True, deep, FLAT_DIST)
    add('dynamic_15bit', w, [items])
    # a dynamic block with a single distance code (one bit, distance 1)
    items = lits(0, 2 * STRIDE + 1) + [(100, 1), (3, 1)] + lits(2 * STRIDE + 104, TOTAL)
    w = Bits()
    coded(w, items, True, FLAT_LIT, [1])
    add('dynamic_single_distance', w, [items])
    # a dynamic block with no match and one zero-length distance code
    items = lits(0, TOTAL)
    w = Bits()
    coded(w, items, True, [8] * 254 + [9] * 4, [0])
    add('dynamic_no_distance', w, [items])
    # a repeat code that runs from the literal/length lengths into the distance lengths: ten zeros as one symbol 17
    lens, dl = [8] * 232 + [9] * 48 + [0] * 6, [0, 0, 0, 0, 1, 1]
    assert (17, 3, 7) in _rle(lens + dl)
    items = lits(0, 1010) + [(40, 5), (9, 8)] + lits(1059, TOTAL)
    w = Bits()
    coded(w, items, True, lens, dl, rle=True)
    add('repeat_across_sets', w, [items])
    return cases


def damaged_streams():
    """[(name, raw DEFLATE bytes, the status every decoder must give)]: one per kind of damage, and one stream that zlib
    decodes and RFC 1951 does not allow (an incomplete literal/length set of a single one-bit code)"""
    rows = bytes(lits(0, TOTAL))
    cases = []

    def deflate(level, strategy=0):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        return z.compress(rows) + z.flush()
    cases.append(('truncated_in_symbol', deflate(9)[:3001], 1))
    cases.append(('truncated_in_stored', deflate(0)[:20000], 1))
    w = Bits()
    coded(w, lits(0, 500), False)
    w.put(1, 1)
    w.put(3, 2)
    cases.append(('block_type_3', w.bytes() + bytes(8), 2))
    w = Bits()
    coded(w, lits(0, 500), False)
    stored(w, lits(500, 600), True, nlen=(100 ^ 0xffff) ^ 0x0100)
    cases.append(('nlen_wrong', w.bytes(), 2))
    w = Bits()
    coded(w, [], True, [8] * 227 + [9] * 59, FLAT_DIST, eob=False)          # one length-8 code too many
    cases.append(('oversubscribed', w.bytes() + bytes(8), 3))
    w = Bits()
    coded(w, [], True, [8] * 225 + [9] * 61, FLAT_DIST, eob=False)          # half a length-8 code unused
    cases.append(('incomplete_literal_tree', w.bytes() + bytes(8), 3))
    w = Bits()                                                              # zlib takes this one: the decoders here do not
    coded(w, lits(0, TOTAL), False)
    coded(w, [], True, [0] * 256 + [1], [0])                                # the end-of-block code alone, one bit long
    assert zlib.decompress(w.bytes(), -15) == rows
    cases.append(('one_code_literal_tree', w.bytes(), 3))
    w = Bits()
    coded(w, lits(0, 700) + [(5, 701)], True)
    cases.append(('distance_past_start', w.bytes(), 4))
    w = Bits()
    coded(w, lits(0, TOTAL) + [7], True)
    cases.append(('one_literal_too_many', w.bytes(), 5))
    w = Bits()
    coded(w, lits(0, 30000), False)
    coded(w, lits(30000, TOTAL - 1), True)
    cases.append(('final_block_one_short', w.bytes(), 5))
    bad = bytearray(rows)
    bad[64 * STRIDE] = 5
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    cases.append(('filter_byte_5', z.compress(bytes(bad)) + z.flush(), 6))
    return cases


SIZES = ((1, 1), (1, 70), (66, 1), (65, 67), (3, 5), (130, 9))
CHANNELS = (1, 3, 4)
KINDS = ((0, 0), (6, 4), (9, 0), (6, 3), (6, 2))          # (level, strategy): stored, Z_FIXED, level 9, Z_RLE, Z_HUFFMAN_ONLY


def pattern(h, w, ch, seed):
    """a smooth pattern plus small noise from a seeded generator -> uint8 (h, w) or (h, w, ch)"""
    rng = np.random.default_rng(seed)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(ch), indexing='ij')
    v = 128 + 90 * np.sin(0.11 * x + 0.07 * y + c) + 30 * np.cos(0.05 * x * (c + 1) - 0.13 * y) + rng.integers(-6, 7, (h, w, ch))
    v = np.clip(v, 0, 255).astype(np.uint8)
    return v[:, :, 0] if ch == 1 else v


def _pairs():
    """a de Bruijn sequence B(5, 2): read as a cycle, every ordered pair of the five filter types occurs once"""
    k, n, a, seq = 5, 2, [0] * 10, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    assert len({(seq[i], seq[(i + 1) % 25]) for i in range(25)}) == 25
    return seq


PAIRS = _pairs()


def filter_types(h, k):
    """the filter type of every row of file k: the pair cycle, shifted by k -- in a file of 26 rows or more every type follows
    every type, and on any one row the files k, k + 1, ... k + 4 have the five types"""
    return [(PAIRS[r % 25] + k) % 5 for r in range(h)]


def filter_files(encode):
    """the files of the filter test: every size x colour type, and the tallest size twice more so that row 128 sees every
    type; the stream kinds in turn -> [(name, file bytes)]; encode is clips.png_encode_host"""
    files = []
    for h, w, ch in [(h, w, ch) for h, w in SIZES for ch in CHANNELS] + [(130, 9, 3), (130, 9, 4)]:
        k = len(files)
        level, strategy = KINDS[k % len(KINDS)]
        files.append(('%d_%dx%dx%d_l%d_s%d' % (k, h, w, ch, level, strategy),
                      encode(pattern(h, w, ch, 100 + k), filters=filter_types(h, k), level=level, strategy=strategy)))
    for row in (0, 63, 64, 128):                              # every type on row 0 and on the band edges
        seen = {filter_types(h, k)[row] for k, (h, w) in enumerate([s for s in SIZES for _ in CHANNELS] + [(130, 9)] * 2) if h > row}
        assert seen == {0, 1, 2, 3, 4}, (row, seen)
    return files


def write_vectors(path, clips):
    """the vectors file of tools/png_inflate_check.cpp, from the Python definition clips._png_inflate: the special and the
    damaged streams, the zlib-written streams of the filter files, a dynamic one cut at 20 lengths, and it and a fixed one with a single bit
    flipped, 30 times (whatever status the definition gives those) -> [(name, status)]"""
    cases = [(name, raw, TOTAL) for name, raw, _ in special_streams()] + [(name, raw, TOTAL) for name, raw, _ in damaged_streams()]
    headers = [(name, clips.png_parse(f)) for name, f in filter_files(clips.png_encode_host)]
    cases += [('file_' + name, hd.data, hd.raw_bytes) for name, hd in headers]
    dynamic = next(h for n, h in headers if n.startswith('17_130x9x4_l9'))
    fixed = next(h for n, h in headers if n.startswith('16_130x9x3_l6_s4'))
    for i in range(20):
        cases.append(('cut_%d' % i, dynamic.data[:len(dynamic.data) * i // 20 + i % 3], dynamic.raw_bytes))
    for i in range(30):
        hd = dynamic if i % 2 else fixed
        bit = (i * 2654435761 + 12345) % (8 * min(len(hd.data), 80 if i < 16 else len(hd.data)))
        flipped = bytearray(hd.data)
        flipped[bit // 8] ^= 1 << (bit % 8)
        cases.append(('flip_%d' % i, bytes(flipped), hd.raw_bytes))
    cases.append(('empty', b'', 7))
    done = []
    with open(path, 'w') as fh:
        for name, raw, expected in cases:
            out, status = clips._png_inflate(raw, expected)
            fh.write('%s %d %d %s %s\n' % (name, status, expected, raw.hex() or '-', bytes(out).hex() if status == 0 else '-'))
            done.append((name, status))
    return done
