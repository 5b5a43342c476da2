"""Files, banks and vectors for the tests of the PNG bank (test_png_bank_cpu.py, test_png_bank_gpu.py; no tests in here): the
fixture bank with the conditions it must meet, the files that are damaged or lie, the doctored table rows, the index shapes,
and the vectors of tools/png_bank_check.cpp written from the definition.  Only rows and streams that program has passed go to
a device: the GPU tests take their banks, doctored rows and files from here and from nowhere else."""
import numpy as np
import torch

import png_bands_cases as B
import png_streams as P

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
_CACHE = {}


def fixture_files(clips):
    """png_bands_cases.MIXED's files and one file without a baND chunk, with the conditions the tests lean on"""
    if 'files' not in _CACHE:
        files = [f for _, f in B.mixed_files(clips)] + [clips.png_encode_host(P.pattern(23, 31, 3, 7), level=6)]
        counts = [1 if hd.bands is None else len(hd.bands[1]) - 1 for hd in map(clips.png_parse, files)]
        assert clips.png_parse(files[-1]).bands is None
        assert max(counts) > 64                                    # the unfilter's ballot loop takes a second round
        assert 1 in counts[:-1]                                    # a file with an index of exactly one band
        assert min(counts) < max(counts)                           # idle waves exist
        assert {clips.png_parse(f).colour_type for f in files} == {0, 2, 6}
        _CACHE['files'] = files
    return _CACHE['files']


def fixture_bank(clips):
    if 'bank' not in _CACHE:
        _CACHE['bank'] = clips.png_bank(fixture_files(clips))
        assert _CACHE['bank'].band_max > 64
    return _CACHE['bank']


def reference(clips):
    """[(frame, status)] of png_decode_bands_host for every fixture file: computed once, shared, never changed"""
    if 'ref' not in _CACHE:
        _CACHE['ref'] = [clips.png_decode_bands_host(f, return_status=True) for f in fixture_files(clips)]
    return _CACHE['ref']


def index_shapes(n):
    """the five index shapes as lists: arange, reversed, all equal, one element, random with repeats"""
    rng = np.random.default_rng(5)
    return [('arange', list(range(n))), ('reversed', list(range(n))[::-1]), ('equal', [n // 2] * 4), ('one', [n - 1]),
            ('repeats', [int(v) for v in rng.integers(0, n, 2 * n)])]


def damaged_files(clips):
    """[file]: lying_files and two cut streams among sound ones"""
    if 'damaged' not in _CACHE:
        good = clips.png_encode_banded_host(P.pattern(36, 25, 3, 91), 8, index=True)
        plain = clips.png_encode_host(P.pattern(20, 17, 3, 12), level=6)
        hd = clips.png_parse(plain)
        cut1 = clips.png_wrap(20, 17, 2, b'\x78\x01' + hd.data[:len(hd.data) // 2] + bytes(4))
        cut2 = clips.png_wrap(20, 17, 2, b'\x78\x01' + hd.data[:3] + bytes(4))
        files = [good]
        for _, f, _ in B.lying_files(clips):
            files += [f, good]
        _CACHE['damaged'] = files + [cut1, plain, cut2]
    return _CACHE['damaged']


def damaged_bank(clips):
    if 'damaged_bank' not in _CACHE:
        _CACHE['damaged_bank'] = clips.png_bank(damaged_files(clips))
    return _CACHE['damaged_bank']


def small_files(clips):
    """three small files for the banks whose first stream lies beyond 2^31 and 2^32 bytes"""
    if 'small' not in _CACHE:
        _CACHE['small'] = [clips.png_encode_banded_host(P.pattern(9, 14, 3, 3), 4, index=True),
                           clips.png_encode_banded_host(P.pattern(12, 7, 1, 4), 16, index=True),
                           clips.png_encode_host(P.pattern(6, 5, 4, 5), level=6)]
    return _CACHE['small']


def with_rows(clips, bank, images=None, bands=None):
    """a second bank over the same bytes with other table rows (host tensors): what a device table that differs from what
    png_bank built looks like"""
    other = clips.PngBank(**{k: v for k, v in bank.__dict__.items() if k != '_on'})
    if images is not None:
        other.images = images
    if bands is not None:
        other.bands, other.nband = bands, int(bands.shape[0])
    return other


def doctored(clips, bank):
    """[(name, the doctored bank, the place whose rows were changed)]: every one gives status 9 at that place and leaves every
    other place as it was.  The places: a = a file with several bands, b = another."""
    images, bands = bank.images, bank.bands
    counts = images[:, 8].tolist()
    a = next(i for i, c in enumerate(counts) if 3 <= c <= 16)
    other = next(i for i, c in enumerate(counts) if i != a and c >= 2)
    grey = next(i for i, r in enumerate(images.tolist()) if r[2] == 0)
    out = []

    def image(name, i, col, value):
        t = images.clone()
        t[i, col] = value
        out.append((name, with_rows(clips, bank, images=t), i))

    def band(name, i, k, col, value):
        t = bands.clone()
        t[int(images[i, 7]) + k, col] = value
        out.append((name, with_rows(clips, bank, bands=t), i))

    image('count_above_band_max', a, 8, bank.band_max + 1)
    image('count_0', a, 8, 0)
    image('band_row_past_nseg', a, 7, bank.nband - 1)            # its second band would be row nband
    image('first_band_row_past_nseg', a, 7, bank.nband)
    image('band_row_of_another_file', a, 7, int(images[other, 7]))
    band('end_beyond_the_stream', a, 1, 2, int(images[a, 6]) + 1)
    band('out_beyond_the_rows', a, 2, 4, int(images[a, 0]) * (1 + int(images[a, 1]) * int(images[a, 3])))
    image('H_above_the_canvas', a, 0, bank.Hmax + 1)
    t = images.clone()
    t[grey, :4] = torch.tensor([bank.Hmax, bank.Wmax, 6, 4], dtype=torch.int32)
    assert bank.Hmax * (1 + bank.Wmax * 4) > bank.raw_stride
    out.append(('rows_above_raw_stride', with_rows(clips, bank, images=t), grey))
    image('unaligned_base', a, 4, int(images[a, 4]) + 8)
    image('base_beyond_nbytes', a, 5, int(images[a, 5]) + 1)
    return out


def call_of(bank, canvas=None):
    """the scalars of a call as tools/png_bank_check.cpp reads them: nbytes n nseg band_max raw_stride Hc Wc"""
    Hc, Wc = canvas or (bank.Hmax, bank.Wmax)
    return '%d %d %d %d %d %d %d' % (bank.first_byte + bank.nbytes, bank.n, bank.nband, bank.band_max, bank.raw_stride, Hc, Wc)


def base_of(row):
    return ((row[5] & 0xffffffff) << 32) | (row[4] & 0xffffffff)


def lookup_line(clips, name, bank, index, expect=None):
    """an L line: the definition's statuses of `index` on the bank -> (the line, the statuses).  expect: statuses known
    without decoding (a bank whose files are sound: 0 inside the bank), else png_bank_decode_host says them"""
    status = expect if expect is not None else clips.png_bank_decode_host(bank, torch.tensor(index, dtype=torch.int32))[2].tolist()
    rows = bank.images.tolist()
    bases = [base_of(rows[i]) if 0 <= i < bank.n else -1 for i in index]    # compared where a wave of the place runs
    csv = lambda v: ','.join(str(int(x)) for x in v)
    return 'L %s %s %d %s %s %s %s %s' % (name, call_of(bank), len(index), csv(bank.images.flatten().tolist()),
                                         csv(bank.bands.flatten().tolist()), csv(index), csv(status), csv(bases)), status


def band_lines(clips, name, bank):
    """the B lines of every band of every file of a bank, from the bank's own rows and bytes -> [(line, status)]"""
    out = []
    csv = lambda v: ','.join(str(int(x)) for x in v)
    for i, im in enumerate(bank.images.tolist()):
        at = base_of(im) - bank.first_byte
        stream = bytes(bank.data[at:at + im[6]].numpy())
        for k in range(im[8]):
            row = bank.bands[im[7] + k].tolist()
            got, status = clips._png_inflate(stream[row[1]:row[2]], row[4], middle=k < im[8] - 1)
            out.append(('B %s_f%d_b%d %d %d %s %s %s %s %s' % (name, i, k, status, k, call_of(bank), csv(im), csv(row),
                                                              stream[row[1]:row[2]].hex() or '-',
                                                              bytes(got).hex() if status == 0 and got else '-'), status))
    return out


def outside_index(n):
    """indices inside the bank, repeated, and -1, n, INT_MIN and INT_MAX"""
    return [0, n - 1, -1, 1, n, 1, INT_MIN, 0, INT_MAX]


def write_vectors(path, clips):
    """Everything the GPU tests hand to a device, as the vectors of tools/png_bank_check.cpp -> (lookups, bands, the set of
    band statuses, the names of the doctored banks written)"""
    bank, dam, lines, names = fixture_bank(clips), damaged_bank(clips), [], []
    n = bank.n
    sound = lambda index, b: [0 if 0 <= i < b.n else 8 for i in index]
    for name, index in index_shapes(n):
        lines.append(lookup_line(clips, 'fixture_' + name, bank, index, sound(index, bank))[0])
    lines.append(lookup_line(clips, 'fixture_outside', bank, outside_index(n), sound(outside_index(n), bank))[0])
    for first in (2 ** 31 + 4096, 2 ** 32 + 16):                   # arithmetic only: no block of that size
        big = clips.png_bank(small_files(clips), first_byte=first)
        index = [2, 0, 1, 1, 0, 2, 2, -1, 3]
        lines.append(lookup_line(clips, 'first_byte_%d' % first, big, index, sound(index, big))[0])
    for name, bad, place in doctored(clips, bank):
        index = [place, (place + 1) % n, place, -1, (place + 2) % n, n]
        want = [9 if i == place else 0 if 0 <= i < n else 8 for i in index]
        line, status = lookup_line(clips, 'doctored_' + name, bad, index)
        assert status == want, (name, status)                      # the definition, decoded from the doctored rows
        lines.append(line)
        names.append(name)
    nlook = len(lines)
    statuses = set()
    for name, b in (('fixture', bank), ('damaged', dam), ('small', clips.png_bank(small_files(clips)))):
        for line, status in band_lines(clips, name, b):
            lines.append(line)
            statuses.add(status)
    with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    return nlook, len(lines) - nlook, statuses, names
