"""What the byte-frame wrappers (frames.py; ops re-exports them) tell their callers and their kernels, at the smallest shapes:
RGB (2, 8, 8, 3), clips (1, 2, 8, 8, 3), NV12 (2, 12, 8) and (1, 2, 12, 8), S = 4, maps (2, 2, 2).

Refusals: every case is one entry, valid arguments and exactly one thing made wrong; the (exception type, message) must be the
pair recorded in tests/golden/frames_refusals.json, which is this project's own output on the device at the commit before
the wrappers moved into one module (device strings normalised).  The cases whose error comes before the device check ran
on host tensors there too and gave the same pair ("cpu": true): test_refusals_before_the_device_check_cpu repeats them
without a device.

Passing calls: every entry with a host table, with checked=True, on clips, and (the NV12 readers) on a (B = 2, T = 2) batch
whose clip stride is not T frame strides, against the clips.*_host definition bit for bit, recording under ops.kernel_profile
exactly the names and byte counts in the same file.  The maps of the two warps are whole-pixel translations, the one case in
which the float64 definition and the kernel sum a single tap: the comparison is exact there."""
import functools
import json
import os
import re

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'frames_refusals.json')
S, T = 4, 2
NV12 = ('nv12_to_rgb_u8', 'crop_resize_nv12', 'warp_similarity_nv12', 'relevance_paste_nv12')
TABLES = {'crop_resize_u8': ('boxes',), 'crop_resize_nv12': ('boxes',), 'nv12_to_rgb_u8': (),
          'warp_similarity_u8': ('M',), 'warp_similarity_nv12': ('M',),
          'relevance_paste_u8': ('A', 'rect'), 'relevance_paste_nv12': ('A', 'rect'),
          'jpeg_roundtrip_u8': ('quality',), 'perturb_u8': ('table',)}
PASTES = ('relevance_paste_u8', 'relevance_paste_nv12')
TAKE_CLIPS = tuple(e for e in TABLES if e not in PASTES)
PER_FRAME = ('boxes', 'M', 'maps', 'A', 'rect', 'quality', 'table')


@pytest.fixture(scope='module')
def pkg():
    import istvt_pkg
    return istvt_pkg.load()


def _bytes(shape, seed=7):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _lut():
    return _bytes((256, 3), 11)


def valid(entry, dev, layout='frames'):
    """the keyword arguments of a passing call of `entry`: the frames (and what must live beside them) on `dev`, the tables on
    the host.  layout: 'frames' (n = 2), 'clip' (B = 1, T = 2) or 'strided' (NV12, B = 2, T = 2, a gap between the clips)"""
    from istvt_amd import clips
    nv = entry in NV12
    pic = (12, 8) if nv else (8, 8, 3)
    if layout == 'strided':
        big = torch.zeros((2, 3) + pic, dtype=torch.uint8, device=dev)
        big[:, :T] = _bytes((2, T) + pic).to(dev)
        frames = big[:, :T]
        assert frames.stride(0) != T * frames.stride(1)
    else:
        frames = _bytes((2,) + pic).to(dev)
        frames = frames[None] if layout == 'clip' else frames
    rows = 1 if layout == 'clip' else 2
    boxes = torch.tensor([[0, 0, 8, 8], [1, 2, 4, 4]], dtype=torch.int32)[:rows]
    a = {'frames': frames}
    if entry.startswith('crop_resize'):
        a.update(boxes=boxes, S=S)
    elif entry.startswith('warp_similarity'):
        a.update(M=torch.tensor([[[1, 0, 2], [0, 1, 3]], [[1, 0, 0], [0, 1, 4]]], dtype=torch.float32)[:rows], S=S)
    elif entry in PASTES:
        A, rect = clips.paste_geometry(2, 8, 8, S, boxes=boxes, even=nv)
        maps = torch.randn((2, 2, 2), generator=torch.Generator().manual_seed(5), dtype=torch.float32).to(dev)
        a.update(maps=maps, A=A, rect=rect, alpha=0.6, S=S)
        a['lut_ycc' if nv else 'lut'] = (clips.lut_to_ycc(_lut()) if nv else _lut()).to(dev)
    elif entry == 'jpeg_roundtrip_u8':
        a.update(quality=torch.tensor([40, 0], dtype=torch.int32)[:rows])
    elif entry == 'perturb_u8':
        a.update(table=torch.tensor([[1, 300, 0, 0], [6, 2, 1, 0]], dtype=torch.int32)[:rows])
    return a


def make_checked(entry, a, dev, layout='frames'):
    """the same call with checked=True: per-frame device tables (perturb_u8 keeps its per-clip rows: the kernel spreads them)"""
    for t in TABLES[entry]:
        tab = a[t]
        if layout != 'frames' and entry != 'perturb_u8':
            tab = tab.repeat_interleave(T, dim=0)
        a[t] = tab.to(dev)
    a['checked'] = True


def _out_shape(entry, a):
    f = a['frames']
    if entry in PASTES or entry in ('jpeg_roundtrip_u8', 'perturb_u8'):
        return tuple(f.shape)
    lead = tuple(f.shape[:-2] if entry in NV12 else f.shape[:-3])
    return lead + ((8, 8, 3) if entry == 'nv12_to_rgb_u8' else (S, S, 3))


# ---- the faults: fn(entry, a, dev) makes one thing wrong ---------------------------------------------------------------------
def _set(key, value):
    return lambda entry, a, dev: a.__setitem__(key, value(entry, a, dev) if callable(value) else value)


def _too_large(entry, a, dev):
    a['frames'] = torch.zeros((1, 24579, 2) if entry in NV12 else (1, 16385, 1, 3), dtype=torch.uint8, device=dev)
    for k in PER_FRAME:
        if k in a:
            a[k] = a[k][:1]


def _pitch(entry, a, dev):
    p = (1 << 20) + 1
    a['frames'] = torch.zeros((11 * p + 8,), dtype=torch.uint8, device=dev).as_strided((2, 12, 8), (0, p, 1))


def _overlap(entry, a, dev):
    if entry == 'nv12_to_rgb_u8':
        buf = torch.zeros((2000,), dtype=torch.uint8, device=dev)
        a['frames'], a['out'] = buf[:192].view(2, 12, 8), buf[100:100 + 384].view(2, 8, 8, 3)
    else:
        a['out'] = a['frames']


def _edit(key, index, value):
    def fn(entry, a, dev):
        a[key] = a[key].clone()
        a[key][index] = value
    return fn


def _inplace_overlapping(entry, a, dev):
    a['frames'] = torch.zeros((200,), dtype=torch.uint8, device=dev).as_strided((2, 12, 8), (50, 8, 1))
    a['inplace'] = True


def _inplace_with_out(entry, a, dev):
    a['inplace'], a['out'] = True, torch.empty_like(a['frames'])


def _inplace_noncontig(entry, a, dev):
    a['frames'], a['inplace'] = _bytes((2, 8, 16, 3)).to(dev)[:, :, ::2], True


_OTHER = {torch.int32: torch.int64, torch.float32: torch.float64, torch.float64: torch.float32}


def _cases():
    """[(id, entry, layout, checked, fault)]"""
    out = []

    def add(entry, name, fn, layout='frames', checked=False):
        out.append(('%s-%s' % (entry, name), entry, layout, checked, fn))

    for e, tabs in TABLES.items():
        nv = e in NV12
        add(e, 'frames_dtype', _set('frames', lambda entry, a, dev: a['frames'].to(torch.int16)))
        add(e, 'frames_rank', _set('frames', lambda entry, a, dev: a['frames'][0]))
        add(e, 'frames_empty', _set('frames', lambda entry, a, dev: a['frames'][:0]))
        add(e, 'frames_too_large', _too_large)
        if nv:
            add(e, 'odd_rows', _set('frames', lambda entry, a, dev: _bytes((2, 13, 8)).to(dev)))
            add(e, 'odd_width', _set('frames', lambda entry, a, dev: _bytes((2, 12, 7)).to(dev)))
            add(e, 'pitch', _pitch)
            if e not in PASTES:
                add(e, 'matrix', _set('matrix', 'bt2020'))
        else:
            add(e, 'last_not_3', _set('frames', lambda entry, a, dev: _bytes((2, 8, 8, 4)).to(dev)))
        if e in ('jpeg_roundtrip_u8', 'perturb_u8'):
            add(e, 'frames_noncontig', _set('frames', lambda entry, a, dev: _bytes((2, 8, 16, 3)).to(dev)[:, :, ::2]))
        if e != 'nv12_to_rgb_u8' and e not in ('jpeg_roundtrip_u8', 'perturb_u8'):
            add(e, 'S_0', _set('S', 0))
            add(e, 'S_481', _set('S', 481))
        add(e, 'out_dtype', _set('out', lambda entry, a, dev: torch.empty(_out_shape(entry, a), dtype=torch.float32, device=dev)))
        add(e, 'out_shape', _set('out', lambda entry, a, dev: torch.empty((3,) + _out_shape(entry, a)[1:], dtype=torch.uint8,
                                                                         device=dev)))
        add(e, 'out_device', _set('out', lambda entry, a, dev: torch.empty(_out_shape(entry, a), dtype=torch.uint8)))
        if e in ('nv12_to_rgb_u8', 'jpeg_roundtrip_u8', 'perturb_u8'):
            add(e, 'out_overlap', _overlap)
        for t in tabs:
            add(e, 'checked_%s_dtype' % t, _set(t, lambda entry, a, dev, t=t: a[t].to(_OTHER[a[t].dtype])), checked=True)
            add(e, 'checked_%s_shape' % t, _set(t, lambda entry, a, dev, t=t: a[t][:1]), checked=True)
            add(e, 'checked_%s_host' % t, _set(t, lambda entry, a, dev, t=t: a[t].cpu()), checked=True)
            add(e, 'unchecked_%s_dtype' % t, _set(t, lambda entry, a, dev, t=t: a[t].to(_OTHER[a[t].dtype])))
            add(e, 'unchecked_%s_shape' % t, _set(t, lambda entry, a, dev, t=t: a[t][:1]))
            if e in TAKE_CLIPS:
                add(e, 'clip_%s_n_rows' % t, _set(t, lambda entry, a, dev, t=t: torch.cat([a[t], a[t]])), layout='clip')
                if e == 'perturb_u8':      # its checked table is per clip
                    add(e, 'clip_checked_n_rows', _set(t, lambda entry, a, dev, t=t: torch.cat([a[t], a[t]])), 'clip', True)
                else:
                    add(e, 'clip_checked_%s_B_rows' % t, _set(t, lambda entry, a, dev, t=t: a[t][:1]), 'clip', True)
            if e in ('jpeg_roundtrip_u8', 'perturb_u8'):
                add(e, 'unchecked_device_%s' % t, _set(t, lambda entry, a, dev, t=t: a[t].to(dev)))
    for e in ('crop_resize_u8', 'crop_resize_nv12'):
        add(e, 'box_outside', _edit('boxes', (1, 0), 6))
    for e in ('warp_similarity_u8', 'warp_similarity_nv12'):
        add(e, 'M_not_a_similarity', _edit('M', (0, 0, 0), 2.0))
        add(e, 'M_nonfinite', _edit('M', (1, 0, 2), float('nan')))
        add(e, 'M_centre_outside', _edit('M', (1, 1, 2), 40.0))
    for e in PASTES:
        add(e, 'inplace_with_out', _inplace_with_out)
        add(e, 'alpha_nan', _set('alpha', float('nan')))
        add(e, 'alpha_inf', _set('alpha', float('inf')))
        add(e, 'alpha_shape', _set('alpha', lambda entry, a, dev: torch.ones((3,), dtype=torch.float32)))
        add(e, 'alpha_dtype', _set('alpha', lambda entry, a, dev: torch.ones((2,), dtype=torch.float64)))
        add(e, 'A_nonfinite', _edit('A', (0, 0, 0), float('inf')))
        add(e, 'rect_negative_extent', _edit('rect', (1, 2), -1))
        add(e, 'maps_dtype', _set('maps', lambda entry, a, dev: a['maps'].double()))
        add(e, 'maps_rows', _set('maps', lambda entry, a, dev: a['maps'][:1]))
        add(e, 'maps_not_square', _set('maps', lambda entry, a, dev: a['maps'].reshape(2, 4)[:, :3]))
        add(e, 'maps_grid_20', _set('maps', lambda entry, a, dev: torch.zeros((2, 20, 20), dtype=torch.float32, device=dev)))
        add(e, 'maps_on_the_host', _set('maps', lambda entry, a, dev: a['maps'].cpu()))
        lut = 'lut_ycc' if e in NV12 else 'lut'
        add(e, 'lut_shape', _set(lut, lambda entry, a, dev, lut=lut: a[lut][:255]))
        add(e, 'lut_dtype', _set(lut, lambda entry, a, dev, lut=lut: a[lut].to(torch.int32)))
    add('relevance_paste_u8', 'inplace_noncontig', _inplace_noncontig)
    add('relevance_paste_nv12', 'frames_rank_4', _set('frames', lambda entry, a, dev: a['frames'][None]))
    add('relevance_paste_nv12', 'inplace_frames_rank_4', lambda entry, a, dev: a.update(frames=a['frames'][None], inplace=True))
    add('relevance_paste_nv12', 'inplace_overlapping_frames', _inplace_overlapping)
    add('jpeg_roundtrip_u8', 'subsampling', _set('subsampling', '422'))
    add('jpeg_roundtrip_u8', 'quality_101', _set('quality', 101))
    add('perturb_u8', 'seed_negative', _set('seed', -1))
    add('perturb_u8', 'seed_2_64', _set('seed', 2 ** 64))
    add('perturb_u8', 'kind_9', _edit('table', (0, 0), 9))
    add('perturb_u8', 'checked_taps_shape', _set('taps', lambda entry, a, dev: torch.zeros((1, 20), dtype=torch.int32, device=dev)),
        checked=True)
    add('perturb_u8', 'unchecked_device_taps', _set('taps', lambda entry, a, dev: torch.zeros((1, 21), dtype=torch.int32,
                                                                                             device=dev)))
    return out


CASES = _cases()
assert len({c[0] for c in CASES}) == len(CASES)


def outcome(case, dev):
    """[exception type, message with the device's name normalised] of one case with its frames on `dev`"""
    from istvt_amd import ops
    _, entry, layout, checked, fault = case
    a = valid(entry, dev, layout)
    if checked:
        make_checked(entry, a, dev, layout)
    fault(entry, a, dev)
    try:
        getattr(ops, entry)(**a)
    except Exception as e:      # noqa: BLE001  (the type is what is compared)
        return [type(e).__name__, re.sub(r'cuda:\d+|\bcuda\b|\bcpu\b', '<dev>', str(e))]
    return ['no error', '']


# ---- the passing calls -------------------------------------------------------------------------------------------------------
def _passing():
    """[(id, entry, layout, checked)]"""
    out = []
    for e, tabs in TABLES.items():
        layouts = ('frames',) + (('clip',) if e in TAKE_CLIPS else ()) + (('strided',) if e in NV12 and e in TAKE_CLIPS else ())
        for layout in layouts:
            for checked in ((False, True) if tabs else (False,)):
                out.append(('%s-%s-%s' % (e, layout, 'checked' if checked else 'host'), e, layout, checked))
    return out


PASSING = _passing()


@functools.lru_cache(maxsize=None)
def definition(entry, layout):
    """the clips.*_host definition's bytes for valid(entry, ., layout), computed once"""
    from istvt_amd import clips
    a = valid(entry, 'cpu', layout)
    f = a['frames'].contiguous()
    if entry == 'crop_resize_u8':
        return clips.crop_resize_host(f, a['boxes'], S)
    if entry == 'crop_resize_nv12':
        return clips.crop_resize_nv12_host(f, a['boxes'], S)
    if entry == 'nv12_to_rgb_u8':
        return clips.nv12_to_rgb_host(f)
    if entry == 'warp_similarity_u8':
        return clips.warp_similarity_host(f, a['M'], S)
    if entry == 'warp_similarity_nv12':
        return clips.warp_similarity_host(clips.nv12_to_rgb_host(f), a['M'], S)
    if entry in PASTES:
        return clips.paste_maps_host(f, a['maps'], a['A'], a['rect'], _lut(), a['alpha'], S,
                                     pixel_format='nv12' if entry in NV12 else 'rgb24')
    if entry == 'jpeg_roundtrip_u8':
        return clips.jpeg_roundtrip_host(f, a['quality'])
    return clips.perturb_host(f, a['table'], None, 0)


def passing_call(case, dev='cuda'):
    """-> (the result on the host, [[name, bytes]] as ops.kernel_profile recorded them)"""
    from istvt_amd import ops
    _, entry, layout, checked = case
    a = valid(entry, dev, layout)
    if checked:
        make_checked(entry, a, dev, layout)
    before = a['frames'].clone()
    ops.kernel_profile = []
    try:
        got = getattr(ops, entry)(**a)
        rec = [[r[0], int(r[3])] for r in ops.kernel_profile]
    finally:
        ops.kernel_profile = None
    assert torch.equal(a['frames'], before)             # out of place: the input stays
    return got.cpu(), rec


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_refusal_is_the_recorded_one(pkg, case):
    want = golden()['refusals'][case[0]]
    assert want['type'] != 'no error'
    got = outcome(case, 'cuda')
    assert got == [want['type'], want['message']]


def test_refusals_before_the_device_check_cpu(pkg):
    """the cases the record marks as answered before the device check, on host tensors: the NV12 entries' argument errors"""
    rec = golden()['refusals']
    assert sorted(rec) == sorted(c[0] for c in CASES)
    ran = 0
    for case in CASES:
        want = rec[case[0]]
        if want['cpu']:
            assert outcome(case, 'cpu') == [want['type'], want['message']], case[0]
            assert case[1] in NV12
            ran += 1
    assert ran >= 29                                    # what _nv12_source and relevance_paste_nv12 refuse on their own


@pytest.mark.gpu
@pytest.mark.parametrize('case', PASSING, ids=[c[0] for c in PASSING])
def test_passing_call_gives_the_definition_and_the_recorded_profile(pkg, case):
    got, rec = passing_call(case)
    want = definition(case[1], case[2])
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want)
    assert rec == golden()['profiles'][case[0]]
    if case[2] == 'strided':
        assert len(rec) == 2                            # one launch per clip
