"""The table behind test_decode_refusals_cpu.py and test_decode_refusals_gpu.py: what the file decoders of frames.py
(jpeg_decode_u8, png_decode_u8, jpeg_decode_indexed_u8, jpeg_decode_drawn_u8; ops re-exports them) answer to a call that is
wrong in one way, as (entry, what is wrong, exception type, the whole message) with the device's name normalised to <dev>, and
what a passing call records under ops.kernel_profile.  Every message and number is written out here as the front end gave it
before its checks moved into shared helpers; none is asked of the code under test.

The inputs: two JPEG files, 17 x 33 in 4:2:0 with a restart marker per MCU row and 8 x 8 in 4:4:4 without (538 scan bytes, 39
blocks, 3 segments); the bank of the two, alone and with split=16 (its longest interval has 302 bytes: 19 state rows per
segment), drawn at m = 3 places [1, 0, 1] or by a plan of B = 1, T = 2; two PNG files of 20 x 31 RGB in bands of 8 rows."""
import functools
import re
from types import SimpleNamespace

import torch

import png_streams as P

# entry -> (the function, the result's leading size, canvas, the scratch a call needs, profile name, profile bytes)
ENTRIES = {
    'jpeg': ('jpeg_decode_u8', 2, (17, 33), 7500, 'jpeg_decode_u8', 538 + 2 * 192 * 39 + 2 * 17 * 33 * 3),
    'jpeg_split': ('jpeg_decode_u8', 2, (17, 33), 8656, 'jpeg_decode_split_u8', 538 + 2 * 192 * 39 + 2 * 17 * 33 * 3),
    'png': ('png_decode_u8', 2, (20, 31), 3776, 'png_decode_u8', 2432 + 2 * 3760 + 2 * 20 * 31 * 3),
    'png_bands': ('png_decode_u8', 2, (20, 31), 3800, 'png_decode_bands_u8', 2432 + 2 * 3760 + 2 * 20 * 31 * 3),
    'indexed': ('jpeg_decode_indexed_u8', 3, (17, 33), 28056, 'jpeg_decode_indexed_u8', 2 * 192 * 3 * 48 + 3 * 17 * 33 * 3),
    'indexed_split': ('jpeg_decode_indexed_u8', 3, (17, 33), 31712, 'jpeg_decode_indexed_split_u8',
                      2 * 192 * 3 * 48 + 3 * 17 * 33 * 3),
    'drawn': ('jpeg_decode_drawn_u8', 2, (17, 33), 18704, 'jpeg_decode_drawn_u8', 2 * 192 * 2 * 48 + 2 * 17 * 33 * 3),
    'drawn_split': ('jpeg_decode_drawn_u8', 2, (17, 33), 21136, 'jpeg_decode_drawn_split_u8', 2 * 192 * 2 * 48 + 2 * 17 * 33 * 3),
}
REFUSED = ('jpeg', 'png', 'png_bands', 'indexed', 'indexed_split', 'drawn')      # the entries the device cases run over
SPLIT_CLAUSE = ' for the split layout (bank.split = 16: 19 state rows per segment)'
INDEX = [1, 0, 1]


@functools.lru_cache(maxsize=None)
def inputs():
    """the files and what is packed from them, made once and left unchanged"""
    import istvt_pkg
    istvt_pkg.load()
    from istvt_amd import clips
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 256, (17, 33, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (8, 8, 3), generator=g, dtype=torch.uint8)
    files = [clips.jpeg_encode_host(a, 60, '420', 'row'), clips.jpeg_encode_host(b, 85, '444', 0)]
    pngs = [clips.png_encode_banded_host(P.pattern(20, 31, 3, s), 8, index=True) for s in (1, 2)]
    bank = clips.jpeg_bank(files)
    return SimpleNamespace(clips=clips, files=files, batch=clips.jpeg_batch(files), bank=bank, split_bank=clips.jpeg_bank(files, split=16),
                           pngs=pngs, png_batch=clips.png_batch(pngs), png_bands_batch=clips.png_batch(pngs, bands='index'))


def plan(bank_or_sizes):
    """a fresh plan of B = 1, T = 2 over one video of two places (every draw is the index [0, 1])"""
    return inputs().clips.BatchPlan(bank_or_sizes, [(0, 2, 1)], T=2, B=1, K=4, jpeg=None, perturb=None)


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)


def valid(entry, dev):
    """-> (the function's name, its positional arguments, its keyword arguments) of a passing call with `out` and `buffers`
    given, on `dev`"""
    x = inputs()
    fn, n, (Hc, Wc), need, _, _ = ENTRIES[entry]
    kw = {'out': _empty((n, Hc, Wc, 3), torch.uint8, dev),
          'buffers': (_empty((need,), torch.uint8, dev), _empty((n, 2), torch.int32, dev), _empty((n,), torch.int32, dev))}
    if entry in ('jpeg', 'jpeg_split'):
        args = (x.batch,)
        kw.update(checked=True, split=16 if entry == 'jpeg_split' else None)
    elif entry in ('png', 'png_bands'):
        args = (x.png_bands_batch if entry == 'png_bands' else x.png_batch,)
        kw.update(checked=True)
    else:
        bank = x.split_bank if entry.endswith('_split') else x.bank
        args = (bank, INDEX) if entry.startswith('indexed') else (bank, plan(bank).on(dev))
    return fn, args, kw


def definition(entry):
    """the clips.*_host definition of valid(entry, .): frames on the canvas"""
    x = inputs()
    c = x.clips
    _, n, (Hc, Wc), _, _, _ = ENTRIES[entry]
    if entry.startswith('indexed'):
        return c.jpeg_bank_decode_host(x.bank, INDEX)[0]
    if entry.startswith('drawn'):
        return c.jpeg_bank_decode_host(x.bank, c.batch_draw_host(plan(x.bank), 0).index)[0]
    one = {'jpeg': c.jpeg_decode_host, 'jpeg_split': c.jpeg_decode_host, 'png': c.png_decode_host,
           'png_bands': c.png_decode_bands_host}[entry]
    want = torch.zeros((n, Hc, Wc, 3), dtype=torch.uint8)
    for i, f in enumerate(x.files if entry.startswith('jpeg') else x.pngs):
        img = one(f).to(torch.uint8)
        want[i, :img.shape[0], :img.shape[1]] = img
    return want


def outcome(fn, args, kw):
    """[exception type, message with the device's name normalised] of one call"""
    from istvt_amd import ops
    try:
        getattr(ops, fn)(*args, **kw)
    except Exception as e:      # noqa: BLE001  (the type is what is compared)
        return [type(e).__name__, re.sub(r'cuda:\d+|\bcuda\b|\bcpu\b', '<dev>', str(e))]
    return ['no error', '']


# ---- before the device check: (id, fn, args, kw, type, message) ------------------------------------------------------------------
class UploadedBlock:
    """stands where a plan's uploaded draw block does, for the one check behind 'is it uploaded' that needs no device"""
    is_cuda = True


def host_cases():
    x = inputs()
    out = []
    for fn, cls, pack in (('jpeg_decode_u8', 'JpegBatch', 'jpeg_batch'), ('png_decode_u8', 'PngBatch', 'png_batch')):
        files = x.files if fn == 'jpeg_decode_u8' else x.pngs
        out += [
            ('%s-bytes' % fn, fn, (files[0],), {}, 'TypeError',
             '%s expects a sequence of files (bytes) or a clips.%s, got bytes' % (fn, cls)),
            ('%s-empty' % fn, fn, ([],), {}, 'RuntimeError', '%s: empty input (no files)' % fn),
            ('%s-checked_list' % fn, fn, (files,), {'checked': True}, 'RuntimeError',
             '%s: checked=True takes a clips.%s (clips.%s packs and validates the files)' % (fn, cls, pack)),
            # wrong twice: the checked refusal comes before the look at the list
            ('%s-checked_empty' % fn, fn, ([],), {'checked': True}, 'RuntimeError',
             '%s: checked=True takes a clips.%s (clips.%s packs and validates the files)' % (fn, cls, pack)),
        ]
    for split, text in ((True, 'True'), (8, '8'), ('x', "'x'")):
        out.append(('jpeg_decode_u8-split_%s' % split, 'jpeg_decode_u8', (x.files,), {'split': split}, 'ValueError',
                    "jpeg_decode_u8: split is None, 'auto' or a chunk size in bytes (an int of at least 16), got %s" % text))
    out.append(('png_decode_u8-bands_on_a_batch_without', 'png_decode_u8', (x.png_batch,), {'checked': True, 'bands': 'index'},
                'ValueError', "png_decode_u8: bands='index' with a clips.PngBatch that was packed without bands "
                              "(clips.png_batch(files, bands='index') packs them)"))
    out += [
        ('jpeg_decode_indexed_u8-not_a_bank', 'jpeg_decode_indexed_u8', (x.files, INDEX), {}, 'TypeError',
         'jpeg_decode_indexed_u8 expects a clips.JpegBank (clips.jpeg_bank, clips.JpegBank.from_encoded), got list'),
        ('jpeg_decode_drawn_u8-not_a_bank', 'jpeg_decode_drawn_u8', (x.batch, plan(x.bank)), {}, 'TypeError',
         'jpeg_decode_drawn_u8 expects a clips.JpegBank, got JpegBatch'),
        ('jpeg_decode_indexed_u8-split', 'jpeg_decode_indexed_u8', (x.bank, INDEX), {'split': 16}, 'ValueError',
         'jpeg_decode_indexed_u8: split= is not available for a bank (the state rows of the split kernel are addressed over the '
         'whole byte range, which here is the whole set): the split is a property of the bank, clips.jpeg_bank(files, split=) or '
         'bank.with_split(split)'),
        ('jpeg_decode_drawn_u8-plan_not_uploaded', 'jpeg_decode_drawn_u8', (x.bank, plan(x.bank)), {}, 'RuntimeError',
         'jpeg_decode_drawn_u8: the plan is drawn from where its draw block lives: upload it first, plan.on(device)'),
    ]
    other = plan([(17, 33), (8, 8), (8, 8)])
    other.block = UploadedBlock()
    out.append(('jpeg_decode_drawn_u8-plan_of_another_bank', 'jpeg_decode_drawn_u8', (x.bank, other), {}, 'ValueError',
                'jpeg_decode_drawn_u8: the plan was built for a bank of 3 places, this one has 2'))
    return out


NO_DEVICE = [('jpeg_decode_u8', 'istvt_amd: jpeg_decode_u8 needs a ROCm device (no CPU fallback exists for the ISTVT hot path)'),
             ('png_decode_u8', 'istvt_amd: png_decode_u8 needs a ROCm device (no CPU fallback exists for the ISTVT hot path)')]


# ---- on the device: (id, entry, fault(kw, dev), type, message) -------------------------------------------------------------------
def _buffers(which, make):
    def fault(kw, dev):
        b = list(kw['buffers'])
        b[which] = make(b[which], dev)
        kw['buffers'] = tuple(b)
    return fault


def device_cases():
    out = []
    for entry in REFUSED:
        fn, n, (Hc, Wc), need, _, _ = ENTRIES[entry]
        bank = entry in ('indexed', 'indexed_split', 'drawn')
        canvas = '%s: the canvas must hold every image%s (%d x %d at least, 16384 x 16384 at most), got %%d x %%d' \
            % (fn, ' of the bank' if bank else '', Hc, Wc)
        bad_out = '%s: out must be contiguous uint8 (%d, %d, %d, 3) on <dev>' % (fn, n, Hc, Wc)
        bad_buffers = '%s: buffers = (uint8 scratch of %d bytes%s, 16-byte aligned; int32 sizes (%d, 2); int32 status (%d,)), ' \
                      'contiguous on <dev>' % (fn, need, SPLIT_CLAUSE if entry == 'indexed_split' else '', n, n)
        hint = 'png_decode_u8: a batch with bands needs a scratch of 3800 bytes: 3776 of filtered rows and a status word for each ' \
               'of its 6 bands, got %d'

        def add(name, fault, kind, message, entry=entry):
            out.append(('%s-%s' % (entry, name), entry, fault, kind, message))
        add('canvas_too_small', lambda kw, dev, c=(Hc - 1, Wc): kw.update(canvas=c), 'ValueError', canvas % (Hc - 1, Wc))
        add('canvas_16385', lambda kw, dev, c=(16385, Wc): kw.update(canvas=c), 'ValueError', canvas % (16385, Wc))
        add('out_shape', lambda kw, dev, s=(n + 1, Hc, Wc, 3): kw.update(out=_empty(s, torch.uint8, dev)), 'RuntimeError', bad_out)
        add('out_dtype', lambda kw, dev, s=(n, Hc, Wc, 3): kw.update(out=_empty(s, torch.int8, dev)), 'RuntimeError', bad_out)
        add('out_noncontiguous', lambda kw, dev, s=(n, Hc, Wc, 6): kw.update(out=_empty(s, torch.uint8, dev)[..., ::2]),
            'RuntimeError', bad_out)
        add('scratch_one_byte_short', _buffers(0, lambda t, dev: t[:-1]), 'RuntimeError',
            hint % 3799 if entry == 'png_bands' else bad_buffers)
        add('scratch_misaligned_by_8', _buffers(0, lambda t, dev: _empty((t.numel() + 8,), torch.uint8, dev)[8:]), 'RuntimeError',
            bad_buffers)
        add('scratch_int8', _buffers(0, lambda t, dev: t.view(torch.int8)), 'RuntimeError', bad_buffers)
        add('sizes_int64', _buffers(1, lambda t, dev: t.to(torch.int64)), 'RuntimeError', bad_buffers)
        add('sizes_n_3', _buffers(1, lambda t, dev: _empty((t.shape[0], 3), torch.int32, dev)), 'RuntimeError', bad_buffers)
        add('status_n_plus_1', _buffers(2, lambda t, dev: _empty((t.shape[0] + 1,), torch.int32, dev)), 'RuntimeError', bad_buffers)
        add('status_on_the_host', _buffers(2, lambda t, dev: t.cpu()), 'RuntimeError', bad_buffers)
        if entry == 'png_bands':
            add('scratch_of_a_batch_without_bands', _buffers(0, lambda t, dev: t[:3776]), 'RuntimeError', hint % 3776)
        if entry == 'jpeg':
            # wrong twice: the canvas is looked at before the buffers
            add('canvas_too_small_and_bad_buffers',
                lambda kw, dev: (kw.update(canvas=(16, 33)), _buffers(0, lambda t, d: t[:-1])(kw, dev)), 'ValueError',
                canvas % (16, 33))
    return out
