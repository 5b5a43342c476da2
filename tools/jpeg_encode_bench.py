#!/usr/bin/env python3
"""JPEG files out (DESIGN.md "JPEG files out") on one GPU in one process: ops.jpeg_encode_u8 on one training step's frames.

    python tools/jpeg_encode_bench.py [--frames 256] [--size 224] [--out profiles/NAME.txt]

--frames frames of --size x --size: 8 distinct smooth_image frames (tests/golden/make_jpeg_golden.py's recipe) repeated, on
the device; quality 75 and 90, 4:2:0, restart interval 'row' and 0.  Per configuration, after checking two distinct files
against clips.jpeg_encode_host:

encode   ops.jpeg_encode_u8 into the caller's buffer, events around the call (four launches); alternating with
         ops.jpeg_roundtrip_u8 on the same frames as the yardstick; medians and min-max over the repeats after the warm-up
download data[:offsets[n]] against the raw frames (3 bytes per pixel), both into pinned memory, host clock around copy +
         synchronise
decode   ops.jpeg_decode_u8 on the encoder's own 'row' files (parsed and packed on the host beforehand), checked against
         ops.jpeg_roundtrip_u8

and last one batch of 1080 x 1920 frames, as VideoScorer.render_explanation(jpeg_quality=75) encodes them: 4:2:0, 'row'.

--optimize  instead of the above (DESIGN.md "JPEG files out, optimised tables"): per configuration, after checking two
         distinct files of ops.jpeg_encode_u8(optimize=True) against clips.jpeg_encode_host(optimize=True), the optimised
         call and the standard call in alternation (encode time, file bytes, scan bytes), then ops.jpeg_decode_u8 on the
         optimised files and on the standard files in alternation: the default call on 'row' files, split=128 on
         restart-less ones; both decodes must give the same frames.  With --against OTHER.so (another build of the library,
         the parent commit's) the standard entry of both libraries is also called in alternation on the same argument block:
         whether this commit's median lies inside the other's own min-max spread.

--layouts  instead of the above (DESIGN.md "JPEG files out, 4:2:2 and greyscale"): per configuration (quality, restart
         interval, standard or optimised tables) ops.jpeg_encode_u8(layout='422') and (layout='grey'), each in alternation
         with the 4:2:0 call of the same configuration (encode time, file bytes), after checking one file of each new
         layout against clips.jpeg_encode_host(layout=) once; then ops.jpeg_decode_u8 on each kind of file in alternation
         with the 4:2:0 files (the default call on 'row' files, split=128 on restart-less ones).  With --against OTHER.so
         istvt_jpeg_encode_u8 and istvt_jpeg_encode_opt_u8 of both libraries are called in alternation on one 4:2:0 argument
         block: whether this commit's median lies inside the other's own min-max spread.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import istvt_pkg  # noqa: E402

istvt_pkg.load()
from istvt_amd import clips, ops  # noqa: E402

DISTINCT = 8
QUALITIES = (75, 90)


def smooth_image(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [128 + 80 * np.sin(x / 5.0 + c) * np.cos(y / 7.0 + 2 * c) for c in range(3)]
    return np.clip(np.round(np.stack(planes, -1) + g.normal(0.0, 12.0, (h, w, 3))), 0, 255).astype(np.uint8)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def fmt(s):
    return '%.3f ms (%.3f-%.3f)' % (s['median_ms'], s['min_ms'], s['max_ms'])


def say(lines, text):
    print(text, flush=True)
    lines.append(text)


def alternate(a, first, second):
    ta, tb = [], []
    for r in range(a.warmup + a.reps):
        x, y = event_ms(first), event_ms(second)
        if r >= a.warmup:
            ta.append(x)
            tb.append(y)
    return stats(ta), stats(tb)


def optimize_main(a):
    from istvt_amd import _lib, frames as F
    n, S = a.frames, a.size
    lines, res = [], {}
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    raw_dev = src.repeat((-(-n // DISTINCT), 1, 1, 1))[:n].contiguous().cuda()
    dev = raw_dev.device
    data = [torch.empty((raw_dev.numel(),), dtype=torch.uint8, device=dev) for _ in range(2)]
    out = [torch.empty_like(raw_dev) for _ in range(2)]
    other = None
    if a.against:
        other = ctypes.CDLL(os.path.abspath(a.against))
        other.istvt_jpeg_encode_u8.argtypes, other.istvt_jpeg_encode_u8.restype = _lib.SIGNATURES['istvt_jpeg_encode_u8'], ctypes.c_int
    for q in QUALITIES:
        qdev = torch.full((n,), q, dtype=torch.int32, device=dev)
        for ri in ('row', 0):
            if a.only and a.only != 'q%d_%s' % (q, ri):
                continue

            def encode(optimize):
                return ops.jpeg_encode_u8(raw_dev, qdev, '420', ri, out=data[optimize], checked=True, optimize=bool(optimize))
            files = [encode(0).files(), encode(1).files()]
            for i in (0, DISTINCT - 1):
                if files[1][i] != clips.jpeg_encode_host(src[i], q, '420', ri, optimize=True) or files[1][n - DISTINCT + i] != files[1][i]:
                    raise SystemExit('q=%d ri=%s: optimised file %d is not the definition' % (q, ri, i))
            so, ss = alternate(a, lambda: encode(1), lambda: encode(0))
            batches = [clips.jpeg_batch(f) for f in files]
            split = None if ri == 'row' else clips.JPEG_SPLIT_DEFAULT

            def decode(k):
                return ops.jpeg_decode_u8(batches[k], out=out[k], checked=True, split=split)
            for k in range(2):
                clips.check_jpeg_status(decode(k)[2])
            if not torch.equal(out[0], out[1]):
                raise SystemExit('q=%d ri=%s: the optimised files do not decode to the frames of the standard files' % (q, ri))
            do, ds = alternate(a, lambda: decode(1), lambda: decode(0))
            key = 'q%d_%s' % (q, ri)
            nb = [sum(len(f) for f in fs) for fs in files]
            res[key] = {'frames': n, 'size': S, 'file_bytes': nb[0], 'file_bytes_opt': nb[1], 'scan_bytes': batches[0].nbytes,
                        'scan_bytes_opt': batches[1].nbytes, 'encode': ss, 'encode_opt': so, 'decode': ds, 'decode_opt': do,
                        'decode_call': 'default' if split is None else 'split=%d' % split}
            say(lines, 'q=%d, restart interval %s, %d frames of %d x %d | encode optimised %s against standard %s beside it = %.2f x | '
                'files %.3f MB against %.3f MB = %.3f, scans %.3f MB against %.3f MB = %.3f | jpeg_decode_u8 (%s) on the optimised '
                'files %s against %s on the standard ones = %.3f'
                % (q, ri, n, S, S, fmt(so), fmt(ss), so['median_ms'] / ss['median_ms'], nb[1] * 1e-6, nb[0] * 1e-6, nb[1] / nb[0],
                   batches[1].nbytes * 1e-6, batches[0].nbytes * 1e-6, batches[1].nbytes / batches[0].nbytes,
                   res[key]['decode_call'], fmt(do), fmt(ds), do['median_ms'] / ds['median_ms']))
            if other is not None:
                r = clips.jpeg_restart_interval(ri, S, '420')
                mcus = (-(-S // 16)) ** 2
                blocks, segments = n * mcus * 6, n * (-(-mcus // min(r, mcus)) if r else 1)
                header, hlen = F._jpeg_header_on(dev, S, S, '420', r)
                scratch = torch.empty((F.jpeg_encode_scratch_bytes(blocks, segments, n),), dtype=torch.uint8, device=dev)
                offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
                status = torch.empty((n,), dtype=torch.int32, device=dev)
                args = _lib.JpegEncodeArgs(
                    frames=raw_dev.data_ptr(), total=raw_dev.numel(), quality=qdev.data_ptr(), header=header.data_ptr(),
                    header_bytes=hlen, scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), data=data[0].data_ptr(),
                    capacity=data[0].numel(), offsets=offsets.data_ptr(), status=status.data_ptr(), stream=F._stream(), n=n, H=S, W=S,
                    subsampling=2, restart_interval=r, dqt0=clips.JPEG_HEADER_DQT[0], dqt1=clips.JPEG_HEADER_DQT[1])
                got = []
                for lib in (_lib.lib(), other):
                    data[0].zero_()
                    _lib.check(lib.istvt_jpeg_encode_u8(ctypes.byref(args)), 'istvt_jpeg_encode_u8')
                    got.append(data[0][:nb[0]].clone())
                if not torch.equal(got[0], got[1]) or bytes(got[0].cpu().numpy()) != b''.join(files[0]):
                    raise SystemExit('q=%d ri=%s: the two libraries write different standard files' % (q, ri))
                st, sp = alternate(a, lambda: _lib.lib().istvt_jpeg_encode_u8(ctypes.byref(args)),
                                   lambda: other.istvt_jpeg_encode_u8(ctypes.byref(args)))
                inside = sp['min_ms'] <= st['median_ms'] <= sp['max_ms']
                res[key].update({'entry_this': st, 'entry_other': sp, 'this_inside_others_spread': inside})
                say(lines, '    istvt_jpeg_encode_u8, this library %s against the other %s in alternation: this / other = %.4f; this '
                    "median %s the other's min-max" % (fmt(st), fmt(sp), st['median_ms'] / sp['median_ms'],
                                                       'inside' if inside else 'below' if st['median_ms'] < sp['min_ms'] else 'ABOVE'))
    line = json.dumps({'jpeg_encode_bench_optimize': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def layouts_main(a):
    from istvt_amd import _lib, frames as F
    n, S = a.frames, a.size
    lines, res = [], {}
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    raw_dev = src.repeat((-(-n // DISTINCT), 1, 1, 1))[:n].contiguous().cuda()
    dev = raw_dev.device
    names = ('420', '422', 'grey')
    data = {k: torch.empty((raw_dev.numel(),), dtype=torch.uint8, device=dev) for k in names}
    out = {k: torch.empty_like(raw_dev) for k in names}
    other = None
    if a.against:
        other = ctypes.CDLL(os.path.abspath(a.against))
        for entry in ('istvt_jpeg_encode_u8', 'istvt_jpeg_encode_opt_u8'):
            getattr(other, entry).argtypes, getattr(other, entry).restype = _lib.SIGNATURES[entry], ctypes.c_int
    checked = set()
    for q in QUALITIES:
        qdev = torch.full((n,), q, dtype=torch.int32, device=dev)
        for ri in ('row', 0):
            for optimize in (False, True):
                key = 'q%d_%s_%s' % (q, ri, 'opt' if optimize else 'std')
                if a.only and a.only != key:
                    continue

                def encode(layout):
                    return ops.jpeg_encode_u8(raw_dev, qdev, restart_interval=ri, out=data[layout], checked=True, optimize=optimize,
                                              layout=layout)
                files = {k: encode(k).files() for k in names}
                for k in names[1:]:
                    if (k, optimize) not in checked:              # the definition takes seconds per frame of this size: once
                        checked.add((k, optimize))
                        want = clips.jpeg_encode_host(src[DISTINCT - 1], q, restart_interval=ri, optimize=optimize, layout=k)
                        if files[k][DISTINCT - 1] != want or files[k][n - 1] != files[k][(n - 1) % DISTINCT]:
                            raise SystemExit('%s: the %s file is not the definition' % (key, k))
                batches = {k: clips.jpeg_batch(files[k], 'all') for k in names}
                split = None if ri == 'row' else clips.JPEG_SPLIT_DEFAULT

                def decode(k):
                    return ops.jpeg_decode_u8(batches[k], out=out[k], checked=True, split=split)
                for k in names:
                    clips.check_jpeg_status(decode(k)[2])
                nb = {k: sum(len(f) for f in files[k]) for k in names}
                res[key] = {'frames': n, 'size': S, 'decode_call': 'default' if split is None else 'split=%d' % split}
                for k in names[1:]:
                    se, sb = alternate(a, lambda: encode(k), lambda: encode('420'))
                    sd, sdb = alternate(a, lambda: decode(k), lambda: decode('420'))
                    res[key][k] = {'file_bytes': nb[k], 'file_bytes_420': nb['420'], 'encode': se, 'encode_420': sb, 'decode': sd,
                                   'decode_420': sdb}
                    say(lines, '%s, %d frames of %d x %d | %s: encode %s against 4:2:0 %s beside it = %.3f | files %.3f MB against %.3f MB '
                        '= %.3f | jpeg_decode_u8 (%s) %s against %s on the 4:2:0 files = %.3f'
                        % (key, n, S, S, k, fmt(se), fmt(sb), se['median_ms'] / sb['median_ms'], nb[k] * 1e-6, nb['420'] * 1e-6,
                           nb[k] / nb['420'], res[key]['decode_call'], fmt(sd), fmt(sdb), sd['median_ms'] / sdb['median_ms']))
                if other is not None:
                    r = clips.jpeg_restart_interval(ri, S, '420')
                    mcus = (-(-S // 16)) ** 2
                    blocks, segments = n * mcus * 6, n * (-(-mcus // min(r, mcus)) if r else 1)
                    header, hlen = F._jpeg_header_on(dev, S, S, '420', r)
                    scratch = torch.empty((F.jpeg_encode_scratch_bytes(blocks, segments, n, optimize),), dtype=torch.uint8, device=dev)
                    offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)
                    status = torch.empty((n,), dtype=torch.int32, device=dev)
                    args = _lib.JpegEncodeArgs(
                        frames=raw_dev.data_ptr(), total=raw_dev.numel(), quality=qdev.data_ptr(), header=header.data_ptr(),
                        header_bytes=hlen, scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), data=data['420'].data_ptr(),
                        capacity=data['420'].numel(), offsets=offsets.data_ptr(), status=status.data_ptr(), stream=F._stream(), n=n,
                        H=S, W=S, subsampling=2, restart_interval=r, dqt0=clips.JPEG_HEADER_DQT[0], dqt1=clips.JPEG_HEADER_DQT[1])
                    entry = 'istvt_jpeg_encode_opt_u8' if optimize else 'istvt_jpeg_encode_u8'
                    rest = clips.JPEG_HEADER_DHT if optimize else ()

                    def call(lib):
                        return getattr(lib, entry)(ctypes.byref(args), *rest)
                    got = []
                    for lib in (_lib.lib(), other):
                        data['420'].zero_()
                        _lib.check(call(lib), entry)
                        got.append(data['420'][:nb['420']].clone())
                    if not torch.equal(got[0], got[1]) or bytes(got[0].cpu().numpy()) != b''.join(files['420']):
                        raise SystemExit('%s: the two libraries write different 4:2:0 files' % key)
                    st, sp = alternate(a, lambda: call(_lib.lib()), lambda: call(other))
                    inside = sp['min_ms'] <= st['median_ms'] <= sp['max_ms']
                    res[key].update({'entry': entry, 'entry_this': st, 'entry_other': sp, 'this_inside_others_spread': inside})
                    say(lines, '    %s at 4:2:0, this library %s against the other %s in alternation: this / other = %.4f; this median '
                        "%s the other's min-max" % (entry, fmt(st), fmt(sp), st['median_ms'] / sp['median_ms'],
                                                    'inside' if inside else 'below' if st['median_ms'] < sp['min_ms'] else 'ABOVE'))
    line = json.dumps({'jpeg_encode_bench_layouts': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--optimize', action='store_true')
    ap.add_argument('--layouts', action='store_true')
    ap.add_argument('--against', default=None)
    ap.add_argument('--only', default=None, help='one configuration (for a kernel trace): with --optimize q75_row | q75_0 | q90_row | '
                    'q90_0, with --layouts the same with _std or _opt behind it')
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--big', type=int, default=4, help='frames of the 1080 x 1920 batch (0: skip it)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_encode_bench.py measures on a GPU; none is visible')
    if a.optimize:
        return optimize_main(a)
    if a.layouts:
        return layouts_main(a)
    n, S = a.frames, a.size
    lines, res = [], {}
    src = torch.stack([torch.from_numpy(smooth_image(S, S, 1000 + i)) for i in range(DISTINCT)])
    raw_dev = src.repeat((-(-n // DISTINCT), 1, 1, 1))[:n].contiguous().cuda()
    raw_host = torch.empty(raw_dev.shape, dtype=torch.uint8).pin_memory()
    rt_out = torch.empty_like(raw_dev)
    data = torch.empty((raw_dev.numel(),), dtype=torch.uint8, device=raw_dev.device)
    for q in QUALITIES:
        qdev = torch.full((n,), q, dtype=torch.int32, device=raw_dev.device)
        for ri in ('row', 0):
            enc = ops.jpeg_encode_u8(raw_dev, qdev, '420', ri, out=data, checked=True)
            files = enc.files()
            for i in (0, DISTINCT - 1):
                if files[i] != clips.jpeg_encode_host(src[i], q, '420', ri) or files[n - DISTINCT + i] != files[i]:
                    raise SystemExit('q=%d ri=%s: file %d is not the definition' % (q, ri, i))
            total = enc.nbytes()
            se, sr = alternate(a, lambda: ops.jpeg_encode_u8(raw_dev, qdev, '420', ri, out=data, checked=True),
                               lambda: ops.jpeg_roundtrip_u8(raw_dev, qdev, '420', out=rt_out, checked=True))
            file_host = torch.empty((total,), dtype=torch.uint8).pin_memory()
            tf, tw = [], []
            for r in range(a.warmup + a.reps):
                x = timed(lambda: file_host.copy_(data[:total], non_blocking=True))
                y = timed(lambda: raw_host.copy_(raw_dev, non_blocking=True))
                if r >= a.warmup:
                    tf.append(x)
                    tw.append(y)
            sf, sw = stats(tf), stats(tw)
            key = 'q%d_%s' % (q, ri)
            res[key] = {'frames': n, 'size': S, 'file_bytes': total, 'raw_bytes': raw_dev.numel(), 'encode': se, 'roundtrip': sr,
                        'download_files': sf, 'download_raw': sw}
            say(lines, "jpeg_encode_u8 q=%d, restart interval %s: %d frames of %d x %d | %s = %.2f us per frame | jpeg_roundtrip_u8 on "
                'the same frames %s | files %.2f MB against %.2f MB raw = 1 / %.1f: to pinned memory %s against %s'
                % (q, ri, n, S, S, fmt(se), se['median_ms'] * 1e3 / n, fmt(sr), total * 1e-6, raw_dev.numel() * 1e-6,
                   raw_dev.numel() / total, fmt(sf), fmt(sw)))
            if ri == 'row':                                       # the decoder on the encoder's own files
                batch = clips.jpeg_batch(files)
                dev = raw_dev.device
                buffers = (torch.empty((batch.scratch_bytes,), dtype=torch.uint8, device=dev),
                           torch.empty((n, 2), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
                out = torch.empty_like(raw_dev)
                got, _, status = ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=buffers)
                clips.check_jpeg_status(status)
                if not torch.equal(got, ops.jpeg_roundtrip_u8(raw_dev, qdev, '420', checked=True)):
                    raise SystemExit('q=%d: decoding the encoder\'s files is not the round trip' % q)
                sd, _ = alternate(a, lambda: ops.jpeg_decode_u8(batch, out=out, checked=True, buffers=buffers),
                                  lambda: ops.jpeg_roundtrip_u8(raw_dev, qdev, '420', out=rt_out, checked=True))
                res[key]['decode'] = sd
                res[key]['segments'] = int(batch.segments.shape[0])
                say(lines, "jpeg_decode_u8 on these files (%d segments): %s" % (res[key]['segments'], fmt(sd)))
    if a.big:
        frame = torch.from_numpy(smooth_image(1080, 1920, 1080))
        big = frame[None].repeat(a.big, 1, 1, 1).contiguous().cuda()
        qdev = torch.full((a.big,), 75, dtype=torch.int32, device=big.device)
        data = torch.empty((big.numel(),), dtype=torch.uint8, device=big.device)
        rt_out = torch.empty_like(big)
        enc = ops.jpeg_encode_u8(big, qdev, '420', 'row', out=data, checked=True)
        files = enc.files()
        got, _, status = ops.jpeg_decode_u8(files[:1])
        clips.check_jpeg_status(status)
        if not torch.equal(got, ops.jpeg_roundtrip_u8(big[:1], 75, '420')) or any(f != files[0] for f in files):
            raise SystemExit('1080 x 1920: decoding the file is not the round trip')
        se, sr = alternate(a, lambda: ops.jpeg_encode_u8(big, qdev, '420', 'row', out=data, checked=True),
                           lambda: ops.jpeg_roundtrip_u8(big, qdev, '420', out=rt_out, checked=True))
        res['big'] = {'frames': a.big, 'file_bytes': enc.nbytes(), 'raw_bytes': big.numel(), 'encode': se, 'roundtrip': sr}
        say(lines, "jpeg_encode_u8 q=75, restart interval row: %d frames of 1080 x 1920 | %s = %.3f ms per frame | jpeg_roundtrip_u8 %s "
            '| files %.2f MB against %.2f MB raw = 1 / %.1f'
            % (a.big, fmt(se), se['median_ms'] / a.big, fmt(sr), enc.nbytes() * 1e-6, big.numel() * 1e-6, big.numel() / enc.nbytes()))
    line = json.dumps({'jpeg_encode_bench': res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')


if __name__ == '__main__':
    main()
