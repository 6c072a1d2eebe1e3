"""Times of the feathered blend (sucre_mosaic_feather, sucre_mosaic_accumulate_feathered) on the shape of tools/mosaic_time.py: 65
resident images of 1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the
renderer's water, the default frame and ground sample distance, three calls per phase (32 + 32 + 1 images).  In ONE run, for
every feather width of --widths: the feather pass alone (both its launches, into one buffer per call), the feathered accumulate
alone (reading maps made before the events), and ``Mosaic.accumulate`` as a caller runs it (the pass, the two counts per image, the
accumulate; one buffer reused).  The yardstick, in the same run: the unfeathered accumulate.  The accumulator is zeroed before
every repetition outside the events.  F = 1 is in the list as a floor: its row pass scans nothing, so its time is the column pass
plus a row pass that only stages and writes.

    python tools/mosaic_feather_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --blend-depth 0.5 --widths 1 16 64 1024]
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import _lib, engine, sucre, synth  # noqa: E402
from mosaic_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--grid', type=int, nargs=2, default=(13, 5))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--blend-depth', type=float, default=0.5, help='blend depth H of the accumulate phase, metres')
    ap.add_argument('--widths', type=int, nargs='+', default=(1, 16, 64, 1024), help='feather widths F, source pixels')
    args = ap.parse_args()
    dev = 'cuda:0'
    survey = synth.make_survey(args.width, args.height, args.grid[0], args.grid[1], seed=0, device=dev)
    views = engine.device_views_from_scene(survey, dev)
    water = list(synth.GT_B) + list(synth.GT_BETA) + list(synth.GT_GAMMA)
    Js = engine.invert_images(views, water)
    n = len(views)
    axes = sucre.mosaic_axes(views)
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views]) * args.gsd_factor
    n_px = sum(v.depth.numel() for v in views)
    print(f'{torch.cuda.get_device_name(0)}; {n} images of {args.width}x{args.height}, {n_px} pixels; gsd {float(gsd):.6g} m; '
          f'blend depth {args.blend_depth:g} m')
    chunks = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]
    lib = _lib.load()
    stream = engine._stream_ptr

    def over(m, **kw):
        for i, v, J in chunks:
            m.accumulate(v, J, i, **kw)

    plain = engine.Mosaic(axes, gsd, dev)
    for _, v, J in chunks:
        plain.add_bounds(v, J)
    bounds = plain.bounds()
    Hm, Wm = plain.begin(bounds, blend=args.blend_depth)
    for i, v, J in chunks:
        plain.splat(v, J, i)
    over(plain)   # warm-up
    torch.cuda.synchronize()
    samples = int(plain.acc[:, 7].sum())
    print(f'mosaic {Wm} x {Hm} cells; unfeathered: {samples} samples')
    rows = [('accumulate, unfeathered (yardstick)', timed(lambda: plain.acc.zero_(), lambda: over(plain), args.reps))]

    for F in args.widths:
        m = engine.Mosaic(axes, gsd, dev)
        m.begin(bounds, blend=args.blend_depth, feather=F)
        m.key.copy_(plain.key)
        calls = []   # per call: its images, its table, its own buffer
        for i, v, J in chunks:
            arr, k, table, keep = m._images(v, J)
            buf = torch.empty(lib.sucre_mosaic_feather_bytes(k, arr), dtype=torch.uint8, device=dev)
            calls.append((i, arr, k, table, buf, keep))

        def feather_pass():
            for _, arr, k, table, buf, _ in calls:
                _lib.check(lib.sucre_mosaic_feather(C.c_void_p(table.data_ptr()), k, arr, F, C.c_void_p(buf.data_ptr()), stream()))

        def feathered():
            for i, arr, k, table, buf, _ in calls:
                _lib.check(lib.sucre_mosaic_accumulate_feathered(C.c_void_p(table.data_ptr()), k, arr, i, C.byref(m.grid), C.c_void_p(m.key.data_ptr()),
                                                                 C.c_float(float(m.inv_h)), F, C.c_void_p(buf.data_ptr()),
                                                                 C.c_void_p(m.acc.data_ptr()), 0, stream()))

        with torch.cuda.device(dev):
            feather_pass(), feathered()   # warm-up; the maps stay for the accumulate's repetitions
            torch.cuda.synchronize()
            direct = m.acc.clone()
            m.acc.zero_()
            over(m)
            torch.cuda.synchronize()
            assert torch.equal(m.acc, direct)
            near, part = (int(x) for x in m.feather_counts.cpu())
            print(f'F = {F}: {int(direct[:, 7].sum())} samples, {100.0 * near / max(1, part):.1f} % of the pixels that take part within F px of an edge, '
                  f'smallest weight sum in a filled cell {int(direct[:, 6][direct[:, 7] > 0].min())} / 4096')
            rows.append((f'F = {F}: feather pass', timed(lambda: None, feather_pass, args.reps)))
            rows.append((f'F = {F}: accumulate, feathered', timed(lambda: m.acc.zero_(), feathered, args.reps)))
            assert torch.equal(m.acc, direct)
            rows.append((f'F = {F}: Mosaic.accumulate (pass, counts, accumulate)', timed(lambda: m.acc.zero_(), lambda: over(m), args.reps)))
        del calls, m
    yard = rows[0][1][0]
    for name, (mean, low) in rows:
        print(f'{name:56s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / yard:5.2f} x the yardstick   '
              f'{n_px / mean / 1e6:7.1f} Gpixel/s')


if __name__ == '__main__':
    main()
