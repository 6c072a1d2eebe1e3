"""Times of the multi-band blend (sucre_mosaic_band_split, sucre_mosaic_band_combine) on the shape of tools/mosaic_time.py: 65
resident images of 1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the
renderer's water, the default frame and ground sample distance, three calls per phase (32 + 32 + 1 images).  In ONE run: every
level s = 1 .. 32 of the split alone (three band buffers per call, made before the events; level j reads the S that level j - 1
left, so every level runs on its true input), all K levels together, one band's accumulate pass (the residual's: the blend's
own weights, the band as J), the combine pass, and the whole phase at K as a caller runs it (``Mosaic.accumulate_bands`` over the
batches, then ``combine_bands``).  The yardsticks, in the same run: ``invert_images`` (a streaming pass over the same images) and
the blend's accumulate.  The accumulators are zeroed before every repetition outside the events.

    python tools/mosaic_bands_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --blend-depth 0.5 --bands 4]
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
    ap.add_argument('--blend-depth', type=float, default=0.5, help='blend depth H, metres')
    ap.add_argument('--bands', type=int, default=4, help='detail bands K of the whole phase')
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
          f'blend depth {args.blend_depth:g} m; K = {args.bands}')
    chunks = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]
    lib = _lib.load()
    stream = engine._stream_ptr
    K, levels = args.bands, engine.MOSAIC_BANDS_RANGE[1]

    m = engine.Mosaic(axes, gsd, dev)
    for _, v, J in chunks:
        m.add_bounds(v, J)
    Hm, Wm = m.begin(blend=args.blend_depth, bands=K)
    for i, v, J in chunks:
        m.splat(v, J, i)
    for i, v, J in chunks:
        m.accumulate(v, J, i)
    m.normalize()
    torch.cuda.synchronize()
    print(f'mosaic {Wm} x {Hm} cells; blend: {int(m.acc[:, 7].sum())} samples; band plan {[(float(h), f) for h, f in m.band_plan]}')

    calls = []   # per call: its images, its table, three band buffers of its own
    for i, v, J in chunks:
        arr, k, table, keep = m._images(v, J)
        bufs = [torch.empty(lib.sucre_mosaic_band_bytes(k, arr) // 4, dtype=torch.float32, device=dev) for _ in range(3)]
        calls.append((i, arr, k, table, bufs, keep))

    def split(level):
        for _, arr, k, table, (Sa, Sb, D), _ in calls:
            S = (Sa, Sb)
            S_in = None if level == 0 else C.c_void_p(S[(level - 1) % 2].data_ptr())
            _lib.check(lib.sucre_mosaic_band_split(C.c_void_p(table.data_ptr()), k, arr, level, S_in, C.c_void_p(S[level % 2].data_ptr()),
                                                   C.c_void_p(D.data_ptr()), stream()))

    def whole():
        for i, v, J in chunks:
            m.accumulate_bands(v, J, i)
        m.combine_bands()

    nothing = lambda: None   # noqa: E731
    with torch.cuda.device(dev):
        rows = []
        for level in range(levels):     # in order: level j times on the S that level j - 1 left in the other buffer
            split(level)                # warm-up, and the input of the next level
            rows.append((f'band_split, level {level} (s = {1 << level})', timed(nothing, lambda: split(level), args.reps)))
        rows.append((f'band_split, levels 0 .. {K - 1} together', timed(nothing, lambda: [split(level) for level in range(K)], args.reps)))
        whole()                         # warm-up; its sums are the reference of the repetitions
        torch.cuda.synchronize()
        final = m.acc_bands.clone()
        assert torch.equal(final[K, :, 3:], m.acc[:, 3:])
        residual = m.acc_bands[K]

        def one_band():                 # the residual of the calls' own stacks: S_K lies in the buffer level K - 1 wrote
            for i, arr, k, table, bufs, keep in calls:
                band = (_lib.MosaicImage * k)()
                C.memmove(band, arr, C.sizeof(band))
                at = 0
                for e in band:
                    e.J = bufs[(K - 1) % 2].data_ptr() + at * 12
                    at += -(-(e.H * e.W) // _lib.MOSAIC_BLOCK_PX) * _lib.MOSAIC_BLOCK_PX
                _lib.check(lib.sucre_mosaic_accumulate(C.c_void_p(table.data_ptr()), k, band, i, C.byref(m.grid), C.c_void_p(m.key.data_ptr()),
                                                       C.c_float(float(m.inv_h)), C.c_void_p(residual.data_ptr()), 0, stream()))

        for level in range(K):
            split(level)
        rows.append(('accumulate of one band (the residual)', timed(lambda: residual.zero_(), one_band, args.reps)))
        assert torch.equal(m.acc_bands[K], final[K])
        rows.append(('band_combine', timed(nothing, m.combine_bands, args.reps)))
        rows.append((f'whole phase, K = {K} (accumulate_bands over the batches, combine_bands)', timed(lambda: m.acc_bands.zero_(), whole, args.reps)))
        assert torch.equal(m.acc_bands, final)
        rows.append(('accumulate of the blend (yardstick)', timed(lambda: m.acc.zero_(), lambda: [m.accumulate(v, J, i) for i, v, J in chunks], args.reps)))
        for _ in range(2):
            engine.invert_images(views, water)
        torch.cuda.synchronize()
        rows.append(('invert_images (yardstick)', timed(nothing, lambda: engine.invert_images(views, water), args.reps)))
    yard = rows[-1][1][0]
    for name, (mean, low) in rows:
        print(f'{name:76s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / yard:6.2f} x invert_images   '
              f'{n_px / mean / 1e6:7.1f} Gpixel/s')
    by_name = {name: mean for name, (mean, _) in rows}
    together, band = by_name[f'band_split, levels 0 .. {K - 1} together'], by_name['accumulate of one band (the residual)']
    print(f'the {K} split levels together / one band\'s accumulate = {together / band:.2f}')
    # what a level moves at the least: level 0 reads depth and J (16 bytes per pixel), a later level S_in (12); both write S_out and D_out (24)
    for level in range(levels):
        mean = rows[level][1][0]
        moved = (16 if level == 0 else 12) + 24
        print(f'level {level}: {moved} bytes per pixel read once and written, {moved * n_px / mean / 1e9:.2f} TB/s if every tap but the first is served '
              f'by a cache; {(9 * (16 if level == 0 else 12) + 24) * n_px / mean / 1e9:.2f} TB/s of requests with all nine taps counted')


if __name__ == '__main__':
    main()
