"""Times of the phases of the seabed mosaic (sucre_mosaic_*) on a resident survey: 65 images of 1920x1080 from
``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the renderer's water, the default frame and
ground sample distance.  Every phase runs over all images (three calls: 32 + 32 + 1 images) between two HIP events, with its
words reset before every repetition outside the events; the splat is timed in both forms -- a load of key[cell] that filters the
64-bit atomic min, and the plain atomic for every pixel (SUCRE_MOSAIC_PLAIN_ATOMIC) -- and once more over keys that are final
already (what the filter costs when it filters everything).  The blend's two phases follow in the same run: the accumulate phase
(sucre_mosaic_accumulate at the blend depth --blend-depth) in both forms -- the sums of every run of a wave's lanes that share a
cell, then eight atomics per run; and eight atomics per pixel (SUCRE_MOSAIC_PLAIN_ATOMIC) -- with the accumulator zeroed before
every repetition outside the events, and the per-cell normalise pass.  The yardstick, in the same run: ``sucre_invert_images`` on the same
images -- the same reads (depth, colours), plain streaming writes of J, no atomics.

    python tools/mosaic_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --blend-depth 0.5]
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import engine, sucre, synth  # noqa: E402


def timed(prepare, fn, reps: int):
    """(mean, min) milliseconds of ``fn`` over ``reps`` repetitions, each between its own pair of HIP events, ``prepare`` before each."""
    pairs = []
    for _ in range(reps):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in pairs]
    return sum(ms) / len(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--grid', type=int, nargs=2, default=(13, 5))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--blend-depth', type=float, default=0.5, help='blend depth H of the accumulate phase, metres')
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
    n_in = sum(int(((v.depth > 0) & ~torch.isnan(J).any(dim=2)).sum()) for v, J in zip(views, Js))
    print(f'{torch.cuda.get_device_name(0)}; {n} images of {args.width}x{args.height}, {n_px} pixels, {n_in} take part; gsd {float(gsd):.6g} m')

    chunks = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]
    m = engine.Mosaic(axes, gsd, dev)

    def over(phase, **kw):
        for i, v, J in chunks:
            phase(v, J, i, **kw)

    def bounds():
        for _, v, J in chunks:
            m.add_bounds(v, J)

    fresh_words = torch.tensor([-1, -1, 0, 0], dtype=torch.int32, device=dev)
    bounds()
    Hm, Wm = m.begin(blend=args.blend_depth)
    over(m.splat), over(m.resolve), over(m.gather)   # warm-up of every kernel; the result is the reference for the variants
    torch.cuda.synchronize()
    final_key, final_pix = m.key.clone(), m.pix.clone()
    filled = int((m.result()['source'] >= 0).sum())
    print(f'mosaic {Wm} x {Hm} cells, {filled} filled ({100.0 * filled / (Hm * Wm):.1f} %), {n_in / max(1, filled):.1f} pixels that take part per filled cell')

    nothing = lambda: None   # noqa: E731
    rows = [('bounds', timed(lambda: m.bounds_words.copy_(fresh_words), bounds, args.reps)),
            ('splat, load then atomic', timed(lambda: m.key.fill_(-1), lambda: over(m.splat), args.reps))]
    assert torch.equal(m.key, final_key)
    rows.append(('splat, plain atomic', timed(lambda: m.key.fill_(-1), lambda: over(m.splat, plain_atomic=True), args.reps)))
    assert torch.equal(m.key, final_key)
    rows.append(('splat over final keys, load then atomic', timed(nothing, lambda: over(m.splat), args.reps)))
    rows.append(('splat over final keys, plain atomic', timed(nothing, lambda: over(m.splat, plain_atomic=True), args.reps)))
    assert torch.equal(m.key, final_key)
    rows.append(('resolve', timed(lambda: m.pix.fill_(-1), lambda: over(m.resolve), args.reps)))
    assert torch.equal(m.pix, final_pix)
    rows.append(('gather', timed(nothing, lambda: over(m.gather), args.reps)))
    over(m.accumulate)   # warm-up; its sums are the reference for the plain form
    torch.cuda.synchronize()
    final_acc = m.acc.clone()
    samples = int(final_acc[:, 7].sum())
    print(f'blend depth {args.blend_depth:g} m: {samples} samples ({100.0 * samples / max(1, n_in):.1f} % of the pixels that take part), '
          f'{samples / max(1, filled):.1f} per filled cell, {int(final_acc[:, 7].max())} at most')
    rows.append(('accumulate, run sums then atomics', timed(lambda: m.acc.zero_(), lambda: over(m.accumulate), args.reps)))
    assert torch.equal(m.acc, final_acc)
    rows.append(('accumulate, plain atomics', timed(lambda: m.acc.zero_(), lambda: over(m.accumulate, plain=True), args.reps)))
    assert torch.equal(m.acc, final_acc)
    m.normalize()   # warm-up (and the check of the largest count)
    rows.append(('normalize', timed(nothing, lambda: m.normalize(check=False), args.reps)))
    for _ in range(2):
        engine.invert_images(views, water)
    torch.cuda.synchronize()
    rows.append(('invert_images (yardstick)', timed(nothing, lambda: engine.invert_images(views, water), args.reps)))
    yard = rows[-1][1][0]
    for name, (mean, low) in rows:
        print(f'{name:42s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / yard:5.2f} x the yardstick   '
              f'{n_px / mean / 1e6:7.1f} Gpixel/s')
    f, p = rows[1][1][0], rows[2][1][0]
    print(f'splat: load then atomic / plain atomic = {f / p:.2f}')
    by_name = {name: mean for name, (mean, _) in rows}
    a, ap_ = by_name['accumulate, run sums then atomics'], by_name['accumulate, plain atomics']
    print(f'accumulate / splat = {a / f:.2f} (run sums), {ap_ / f:.2f} (plain); accumulate: run sums / plain = {a / ap_:.2f}')


if __name__ == '__main__':
    main()
