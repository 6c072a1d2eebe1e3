"""Times of the mosaic's surface test (sucre_mosaic_surface, sucre_mosaic_cull) on the shape of tools/mosaic_time.py: 65 resident
images of 1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the renderer's
water, the default frame and ground sample distance, three calls per phase (32 + 32 + 1 images).  In ONE run: the surface phase
in both forms -- a load of top[cell] that filters the 32-bit atomic min, and the plain atomic for every pixel
(SUCRE_MOSAIC_PLAIN_ATOMIC) --, with ``top`` reset before every repetition outside the events, and once more over tops that are
final already; for every tolerance of --tolerances the cull without and with its counts (``culled`` and ``surface_counts`` zeroed
outside the events); and the yardsticks: the splat in its default form and ``sucre_invert_images`` on the same images.  The
survey is a consistent 2.5-D scene, so a test culls next to nothing of it: all of this is repeated for every factor of --biases
with the depth map of every second image scaled by it (1.01: those views' surface lies 3 cm lower), which gives the cull its
culled pixels and their per-cell atomics.  The lines are printed and written to --out.

    python tools/mosaic_surface_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --tolerances 0.05 0.005 --biases 1 1.01]
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import engine, sucre, synth  # noqa: E402
from mosaic_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--grid', type=int, nargs=2, default=(13, 5))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--tolerances', type=float, nargs='+', default=(0.05, 0.005), help='tolerances T of the cull, metres')
    ap.add_argument('--biases', type=float, nargs='+', default=(1.0, 1.01), help='factors on the depth maps of every second image')
    ap.add_argument('--out', type=Path, default=Path(__file__).resolve().parent.parent / 'profiles' / 'mosaic_surface_time.txt')
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = 'cuda:0'
    survey = synth.make_survey(args.width, args.height, args.grid[0], args.grid[1], seed=0, device=dev)
    views = engine.device_views_from_scene(survey, dev)
    water = list(synth.GT_B) + list(synth.GT_BETA) + list(synth.GT_GAMMA)
    Js = engine.invert_images(views, water)
    n = len(views)
    axes = sucre.mosaic_axes(views)
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views]) * args.gsd_factor
    n_px = sum(v.depth.numel() for v in views)
    say(f'{torch.cuda.get_device_name(0)}; {n} images of {args.width}x{args.height}, {n_px} pixels; gsd {float(gsd):.6g} m')
    chunks = []

    def over(phase, **kw):
        for i, v, J in chunks:
            phase(v, J, i, **kw)

    true_views, rows, nothing = views, [], lambda: None   # noqa: E731
    for bias in args.biases:
        views = [v if k % 2 == 0 or bias == 1.0 else engine.DeviceView(depth=(v.depth * bias).contiguous(), rgb=v.rgb, K=v.K, R=v.R, t=v.t,
                                                                         name=v.name, Kinv=v.Kinv) for k, v in enumerate(true_views)]
        chunks = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]
        tag = f'depth x {bias:g}: '
        m = engine.Mosaic(axes, gsd, dev)
        for _, v, J in chunks:
            m.add_bounds(v, J)
        bounds = m.bounds()
        Hm, Wm = m.begin(bounds, surface=args.tolerances[0])
        over(m.add_surface)   # warm-up; the result is the reference for the plain form
        torch.cuda.synchronize()
        final_top = m.top.clone()
        filled = int((final_top != -1).sum())
        tops = m.result()['surface']
        say(tag + f'mosaic {Wm} x {Hm} cells, {filled} with a top ({100.0 * filled / (Hm * Wm):.1f} %), between {float(tops[~torch.isnan(tops)].min()):.6g} and '
            f'{float(tops[~torch.isnan(tops)].max()):.6g} m along the view axis')
        rows.append((tag + 'surface, load then atomic', timed(lambda: m.top.fill_(-1), lambda: over(m.add_surface), args.reps)))
        assert torch.equal(m.top, final_top)
        rows.append((tag + 'surface, plain atomic', timed(lambda: m.top.fill_(-1), lambda: over(m.add_surface, plain_atomic=True), args.reps)))
        assert torch.equal(m.top, final_top)
        rows.append((tag + 'surface over final tops, load then atomic', timed(nothing, lambda: over(m.add_surface), args.reps)))
        rows.append((tag + 'surface over final tops, plain atomic', timed(nothing, lambda: over(m.add_surface, plain_atomic=True), args.reps)))
        assert torch.equal(m.top, final_top)

        def reset():
            m.surface_counts.zero_()
            m.result()['culled'].zero_()

        for T in args.tolerances:
            m.surface = engine.mosaic_surface_tol(T)
            reset()
            over(m.culled_images, count=True)   # warm-up, and the counts of this tolerance
            torch.cuda.synchronize()
            gone, part = (int(x) for x in m.surface_counts.cpu())
            say(tag + f'T = {T:g} m: {gone} of {part} samples culled ({100.0 * gone / max(1, part):.1f} %), in {int((m.result()["culled"] > 0).sum())} cells')
            rows.append((tag + f'T = {T:g}: cull', timed(nothing, lambda: over(m.culled_images), args.reps)))
            rows.append((tag + f'T = {T:g}: cull with its counts', timed(reset, lambda: over(m.culled_images, count=True), args.reps)))
            assert [int(x) for x in m.surface_counts.cpu()] == [gone, part]

    views = true_views
    chunks[:] = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]
    plain = engine.Mosaic(axes, gsd, dev)
    for _, v, J in chunks:
        plain.add_bounds(v, J)
    plain.begin()
    over(plain.splat)   # warm-up
    torch.cuda.synchronize()
    rows.append(('splat, load then atomic (yardstick)', timed(lambda: plain.key.fill_(-1), lambda: over(plain.splat), args.reps)))
    for _ in range(2):
        engine.invert_images(views, water)
    torch.cuda.synchronize()
    rows.append(('invert_images (yardstick)', timed(nothing, lambda: engine.invert_images(views, water), args.reps)))
    splat, yard = rows[-2][1][0], rows[-1][1][0]
    for name, (mean, low) in rows:
        say(f'{name:60s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / splat:5.2f} x the splat   '
            f'{mean / yard:5.2f} x invert_images   {n_px / mean / 1e6:7.1f} Gpixel/s')
    f, p = rows[0][1][0], rows[1][1][0]
    say(f'{rows[0][0]} / plain atomic = {f / p:.2f}; / the splat = {f / splat:.2f}')
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
