"""Times of the mosaic's view-supported surface (sucre_mosaic_support, sucre_mosaic_support_top, sucre_mosaic_cull_supported) on
the shape of tools/mosaic_surface_time.py: 65 resident images of 1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0),
every J the single-view inversion at the renderer's water, the default frame and ground sample distance, three calls per phase
(32 + 32 + 1 images).  In ONE run, for M = 1 .. 4: every level of the ranks in its default form -- a load of the level's word that
filters the 64-bit atomic min -- and with the plain atomic for every pixel, the level's words reset before every repetition
outside the events and the levels below it final; ``finish_support``; the two-sided cull without and with its counts (``culled``,
``culled_above`` and ``support_counts`` zeroed outside the events).  And the yardsticks the surface test used: the surface phase
(``sucre_mosaic_surface``), the splat and ``sucre_invert_images`` on the same images.  The survey is a consistent 2.5-D scene, so
all of this is repeated for every factor of --biases with the depth map of every second image scaled by it (1.01: those views'
surface lies 3 cm lower), which gives the cull something to cull on either side.  The lines are printed and written to --out.

    python tools/mosaic_support_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --tolerance 0.005 --biases 1 1.01]
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
    ap.add_argument('--tolerance', type=float, default=0.005, help='tolerance T of the cull, metres')
    ap.add_argument('--biases', type=float, nargs='+', default=(1.0, 1.01), help='factors on the depth maps of every second image')
    ap.add_argument('--out', type=Path, default=Path(__file__).resolve().parent.parent / 'profiles' / 'mosaic_support_time.txt')
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
    say(f'{torch.cuda.get_device_name(0)}; {n} images of {args.width}x{args.height}, {n_px} pixels; gsd {float(gsd):.6g} m; T = {args.tolerance:g} m')
    chunks = []

    def over(phase, *a, **kw):
        for i, v, J in chunks:
            phase(v, J, i, *a, **kw)

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
        for M in range(1, engine.MOSAIC_SUPPORT_RANGE[1] + 1):
            Hm, Wm = m.begin(bounds, surface=args.tolerance, support=M)
            head = tag + f'M = {M}: '
            for level in range(M):
                over(m.add_support, level)   # warm-up; the result is the reference for the plain form and stays for the next level
                torch.cuda.synchronize()
                final = m.rank[level].clone()
                held = int((final != -1).sum())
                if M == engine.MOSAIC_SUPPORT_RANGE[1]:
                    say(tag + f'level {level}: {held} of {Hm * Wm} cells hold it ({100.0 * held / (Hm * Wm):.1f} %)')
                rows.append((head + f'level {level}, load then atomic',
                             timed(lambda: m.rank[level].fill_(-1), lambda: over(m.add_support, level), args.reps)))
                assert torch.equal(m.rank[level], final)
                rows.append((head + f'level {level}, plain atomic',
                             timed(lambda: m.rank[level].fill_(-1), lambda: over(m.add_support, level, plain_atomic=True), args.reps)))
                assert torch.equal(m.rank[level], final)
            m.finish_support()   # warm-up
            rows.append((head + 'finish_support', timed(nothing, m.finish_support, args.reps)))

            def reset():
                m.support_counts.zero_()
                m.result()['culled'].zero_()
                m.result()['culled_above'].zero_()

            reset()
            over(m.culled_images, count=True)   # warm-up, and the counts
            torch.cuda.synchronize()
            below, above, part = (int(x) for x in m.support_counts.cpu())
            out = m.result()
            say(head + f'{int(((out["support"] < M) & (out["support"] > 0)).sum())} of {int((out["support"] > 0).sum())} cells rest on fewer than '
                f'{M} views; {below} of {part} samples culled below ({100.0 * below / max(1, part):.1f} %), {above} above '
                f'({100.0 * above / max(1, part):.1f} %), in {int((out["culled"] > 0).sum())} and {int((out["culled_above"] > 0).sum())} cells')
            rows.append((head + 'two-sided cull', timed(nothing, lambda: over(m.culled_images), args.reps)))
            rows.append((head + 'two-sided cull with its counts', timed(reset, lambda: over(m.culled_images, count=True), args.reps)))
            assert [int(x) for x in m.support_counts.cpu()] == [below, above, part]
        m.begin(bounds, surface=args.tolerance)
        over(m.add_surface)   # warm-up
        torch.cuda.synchronize()
        rows.append((tag + 'sucre_mosaic_surface, load then atomic (yardstick)', timed(lambda: m.top.fill_(-1), lambda: over(m.add_surface), args.reps)))
        rows.append((tag + 'one-sided cull (yardstick)', timed(nothing, lambda: over(m.culled_images), args.reps)))

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
        say(f'{name:66s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / splat:5.2f} x the splat   '
            f'{mean / yard:5.2f} x invert_images   {n_px / mean / 1e6:7.1f} Gpixel/s')
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
