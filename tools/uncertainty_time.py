"""Time of the uncertainty pass (sucre_fit_uncertainty; csrc/uncertainty.h) next to the residual pass whose skeleton it shares and
next to the fit it follows, in ONE run, at bench.py's config-2 shape (1920x1080, 64 neighbours = 65 views, seed 0, the f32 store):
warm up, HIP events around ``--reps`` back-to-back ``uncertainty()`` calls, the same around ``residuals()``, and around ``fit(20)``
of the same workspace.  The expectation was set before any run (the issue of this feature): the pass is FP64-bound, not
byte-bound -- about 100 double operations and two double exponentials per observation and channel --, so several times the
residual pass's time and well under one fit's (200 iterations).  The lines are printed and written to --out; nothing is asserted
about the times.  What the figures can show is whether the pass is byte-bound (its GB/s of the dense store next to the residual
pass's over the same bytes); they cannot tell FP64 throughput from latency -- the TFLOP/s line is a nominal count, and no
counters are collected.

    python tools/uncertainty_time.py [--width 1920 --height 1080 --neighbours 64 --reps 10]
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import engine, synth  # noqa: E402
from residual_pass_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--neighbours', type=int, default=64)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--formats', default='f32,u16mm')
    ap.add_argument('--out', type=Path, default=Path(__file__).resolve().parent.parent / 'profiles' / 'uncertainty_time.txt')
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = 'cuda:0'
    scene = synth.make_scene(args.width, args.height, args.neighbours, seed=0, device=dev)
    views = engine.device_views_from_scene(scene, dev)
    say(f'{torch.cuda.get_device_name(0)}; {args.width}x{args.height}, {len(views)} views')
    for fmt in args.formats.split(','):
        r = engine.Restoration(scene.height, scene.width, len(views), device=dev, obs_format=fmt)
        r.match(views[scene.target], views)
        r.fit_init(views[scene.target])
        r.fit(20, record_trace=False)          # warm-up of the fit kernels; the passes then see a fitted J
        for _ in range(2):
            r.residuals()
            r.uncertainty()
        torch.cuda.synchronize()
        n_obs = r.n_obs()
        kept = int((r.view_keep() != 0).sum())
        t_res = timed(r.residuals, args.reps)
        t_unc = timed(r.uncertainty, args.reps)
        t_fit = timed(lambda: r.fit(20, record_trace=False), 1) / 20
        t_unc2 = timed(r.uncertainty, args.reps)
        count, jterms, sums = r.uncertainty()
        res = engine.water_uncertainty(sums)
        assert int(count.sum()) == n_obs == int(sums[0])
        tiles = ((args.width + 15) // 16) * ((args.height + 15) // 16)
        dense = tiles * kept * 1792
        flops = 3 * n_obs * 100
        say(f'[{fmt}] {n_obs} observations over {kept} kept views; dense store read at most {dense / 1e6:.0f} MB; '
            f'se(B, beta, gamma) red {res["se"][0]}, cond {res["cond"]}')
        say(f'[{fmt}] residual pass     {t_res * 1e3:9.1f} us per call ({args.reps} back to back) = {dense / 1e6 / t_res:.0f} GB/s of the dense store')
        say(f'[{fmt}] uncertainty pass  {t_unc * 1e3:9.1f} us per call ({args.reps} back to back; again after the fit: {t_unc2 * 1e3:.1f} us)'
            f' = {dense / 1e6 / t_unc:.0f} GB/s of the dense store, {flops / 1e9 / t_unc:.2f} TFLOP/s at 100 double operations per '
            f'observation and channel (the two exponentials not counted)')
        say(f'[{fmt}] fit iteration     {t_fit * 1e3:9.1f} us (fit(20) of the same workspace, same run); a fit of 200: {t_fit * 200:.1f} ms')
        say(f'[{fmt}] uncertainty / residual = {t_unc / t_res:.2f}; uncertainty / fit of 200 iterations = {t_unc / (200 * t_fit):.3f}')
        del r
        engine.release_pool()
        torch.cuda.empty_cache()
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
