"""Time of the residual pass (sucre_fit_residuals) next to the fit it follows, in ONE process, at bench.py's config-2 shape
(1920x1080, 64 neighbours, seed 0, the f32 store): warm up, HIP events around 20 back-to-back ``residuals()`` calls, and in the
same run events around ``fit(20)`` of the same workspace.  The bar the pass is held to: no longer than 4 fit iterations of that
same run.

    python tools/residual_pass_time.py [--width 1920 --height 1080 --neighbours 64] > profiles/r07_residual_pass.txt
"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import engine, synth  # noqa: E402


def timed(fn, reps: int) -> float:
    """Milliseconds per call of ``fn`` over ``reps`` back-to-back calls, HIP events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--neighbours', type=int, default=64)
    ap.add_argument('--modes', default='plain,light')
    args = ap.parse_args()
    dev = 'cuda:0'
    scene = synth.make_scene(args.width, args.height, args.neighbours, seed=0, device=dev)
    views = engine.device_views_from_scene(scene, dev)
    print(f'{torch.cuda.get_device_name(0)}; {args.width}x{args.height}, {len(views)} views')
    for mode in args.modes.split(','):
        r = engine.Restoration(scene.height, scene.width, len(views), device=dev, light=mode == 'light')
        r.match(views[scene.target], views)
        r.fit_init(views[scene.target])
        r.fit(20, record_trace=False)          # warm-up of the fit kernels; the pass then sees a fitted J
        for _ in range(3):
            r.residuals()
        torch.cuda.synchronize()
        n_obs = r.n_obs()
        kept = int((r.view_keep() != 0).sum())
        t_pass = timed(r.residuals, 20)
        t_fit = timed(lambda: r.fit(20, record_trace=False), 1) / 20
        t_pass2 = timed(r.residuals, 20)
        count, ssr, stats = r.residuals()
        torch.cuda.synchronize()
        assert int(count.sum()) == n_obs == int(stats[:, 0].sum())
        tiles = ((args.width + 15) // 16) * ((args.height + 15) // 16)
        dense = tiles * kept * (1792 + (3072 if mode == 'light' else 0))
        print(f'[{mode}] {n_obs} observations over {kept} kept views; dense store read at most {dense / 1e6:.0f} MB')
        print(f'[{mode}] residual pass  {t_pass * 1e3:8.1f} us per call (20 back to back; again after the fit: {t_pass2 * 1e3:.1f} us)'
              f'  = {dense / 1e6 / t_pass:.0f} GB/s of the dense store')
        print(f'[{mode}] fit iteration  {t_fit * 1e3:8.1f} us (fit(20) of the same workspace, same run)')
        print(f'[{mode}] pass / iteration = {t_pass / t_fit:.2f} (bar: 4.00)  {"OK" if t_pass <= 4 * t_fit else "MISSED"}')
        del r
        engine.release_pool()
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
