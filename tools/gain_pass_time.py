"""Time of the per-view gain passes (sucre_view_gains, sucre_apply_view_gains) next to the residual pass and the fit they follow,
in ONE process, at bench.py's config-2 shape (1920x1080, 64 neighbours, seed 0, the f32 store).  The apply changes the store, so
each of its timed calls runs on a fresh copy of one fitted workspace (the copy is outside the events) with the gains estimated
from it, times 0.9 so that every colour is rewritten; HIP events go around every apply call, around 20 back-to-back ``view_gains()`` and ``residuals()`` calls and around
``fit(20)`` of the same workspace.  The expectation (no bar): the estimate costs about a residual pass (same bytes, same model),
the apply less (no model, no J; it reads ranges and colours and writes back only colours that changed).

    python tools/gain_pass_time.py [--width 1920 --height 1080 --neighbours 64] > profiles/r10_gain_pass.txt

Under ``rocprofv3 --kernel-trace --stats -- python tools/gain_pass_time.py`` the kernel statistics of the same run give the two
new kernels' own durations (gain_sum_kernel, gain_apply_kernel) next to residual_kernel's.
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import _lib, engine, synth  # noqa: E402

from residual_pass_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--neighbours', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = 'cuda:0'
    scene = synth.make_scene(args.width, args.height, args.neighbours, seed=0, device=dev)
    views = engine.device_views_from_scene(scene, dev)
    print(f'{torch.cuda.get_device_name(0)}; {args.width}x{args.height}, {len(views)} views')
    r = engine.Restoration(scene.height, scene.width, len(views), device=dev)
    r.match(views[scene.target], views)
    r.fit_init(views[scene.target])
    r.fit(20, record_trace=False)          # warm-up of the fit kernels; the passes then see a fitted J
    for _ in range(3):
        r.residuals()
        gains, inv, sums = r.view_gains()
    torch.cuda.synchronize()
    n_obs = r.n_obs()
    kept = int((r.view_keep() != 0).sum())
    t_res = timed(r.residuals, args.reps)
    t_est = timed(r.view_gains, args.reps)
    t_fit = timed(lambda: r.fit(20, record_trace=False), 1) / 20
    gains, inv, sums = r.view_gains()
    inv = (inv * 0.9).contiguous()         # a clean scene's gains are 1 to three digits: time an apply that rewrites every colour
    saved = r.ws.clone()

    lib = r.lib
    clipped = torch.empty(r.n_views, dtype=torch.int64, device=dev)
    scratch = torch.empty(lib.sucre_gain_scratch_bytes(r.H, r.W, r.n_views), dtype=torch.uint8, device=dev)

    def apply_only():
        _lib.check(lib.sucre_apply_view_gains(C.c_void_p(r.ws.data_ptr()), r.H, r.W, r.n_views, C.c_void_p(inv.data_ptr()),
                                              C.c_void_p(clipped.data_ptr()), C.c_void_p(scratch.data_ptr()), r._sp()))

    def over_copies(fn):
        total = 0.0
        for i in range(args.reps + 2):       # two warm-up passes
            r.ws.copy_(saved)
            t = timed(fn, 1)
            total += t if i >= 2 else 0.0
        return total / args.reps

    t_apply = over_copies(apply_only)
    t_round = over_copies(lambda: r.apply_view_gains(inv))
    torch.cuda.synchronize()
    assert r.n_obs() == n_obs == int(sums[:, 0].sum())
    g = gains[r.view_keep() != 0]
    tiles = ((args.width + 15) // 16) * ((args.height + 15) // 16)
    dense = tiles * kept * 1792
    print(f'{n_obs} observations over {kept} kept views; gains {float(g.min()):.4f} .. {float(g.max()):.4f}, {int(clipped.sum())} values clipped; '
          f'a pass reads at most {dense / 1e6:.0f} MB of the dense store')
    print(f'residual pass    {t_res * 1e3:8.1f} us per call ({args.reps} back to back) = {dense / 1e6 / t_res:.0f} GB/s')
    print(f'gain estimate    {t_est * 1e3:8.1f} us per call ({args.reps} back to back) = {dense / 1e6 / t_est:.0f} GB/s')
    print(f'gain apply       {t_apply * 1e3:8.1f} us per call ({args.reps} calls, each on a fresh copy of the store)')
    print(f'apply + finalise {t_round * 1e3:8.1f} us per call (Restoration.apply_view_gains)')
    print(f'fit iteration    {t_fit * 1e3:8.1f} us (fit(20) of the same workspace, same run)')
    print(f'estimate / residual pass = {t_est / t_res:.2f}, apply / residual pass = {t_apply / t_res:.2f} (no bar)')


if __name__ == '__main__':
    main()
