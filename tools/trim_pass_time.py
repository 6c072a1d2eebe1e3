"""Time of the outlier trim (sucre_trim_outliers) next to the residual pass it takes its scale from and the fit it follows, in
ONE process, at bench.py's config-2 shape (1920x1080, 64 neighbours, seed 0, the f32 store).  The trim changes the store, so
each of its 20 timed passes runs on a fresh copy of one fitted workspace (the copy is outside the events); HIP events go
around every trim call, around 20 back-to-back ``residuals()`` calls and around ``fit(20)`` of the same workspace.  What the
trim is compared with is the residual pass of the same run: it evaluates the same arithmetic twice over the same bytes, so a
ratio of about 2 is expected (no bar).  The re-finalise behind the trim (``Restoration.trim_outliers`` runs both) is timed too.

    python tools/trim_pass_time.py [--width 1920 --height 1080 --neighbours 64 --k 3] > profiles/r08_trim_pass.txt
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
    ap.add_argument('--k', type=float, default=3.0)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = 'cuda:0'
    scene = synth.make_scene(args.width, args.height, args.neighbours, seed=0, device=dev)
    views = engine.device_views_from_scene(scene, dev)
    print(f'{torch.cuda.get_device_name(0)}; {args.width}x{args.height}, {len(views)} views, k = {args.k}')
    r = engine.Restoration(scene.height, scene.width, len(views), device=dev)
    r.match(views[scene.target], views)
    r.fit_init(views[scene.target])
    r.fit(20, record_trace=False)          # warm-up of the fit kernels; the passes then see a fitted J
    for _ in range(3):
        res = r.residuals()
    torch.cuda.synchronize()
    n_obs = r.n_obs()
    kept = int((r.view_keep() != 0).sum())
    t_res = timed(r.residuals, args.reps)
    t_fit = timed(lambda: r.fit(20, record_trace=False), 1) / 20
    res = r.residuals()
    saved = r.ws.clone()

    lib = r.lib
    dropped = torch.empty((r.H, r.W), dtype=torch.int32, device=dev)
    view_dropped = torch.empty(r.n_views, dtype=torch.int64, device=dev)
    tau2 = torch.empty(3, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.sucre_trim_scratch_bytes(r.H, r.W, r.n_views), dtype=torch.uint8, device=dev)

    def trim_only():
        _lib.check(lib.sucre_trim_outliers(C.c_void_p(r.ws.data_ptr()), r.H, r.W, r.n_views, r._fmt, args.k,
                                           C.c_void_p(res[2].data_ptr()), C.c_void_p(dropped.data_ptr()),
                                           C.c_void_p(view_dropped.data_ptr()), C.c_void_p(tau2.data_ptr()),
                                           C.c_void_p(scratch.data_ptr()), r._sp()))

    def over_copies(fn):
        total = 0.0
        for i in range(args.reps + 2):       # two warm-up passes
            r.ws.copy_(saved)
            t = timed(fn, 1)
            total += t if i >= 2 else 0.0
        return total / args.reps

    t_trim = over_copies(trim_only)
    n_dropped = int(view_dropped.sum())
    t_round = over_copies(lambda: r.trim_outliers(args.k, res))
    torch.cuda.synchronize()
    assert r.n_obs() == n_obs - n_dropped
    tiles = ((args.width + 15) // 16) * ((args.height + 15) // 16)
    dense = tiles * kept * 1792
    print(f'{n_obs} observations over {kept} kept views, {n_dropped} dropped; one sweep reads at most {dense / 1e6:.0f} MB of the dense store')
    print(f'residual pass   {t_res * 1e3:8.1f} us per call ({args.reps} back to back) = {dense / 1e6 / t_res:.0f} GB/s')
    print(f'trim            {t_trim * 1e3:8.1f} us per call ({args.reps} calls, each on a fresh copy of the store)')
    print(f'trim + finalise {t_round * 1e3:8.1f} us per call (Restoration.trim_outliers with the residuals handed in)')
    print(f'fit iteration   {t_fit * 1e3:8.1f} us (fit(20) of the same workspace, same run)')
    print(f'trim / residual pass = {t_trim / t_res:.2f} (two sweeps: about 2 expected; no bar)')


if __name__ == '__main__':
    main()
