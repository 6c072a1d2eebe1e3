"""Time of the single-view inversion (sucre_invert_images) next to a device-to-device copy of the same bytes, in ONE process:
HIP events around 20 launches of 32 1920x1080 images (uint8 colours, water model; --light for the light model) and around 20
copies of the 19 bytes per pixel the kernel moves (4 depth + 3 colour read, 12 of J written: a copy of 9.5 B per pixel reads and
writes as much).  The kernel is elementwise, so it should sit near the copy's time; no bar is set, the ratio is recorded.

    python tools/invert_time.py [--width 1920 --height 1080 --images 32 --light] > profiles/r09_invert.txt
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
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--light', action='store_true')
    args = ap.parse_args()
    dev = 'cuda:0'
    scene = synth.make_scene(args.width, args.height, 3, seed=0, device=dev)
    base = engine.device_views_from_scene(scene, dev)
    # every image of the launch has its own pixels (no two of them share cache lines)
    views = [engine.DeviceView(depth=base[i % len(base)].depth.clone(), rgb=base[i % len(base)].rgb.clone(), K=scene.K,
                               R=base[i % len(base)].R, t=base[i % len(base)].t) for i in range(args.images)]
    params = [.094, .121, .119, .321, .073, .072, .140, .137, .142]
    if args.light:
        params += [0.02, -0.03, 0.01, 0.05, -0.04, 0.03, 0.9, 0.1, -0.05, 1.1]
    print(f'{torch.cuda.get_device_name(0)}; {args.images} images of {args.width}x{args.height} per launch, '
          f'{"light model" if args.light else "water model"}, uint8 colours')
    for _ in range(3):
        engine.invert_images(views, params, light=args.light)
    torch.cuda.synchronize()
    t_inv = timed(lambda: engine.invert_images(views, params, light=args.light), args.reps)
    n_px = args.images * args.width * args.height
    moved = 19 * n_px
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    t_copy = timed(lambda: dst.copy_(src), args.reps)
    print(f'invert {t_inv * 1e3:9.1f} us per launch ({args.reps} back to back, output allocation and table included) = {moved / 1e6 / t_inv:.0f} GB/s')
    print(f'copy   {t_copy * 1e3:9.1f} us per copy of {moved // 2} bytes (reads and writes {moved / 1e6:.0f} MB) = {moved / 1e6 / t_copy:.0f} GB/s')
    print(f'invert / copy = {t_inv / t_copy:.2f} (near 1 expected; no bar)')


if __name__ == '__main__':
    main()
