"""Time of the cross-view consistency check (sucre_view_consistency) at bench.py's config-2 shape (1920x1080, 64 neighbours,
seed 0): the target of ``synth.make_scene`` against its 64 neighbours, every J the single-view inversion at the renderer's
water.  Warm up, HIP events around 20 back-to-back calls, and in the same run events around ``sucre_match_views`` of the same
target for scale.  The bytes are those of DESIGN.md's model, counted here from the matches and the valid pairs themselves.

    python tools/consistency_time.py [--width 1920 --height 1080 --neighbours 64]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o consist -- python tools/consistency_time.py --reps 5   (kernel times; a run of its own)
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import _lib, engine, synth  # noqa: E402


def timed(fn, reps: int) -> float:
    """Milliseconds per call of ``fn`` over ``reps`` back-to-back calls, HIP events on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def model_bytes(H, W, maps, J_A, Js):
    """(bytes, matches, valid pairs, (wave, view) pairs -- a wave owns four rows of a 16x16 tile --, those with a valid pair) of
    DESIGN.md's byte model."""
    ty, tx = (H + 15) // 16, (W + 15) // 16
    nan_a = torch.isnan(J_A).any(dim=2)
    matches = valid_pairs = active = 0
    for m, J in zip(maps, Js):
        hit = m >= 0
        q = m.clamp(min=0).long()
        valid = hit & ~nan_a & ~torch.isnan(J).any(dim=2).view(-1)[q]
        matches += int(hit.sum())
        valid_pairs += int(valid.sum())
        padded = torch.zeros((ty * 16, tx * 16), dtype=torch.bool, device=m.device)
        padded[:H, :W] = valid
        active += int(padded.view(ty * 4, 4, tx, 16).any(dim=3).any(dim=1).sum())
    pairs = ty * tx * 4 * len(maps)
    total = H * W * (4 + 12 + 3) + H * W * (4 + 12) + matches * (4 + 12 + 3) + pairs * (4 + 4) + active * (96 + 96) + len(maps) * 26 * 8
    return total, matches, valid_pairs, pairs, active


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--neighbours', type=int, default=64)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    dev = 'cuda:0'
    scene = synth.make_scene(args.width, args.height, args.neighbours, seed=0, device=dev)
    every = engine.device_views_from_scene(scene, dev)
    water = list(synth.GT_B) + list(synth.GT_BETA) + list(synth.GT_GAMMA)
    restored = engine.invert_images(every, water)
    target, J_A = every[scene.target], restored[scene.target]
    views = [v for i, v in enumerate(every) if i != scene.target]
    Js = [J for i, J in enumerate(restored) if i != scene.target]
    H, W, n = scene.height, scene.width, len(views)
    print(f'{torch.cuda.get_device_name(0)}; {W}x{H} target, {n} neighbours')

    call = lambda: engine.view_consistency(target, J_A, views, Js)   # noqa: E731
    for _ in range(3):
        count, ssd, stats = call()
    torch.cuda.synchronize()
    t_call = timed(call, args.reps)

    r = engine.Restoration(H, W, n, device=dev)
    r.match(target, views, packed=False)   # uploads the view table (plain planes, as the check reads them) and warms the kernel up
    ws, _, _, _ = r._geom
    tgt = target.to_struct()
    match = lambda: _lib.check(r.lib.sucre_match_views(ws, H, W, n, C.byref(tgt), C.c_void_p(r._views_dev.data_ptr()), 0, n, r._sp()))   # noqa: E731
    for _ in range(3):
        match()
    torch.cuda.synchronize()
    t_match = timed(match, args.reps)
    t_call2 = timed(call, args.reps)

    maps = [r.match_map(k) for k in range(n)]
    total, matches, valid_pairs, pairs, active = model_bytes(H, W, maps, J_A, Js)
    assert matches == int(stats[:, 0].sum()) and valid_pairs == int(stats[:, 1].sum()) == int(count.sum())
    print(f'{matches} matches, {valid_pairs} valid pairs; {active} of {pairs} (wave, view) pairs hold a valid pair')
    print(f'byte model: {total / 1e6:.1f} MB')
    print(f'view_consistency  {t_call * 1e3:8.1f} us per call ({args.reps} back to back, device events; host staging of the view table '
          f'included; again after the match: {t_call2 * 1e3:.1f} us)  = {total / 1e6 / t_call:.0f} GB/s of the model\'s bytes')
    print(f'sucre_match_views {t_match * 1e3:8.1f} us per call (same target and views, plain planes, same run)')
    print(f'consistency / match = {t_call / t_match:.2f}')


if __name__ == '__main__':
    main()
