"""Times the pooled radix select (engine.pooled_percentiles, csrc/pool.hip) over the J of a synthetic survey against what the
per-image output stage spends on the same images (engine.count_valid + engine.select_ranks, csrc/plot.hip, once per image),
on the box it runs on, and prints both next to the byte floor of the four passes.

    python tools/exp/pool_select_time.py [--images 32] [--height 1080] [--width 1920] [--rounds 7] [--out FILE.json]

SUCRE_HIP_LIB selects the build (the product, or `make -C sucre_amd/csrc VARIANT=vote3 EXTRA=-DSUCRE_POOL_VOTE_ROUNDS=3`: the
pass kernel with the wave's vote in front of its LDS atomics).  Times are host clocks around work that ends in a device
synchronise, the two methods alternating, after one warm-up round; the four pass launches are also timed one by one with
device events.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from sucre_amd import _lib, engine          # noqa: E402
from sucre_amd.sucre import percentile_plan, percentile_plan64   # noqa: E402


def survey(n, H, W, dev):
    """Restored images as a fit leaves them: most values in [0.05, 2], a per-image cast, one per cent of invalid pixels."""
    Js = []
    for i in range(n):
        g = torch.Generator(device=dev).manual_seed(1000 + i)
        J = torch.rand((H, W, 3), generator=g, device=dev) ** 2 * (1.2 + 0.02 * (i % 7)) + 0.05 + 0.01 * (i % 5)
        bad = torch.rand((H, W), generator=g, device=dev) < 0.01
        J[bad] = float('nan')
        Js.append(J.contiguous())
    return Js


def per_image(Js):
    out = []
    for J in Js:
        n = engine.count_valid(J)
        plan = [percentile_plan(n, q) for q in (1, 99)]
        out.append(engine.select_ranks(J, [plan[0][0], plan[0][1], plan[1][0], plan[1][1]]))
    torch.cuda.synchronize()
    return out


def pooled(Js):
    P, n = engine.pooled_percentiles(Js)
    torch.cuda.synchronize()
    return P, n


def passes_alone(Js, n):
    """The four pass launches by device events (the ranks of the pooled 1st and 99th percentile, known beforehand)."""
    sel = engine.PoolSelect(Js[0].device)
    sel.begin()
    ranks = [r for q in (1.0, 99.0) for r in percentile_plan64(n, q)[:2]]
    ms = []
    for p in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sel.add(Js, p, n_ranks=4)
        b.record()
        sel.locate(p, ranks if p == 0 else None)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=32)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', type=Path)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs a GPU'
    dev = torch.device('cuda:0')
    Js = survey(a.images, a.height, a.width, dev)
    torch.cuda.synchronize()
    P, n = pooled(Js)          # warm-up of both
    per_image(Js)
    passes_alone(Js, n)
    t_pool, t_img, t_pass = [], [], []
    for _ in range(a.rounds):
        t0 = time.perf_counter(); pooled(Js); t1 = time.perf_counter(); per_image(Js); t2 = time.perf_counter()   # noqa: E702
        t_pool.append((t1 - t0) * 1e3)
        t_img.append((t2 - t1) * 1e3)
        t_pass.append(passes_alone(Js, n))
    px = a.images * a.height * a.width
    floor_bytes = 4 * 12 * px
    t_pass = np.asarray(t_pass)
    passes_ms = np.median(t_pass, axis=0)
    res = {
        'device': torch.cuda.get_device_name(0), 'library': str(_lib.LIB_PATH.name), 'images': a.images, 'height': a.height, 'width': a.width,
        'valid_pixels': int(n), 'P': np.asarray(P).tolist(),
        'pooled_percentiles_ms': {'median': float(np.median(t_pool)), 'min': float(min(t_pool)), 'max': float(max(t_pool))},
        'per_image_count_and_select_ms': {'median': float(np.median(t_img)), 'min': float(min(t_img)), 'max': float(max(t_img))},
        'pass_launch_ms_median': [float(x) for x in passes_ms], 'pass_launch_ms_min': [float(x) for x in t_pass.min(axis=0)],
        'four_passes_ms': float(passes_ms.sum()),
        'floor_bytes': floor_bytes, 'four_passes_TB_per_s': floor_bytes / (passes_ms.sum() * 1e-3) / 1e12,
        'rounds': a.rounds,
    }
    print(json.dumps(res))
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
