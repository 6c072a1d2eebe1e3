"""Times of the mosaic's hole filling (sucre_mosaic_fill_pull / _push) on the resident survey of tools/mosaic_time.py: 65 images of
1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the renderer's water, the
default frame, the default ground sample distance times --gsd-factor.  The mosaic is made once (all four phases); then, on a warm
run, the pull (L launches) and the push (L launches) each between two HIP events, next to the bytes each pass moves and next to
the gather phase over all images in the same run.  The bytes: 19 per cell of level 0 (J, raw, source in; J_filled, raw_filled,
fill_level out), 32 per record.  The pull reads and writes every array it touches once: its bytes are the least it can move.
The push reads the taps of EMPTY cells only and, above level 0, one word of a cell that holds something, so its traffic depends
on the holes: given are a lower count (level 0 in and out, the w word of every record of the levels 1..L-1, no tap) and an
upper one (every record of every level read whole, once as taps and once in place).

    python tools/mosaic_fill_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --gsd-factor 1 --fill-cells 8]
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import _lib, engine, sucre, synth  # noqa: E402
from tools.mosaic_time import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--grid', type=int, nargs=2, default=(13, 5))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--fill-cells', type=float, default=8.0, help='the reach R of the fill, in cells (R = this x gsd): 8 gives L = 3')
    args = ap.parse_args()
    dev = 'cuda:0'
    survey = synth.make_survey(args.width, args.height, args.grid[0], args.grid[1], seed=0, device=dev)
    views = engine.device_views_from_scene(survey, dev)
    water = list(synth.GT_B) + list(synth.GT_BETA) + list(synth.GT_GAMMA)
    Js = engine.invert_images(views, water)
    axes = sucre.mosaic_axes(views)
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views]) * args.gsd_factor
    m = engine.mosaic_of(views, Js, axes, gsd)
    R = args.fill_cells * float(m.gsd)
    L = m.fill(R)   # warm-up of every kernel; allocates the pyramid and the outputs
    torch.cuda.synchronize()
    Hm, Wm = m.Hm, m.Wm
    out = m.result()
    level = out['fill_level']
    measured, filled, empty = int((level == 0).sum()), int((level > 0).sum()), int((level < 0).sum())
    print(f'{torch.cuda.get_device_name(0)}; {len(views)} images of {args.width}x{args.height}; mosaic {Wm} x {Hm} cells of {float(m.gsd):.6g} m: '
          f'{measured} measured, {Hm * Wm - measured} holes')
    print(f'fill of {R:.6g} m ({L} levels, pyramid {m.pyramid.numel()} bytes): {filled} cells filled, {empty} left empty; deepest level {int(level.max())}')

    lib = _lib.load()
    base = (Hm, Wm, L, C.c_void_p(out['J'].data_ptr()), C.c_void_p(out['raw'].data_ptr()), C.c_void_p(out['source'].data_ptr()),
            C.c_void_p(m.pyramid.data_ptr()))
    outs = [C.c_void_p(out[k].data_ptr()) for k in ('J_filled', 'raw_filled', 'fill_level')]
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pull():
        _lib.check(lib.sucre_mosaic_fill_pull(*base, sp))

    def push():
        _lib.check(lib.sucre_mosaic_fill_push(*base, *outs, sp))

    def gather():
        for i in range(0, len(views), 32):
            m.gather(views[i:i + 32], Js[i:i + 32], i)

    nothing = lambda: None   # noqa: E731
    cells = [Hm * Wm]
    h, w = Hm, Wm
    for _ in range(L):
        h, w = (h + 1) >> 1, (w + 1) >> 1
        cells.append(h * w)
    pull_bytes = 19 * cells[0] + 32 * sum(cells[1:]) + 32 * sum(cells[1:L])          # level 0 in; every level out; levels 1..L-1 in again
    push_low = 2 * 19 * cells[0] + 4 * sum(cells[1:L])                                # level 0 in and out; the w words of levels 1..L-1
    push_high = 2 * 19 * cells[0] + 32 * sum(cells[1:]) + 32 * sum(cells[1:L])        # and every level's records whole, as taps and in place
    with torch.cuda.device(dev):
        gather()
        rows = [('pull', (pull_bytes, pull_bytes), timed(nothing, pull, args.reps)), ('push', (push_low, push_high), timed(pull, push, args.reps)),
                ('gather (all images, same run)', None, timed(nothing, gather, args.reps))]
    assert torch.equal(out['fill_level'], level)
    for name, nbytes, (mean, low) in rows:
        moved = ''
        if nbytes:
            a, b = nbytes
            moved = (f'{a / 1e6:9.2f} MB  {a / low / 1e6:7.1f} GB/s at the min' if a == b else
                     f'{a / 1e6:9.2f} to {b / 1e6:.2f} MB  {a / low / 1e6:7.1f} to {b / low / 1e6:.1f} GB/s at the min')
        print(f'{name:32s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {moved}')
    by = {name: mean for name, _, (mean, _) in rows}
    print(f'(pull + push) / gather = {(by["pull"] + by["push"]) / by["gather (all images, same run)"]:.2f}; {2 * L} launches')


if __name__ == '__main__':
    main()
