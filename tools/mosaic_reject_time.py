"""Times of the mosaic's colour consensus across views (sucre_mosaic_reject_claim, sucre_mosaic_reject_sums,
sucre_mosaic_reject_consensus, sucre_mosaic_reject_cull; csrc/reject.h) on the shape of tools/mosaic_gains_time.py: 65 resident
images of 1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the renderer's water
times a factor of its own (0.9 .. 1.1), the default frame and ground sample distance, three calls per phase (32 + 32 + 1 images).  In
ONE run: the claim behind its load, with every sample walking the whole chain, and over words that are final already; the sums with
the run sums of a wave's lanes and with every sample for itself; the consensus; the cull with and without its counts; and the
yardsticks: the splat, sucre_mosaic_gain_span, sucre_mosaic_gain_slots and sucre_mosaic_cull.  The expectations were set before any
run (the issue of this feature): the claim behind its loads near the span, the sums near gain_slots, the cull near
sucre_mosaic_cull -- "near": within a factor of 1.5 either way.  The lines are printed and written to --out.

    python tools/mosaic_reject_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --tol 0.05]
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sucre_amd import _lib, engine, sucre, synth  # noqa: E402
from mosaic_time import timed  # noqa: E402

NEAR = 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--grid', type=int, nargs=2, default=(13, 5))
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--tol', type=float, default=0.05, help='the reject tolerance T, units of J')
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--out', type=Path, default=Path(__file__).resolve().parent.parent / 'profiles' / 'mosaic_reject_time.txt')
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = 'cuda:0'
    survey = synth.make_survey(args.width, args.height, args.grid[0], args.grid[1], seed=0, device=dev)
    views = engine.device_views_from_scene(survey, dev)
    water = list(synth.GT_B) + list(synth.GT_BETA) + list(synth.GT_GAMMA)
    n = len(views)
    factors = [0.9 + 0.2 * ((7 * k) % n) / max(1, n - 1) for k in range(n)]
    Js = [(J * torch.tensor(f, dtype=torch.float32, device=dev)).contiguous() for J, f in zip(engine.invert_images(views, water), factors)]
    axes = sucre.mosaic_axes(views)
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views]) * args.gsd_factor
    n_px = sum(v.depth.numel() for v in views)
    say(f'{torch.cuda.get_device_name(0)}; {n} images of {args.width}x{args.height}, {n_px} pixels; gsd {float(gsd):.6g} m; '
        f'reject tolerance {args.tol:g}; factors {min(factors):.3g} .. {max(factors):.3g}')
    chunks = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]

    def over(phase, *a, **kw):
        for i, v, J in chunks:
            phase(v, J, i, *a, **kw)

    rows = []
    m = engine.Mosaic(axes, gsd, dev)
    for _, v, J in chunks:
        m.add_bounds(v, J)
    bounds = m.bounds()
    Hm, Wm = m.begin(bounds, reject=args.tol)
    over(m.add_reject_claim)   # warm-up, and the reference for the other forms
    torch.cuda.synchronize()
    want_ord, want_over = m.reject_slot_ord.clone(), m.reject_slot_over.clone()
    held = (want_ord != -1).sum(dim=1)
    say(f'{Wm} x {Hm} cells, {int((held > 0).sum())} reached, {int((held >= 3).sum())} by 3 images or more, {int(want_over.sum())} by more '
        f'than 8; {float(held[held > 0].double().mean()):.2f} of the 8 slots of a reached cell held on average')

    def reset_claim():
        m.reject_slot_ord.fill_(-1)
        m.reject_slot_over.zero_()

    def same_claim():
        return torch.equal(m.reject_slot_ord, want_ord) and torch.equal(m.reject_slot_over, want_over)

    rows.append(('claim, load then chain, one lane per run', timed(reset_claim, lambda: over(m.add_reject_claim), args.reps)))
    assert same_claim()
    rows.append(('claim, every sample walks the whole chain', timed(reset_claim, lambda: over(m.add_reject_claim, plain_atomic=True), args.reps)))
    assert same_claim()
    rows.append(('claim over words that are final already', timed(lambda: None, lambda: over(m.add_reject_claim), args.reps)))
    assert same_claim()

    over(m.add_reject_sums)
    torch.cuda.synchronize()
    want_sum = m.reject_slot_sum.clone()
    rows.append(('sums, run sums of a wave\'s lanes', timed(m.reject_slot_sum.zero_, lambda: over(m.add_reject_sums), args.reps)))
    assert torch.equal(m.reject_slot_sum, want_sum)
    rows.append(('sums, every sample for itself', timed(m.reject_slot_sum.zero_, lambda: over(m.add_reject_sums, plain=True), args.reps)))
    assert torch.equal(m.reject_slot_sum, want_sum)

    o, big = m._out, torch.zeros(1, dtype=torch.int64, device=dev)

    def consensus():
        _lib.check(_lib.load().sucre_mosaic_reject_consensus(C.byref(m.grid), *(C.c_void_p(x.data_ptr()) for x in (
            m.reject_slot_ord, m.reject_slot_sum, o['reject_ref'], o['reject_source'], o['reject_views'], big)), engine._stream_ptr()))

    consensus()
    rows.append(('consensus, one lane per cell', timed(lambda: None, consensus, args.reps)))
    m.finish_reject()
    assert int(big) == 0
    over(m.rejected_images, count=True)
    torch.cuda.synchronize()
    per = m.reject_counts[:, :2].sum(dim=0).tolist()
    say(f'{int((o["reject_source"] >= 0).sum())} cells with a consensus; {per[1]} of {per[0]} samples in them ({100.0 * per[1] / max(1, per[0]):.1f} %) '
        f'rejected at T = {args.tol:g}, in {int((o["rejected"] > 0).sum())} cells')

    def reset_counts():
        o['rejected'].zero_()
        m.reject_counts.zero_()

    rows.append(('cull, no counts', timed(lambda: None, lambda: over(m.rejected_images), args.reps)))
    rows.append(('cull with its counts (2 atomics per 8192 pixels of an image)', timed(reset_counts, lambda: over(m.rejected_images, count=True), args.reps)))
    assert m.reject_counts[:, :2].sum(dim=0).tolist() == per

    # the yardsticks, on a mosaic of the same grid without the rejection: every phase reads the images themselves
    t = engine.Mosaic(axes, gsd, dev)
    t.begin(bounds, gains=1, gain_solve='direct')
    over(t.splat)
    rows.append(('splat, load then atomic (yardstick)', timed(lambda: t.key.fill_(-1), lambda: over(t.splat), args.reps)))

    def reset_span():
        t.span[:, 0] = -1
        t.span[:, 1] = 0

    over(t.add_span)
    rows.append(('sucre_mosaic_gain_span behind its loads (yardstick)', timed(reset_span, lambda: over(t.add_span), args.reps)))
    t.gain_pass([(i, lambda v=v, J=J: (v, J)) for i, v, J in chunks])
    over(t.add_gain_slots)   # allocates

    def reset_slots():
        t.slot_ord.fill_(-1)
        t.slot_sum.zero_()
        t.slot_over.zero_()

    rows.append(('sucre_mosaic_gain_slots, run sums (yardstick)', timed(reset_slots, lambda: over(t.add_gain_slots), args.reps)))
    s = engine.Mosaic(axes, gsd, dev)
    s.begin(bounds, surface=0.05)
    over(s.add_surface)
    over(s.culled_images)
    rows.append(('sucre_mosaic_cull, no counts (yardstick)', timed(lambda: None, lambda: over(s.culled_images), args.reps)))

    name_of = {name: mean for name, (mean, _) in rows}
    cull = name_of['cull, no counts']
    splat = name_of['splat, load then atomic (yardstick)']
    span = name_of['sucre_mosaic_gain_span behind its loads (yardstick)']
    slots = name_of['sucre_mosaic_gain_slots, run sums (yardstick)']
    for name, (mean, low) in rows:
        say(f'{name:66s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / splat:5.2f} x the splat')
    claim, sums = rows[0][1][0], rows[3][1][0]
    plain_cull = name_of['sucre_mosaic_cull, no counts (yardstick)']

    def verdict(x, y):
        return 'HELD' if 1 / NEAR <= x / y <= NEAR else 'REFUTED'

    say(f'expected: the claim behind its loads near the span -- {claim / span:.2f} x: {verdict(claim, span)}; the sums near gain_slots -- '
        f'{sums / slots:.2f} x: {verdict(sums, slots)}; the cull near sucre_mosaic_cull -- {cull / plain_cull:.2f} x: {verdict(cull, plain_cull)} '
        f'(near: within a factor of {NEAR:g} either way)')
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
