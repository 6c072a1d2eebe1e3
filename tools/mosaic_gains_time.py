"""Times of the mosaic's per-image gain compensation (sucre_mosaic_gain_span, sucre_mosaic_gain_apply, sucre_mosaic_gain_sums) on the
shape of tools/mosaic_support_time.py: 65 resident images of 1920x1080 from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J
the single-view inversion at the renderer's water times a factor of its own (0.9 .. 1.1, so that there is something to find), the
default frame and ground sample distance, three calls per phase (32 + 32 + 1 images).  In ONE run: the span pass in its default
form -- loads that filter the two atomics -- and with the plain atomics; the apply; the reference accumulate (the blend's accumulate
at inv_h = 2^-126 over the gained images); the sums in the counting form and with one set of atomics per 256 pixels; a whole round
(apply, reference, sums over every batch, and the solve on the host).  And the yardsticks: the splat, the blend's accumulate at
H = 0.5 m and ``sucre_invert_images`` on the same images.  The lines are printed and written to --out.

    python tools/mosaic_gains_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10 --rounds 3]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
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
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--out', type=Path, default=Path(__file__).resolve().parent.parent / 'profiles' / 'mosaic_gains_time.txt')
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
        f'{args.rounds} rounds, limit {engine.MOSAIC_GAIN_LIMIT:g}; factors {min(factors):.3g} .. {max(factors):.3g}')
    chunks = [(i, views[i:i + 32], Js[i:i + 32]) for i in range(0, n, 32)]
    batches = [(i, lambda v=v, J=J: (v, J)) for i, v, J in chunks]

    def over(phase, *a, **kw):
        for i, v, J in chunks:
            phase(v, J, i, *a, **kw)

    rows, nothing = [], lambda: None   # noqa: E731
    m = engine.Mosaic(axes, gsd, dev)
    for _, v, J in chunks:
        m.add_bounds(v, J)
    bounds = m.bounds()
    Hm, Wm = m.begin(bounds, gains=args.rounds)
    over(m.splat)
    over(m.add_span)   # warm-up, and the reference for the plain form
    torch.cuda.synchronize()
    span = m.span.clone()
    lo, hi = span[:, 0].to(torch.int64) & 0xffffffff, span[:, 1].to(torch.int64)
    say(f'{Wm} x {Hm} cells, {int((lo != 0xffffffff).sum())} reached, {int((lo < hi).sum())} shared by two images or more')

    def reset_span():
        m.span[:, 0].fill_(-1)
        m.span[:, 1].zero_()

    rows.append(('span, loads then atomics', timed(reset_span, lambda: over(m.add_span), args.reps)))
    assert torch.equal(m.span, span)
    rows.append(('span, plain atomics', timed(reset_span, lambda: over(m.add_span, plain_atomic=True), args.reps)))
    assert torch.equal(m.span, span)
    rows.append(('span over final words', timed(nothing, lambda: over(m.add_span), args.reps)))

    # the whole chain once, for the figures and as the warm-up of every kernel
    for _ in range(args.rounds):
        m.gain_pass(batches)
        m.solve_gains()
    m.gain_pass(batches)
    torch.cuda.synchronize()
    out = m.result()
    rms = out['gain_rms']
    say('RMS disagreement in shared cells ' + ' '.join(f'{ch} {float(rms[0, c]):.6g} -> {float(rms[-1, c]):.6g}' for c, ch in enumerate('RGB'))
        + f'; {int(out["gain_overlap"].sum())} samples in shared cells; largest |gain x factor / mean - 1| '
        f'{float(((out["gains"].double().cpu() * torch.tensor(factors)[:, None]) / (out["gains"].double().cpu() * torch.tensor(factors)[:, None]).mean(dim=0) - 1).abs().max()):.3g}')

    rows.append(('apply (J x gain into the transient buffer)', timed(nothing, lambda: over(m._apply_gains), args.reps)))
    # one more pass's worth of work on a mosaic of its own, so that the table above stays what the run found
    t = engine.Mosaic(axes, gsd, dev)
    t.begin(bounds, gains=1)
    over(t.splat)
    over(t.add_span)
    t.begin_gain_pass(n)
    t.gain_table.copy_(m.gain_table)
    over(t.add_gain_reference)   # warm-up; acc_gain holds twice the sums from here on, which changes no timing
    rows.append(('apply + reference accumulate (add_gain_reference)', timed(t.acc_gain.zero_, lambda: over(t.add_gain_reference), args.reps)))
    over(t.add_gain_sums)
    torch.cuda.synchronize()
    sums = t.gain_sums_words[0].clone()
    rows.append(('sums, counting form (10 atomics per 8192 pixels of an image)', timed(t.gain_sums_words[0].zero_, lambda: over(t.add_gain_sums), args.reps)))
    assert torch.equal(t.gain_sums_words[0], sums)
    rows.append(('sums, one set of atomics per 256 pixels', timed(t.gain_sums_words[0].zero_, lambda: over(t.add_gain_sums, plain=True), args.reps)))
    assert torch.equal(t.gain_sums_words[0], sums)
    t.end_gain_pass()

    def one_round():
        t._gain_passes = 0   # the same row of the sums every time
        t.gain_sums_words.zero_()
        t.gain_pass(batches)
        t.solve_gains()

    one_round()
    rows.append(('a whole round (apply, reference, sums, solve on the host)', timed(nothing, one_round, args.reps)))

    Jg = [(J * m.gain_table[k]).contiguous() for k, J in enumerate(Js)]
    gained = [(i, views[i:i + 32], Jg[i:i + 32]) for i in range(0, n, 32)]
    b = engine.Mosaic(axes, gsd, dev)
    b.begin(bounds, blend=0.5)
    for i, v, J in gained:
        b.splat(v, J, i)

    def accumulate():
        for i, v, J in gained:
            b.accumulate(v, J, i)

    accumulate()   # warm-up
    torch.cuda.synchronize()
    rows.append(("the blend's accumulate, H = 0.5 m (yardstick)", timed(b.acc.zero_, accumulate, args.reps)))
    b.inv_h = np.float32(2.0 ** -126)
    accumulate()
    rows.append(('reference accumulate alone (inv_h = 2^-126)', timed(b.acc.zero_, accumulate, args.reps)))
    rows.append(('splat, load then atomic (yardstick)', timed(lambda: b.key.fill_(-1), lambda: over(b.splat), args.reps)))
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
