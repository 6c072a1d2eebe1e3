"""Times of the direct solve of the mosaic's gain compensation (sucre_mosaic_gain_slots, sucre_mosaic_gain_pairs,
sucre_mosaic_gain_diag, engine.mosaic_gain_solve_direct) on the shape of tools/mosaic_gains_time.py: 65 resident images of 1920x1080
from ``synth.make_survey`` (13 x 5 cameras, seed 0), every J the single-view inversion at the renderer's water times a factor of its
own (0.9 .. 1.1), the default frame and ground sample distance, three calls per phase (32 + 32 + 1 images).  In ONE run: the slots
with the run sums of a wave's lanes and with every sample for itself; the pairs with the LDS table and with global atomics per cell
and pair; the diag in the counting form and with one set of atomics per 256 pixels; the solve on the host; the whole direct phase
(slots, pairs, diag over every batch, and the solve); and the yardsticks: one whole round of the relaxation, the splat and the
blend's accumulate at H = 0.5 m.  The lines are printed and written to --out.

    python tools/mosaic_gain_direct_time.py [--width 1920 --height 1080 --grid 13 5 --reps 10]
"""
import argparse
import sys
import time
from pathlib import Path

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
    ap.add_argument('--gsd-factor', type=float, default=1.0, help='multiple of the default ground sample distance')
    ap.add_argument('--out', type=Path, default=Path(__file__).resolve().parent.parent / 'profiles' / 'mosaic_gain_direct_time.txt')
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
        f'limit {engine.MOSAIC_GAIN_LIMIT:g}; factors {min(factors):.3g} .. {max(factors):.3g}')
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
    Hm, Wm = m.begin(bounds, gains=1, gain_solve='direct')
    over(m.splat)
    over(m.add_span)
    m.gain_pass(batches)
    over(m.add_gain_slots)   # warm-up, allocates, and the reference for the other forms
    torch.cuda.synchronize()
    span = m.span.cpu().numpy().view('uint32')
    over_cells = int(((span[:, 0] < span[:, 1]) & (m.slot_over.cpu().numpy() != 0)).sum())
    held = (m.slot_ord != -1).sum(dim=1)
    say(f'{Wm} x {Hm} cells, {int((span[:, 0] < span[:, 1]).sum())} shared, {over_cells} of them hold more than 8 images; '
        f'{float(held[held > 0].double().mean()):.2f} of the 8 slots of a shared cell held on average')

    def sorted_slots():
        order = torch.argsort(m.slot_ord.to(torch.int64) & 0xffffffff, dim=1, stable=True)
        return torch.gather(m.slot_ord, 1, order), torch.gather(m.slot_sum, 1, order[:, :, None].expand(-1, -1, 4)), m.slot_over.clone()

    want = sorted_slots()
    ok = want[2] == 0

    def reset_slots():
        m.slot_ord.fill_(-1)
        m.slot_sum.zero_()
        m.slot_over.zero_()

    def same_slots():
        got = sorted_slots()
        return torch.equal(got[2], want[2]) and torch.equal(got[0][ok], want[0][ok]) and torch.equal(got[1][ok], want[1][ok])

    rows.append(('slots, run sums of a wave\'s lanes', timed(reset_slots, lambda: over(m.add_gain_slots), args.reps)))
    assert same_slots()
    rows.append(('slots, every sample for itself', timed(reset_slots, lambda: over(m.add_gain_slots, plain=True), args.reps)))
    assert same_slots()

    def pairs(**kw):
        m._paired = False
        m.gain_pairs(**kw)

    pairs()
    torch.cuda.synchronize()
    words = m.gain_pairs_words.clone()
    say(f'{int((words[:, :, 3] > 0).sum()) - int((words[:, :, 3].diagonal() > 0).sum())} overlapping pairs among {n} images')
    rows.append(('pairs, LDS table of 512 entries per 4096 cells', timed(m.gain_pairs_words.zero_, pairs, args.reps)))
    assert torch.equal(m.gain_pairs_words, words)
    rows.append(('pairs, global atomics per cell and pair', timed(m.gain_pairs_words.zero_, lambda: pairs(plain=True), args.reps)))
    assert torch.equal(m.gain_pairs_words, words)
    over(m.add_gain_diag)
    torch.cuda.synchronize()
    diag = m.gain_diag_words.clone()
    rows.append(('diag, counting form (4 atomics per 8192 pixels of an image)', timed(m.gain_diag_words.zero_, lambda: over(m.add_gain_diag), args.reps)))
    assert torch.equal(m.gain_diag_words, diag)
    rows.append(('diag, one set of atomics per 256 pixels', timed(m.gain_diag_words.zero_, lambda: over(m.add_gain_diag, plain=True), args.reps)))
    assert torch.equal(m.gain_diag_words, diag)

    host_pairs, host_diag, ones = words.cpu().numpy(), m.gain_diag().cpu().numpy(), torch.ones(n, 3).numpy()
    for _ in range(2):   # warm-up: the first LAPACK call loads and sizes its library
        engine.mosaic_gain_solve_direct(host_pairs, host_diag, ones, m.gain_limit)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        engine.mosaic_gain_solve_direct(host_pairs, host_diag, ones, m.gain_limit)
    say(f'{"the solve on the host (three n x n systems, numpy.linalg.solve)":66s} {(time.perf_counter() - t0) / args.reps * 1e3:8.3f} ms mean  '
        f'over {args.reps} repetitions after 2 warm-up calls (host clock: no device work, the copies to the host not included)')

    def direct_phase():
        reset_slots()
        m.gain_pairs_words.zero_()
        m.gain_diag_words.zero_()
        m._paired = False
        m.gain_table.fill_(1.0)
        over(m.add_gain_slots)
        m.gain_pairs()
        over(m.add_gain_diag)
        m.solve_gains_direct()

    direct_phase()
    rows.append(('the whole direct phase (resets, slots, pairs, diag, solve)', timed(nothing, direct_phase, args.reps)))
    m.gain_pass(batches)
    torch.cuda.synchronize()
    rms = m.result()['gain_rms']
    say('RMS disagreement in shared cells ' + ' '.join(f'{ch} {float(rms[0, c]):.6g} -> {float(rms[-1, c]):.6g}' for c, ch in enumerate('RGB'))
        + ' after the one direct solve')

    t = engine.Mosaic(axes, gsd, dev)
    t.begin(bounds, gains=1)
    over(t.splat)
    over(t.add_span)

    def one_round():
        t._gain_passes = 0   # the same row of the sums every time
        t.gain_sums_words.zero_() if t.gain_sums_words is not None else None
        t.gain_pass(batches)
        t.solve_gains()

    one_round()
    rows.append(('a whole round of the relaxation (yardstick)', timed(nothing, one_round, args.reps)))
    b = engine.Mosaic(axes, gsd, dev)
    b.begin(bounds, blend=0.5)
    over(b.splat)
    over(b.accumulate)   # warm-up
    torch.cuda.synchronize()
    rows.append(("the blend's accumulate, H = 0.5 m (yardstick)", timed(b.acc.zero_, lambda: over(b.accumulate), args.reps)))
    rows.append(('splat, load then atomic (yardstick)', timed(lambda: b.key.fill_(-1), lambda: over(b.splat), args.reps)))
    whole, acc, splat = rows[-3][1][0], rows[-2][1][0], rows[-1][1][0]
    for name, (mean, low) in rows:
        say(f'{name:66s} {mean:8.3f} ms mean  {low:8.3f} ms min  over {args.reps} repetitions   {mean / splat:5.2f} x the splat   '
            f'{mean / acc:5.2f} x the accumulate   {mean / whole:5.2f} x a round')
    slots, phase = rows[0][1][0], rows[6][1][0]
    say(f'expected: the slots about half an accumulate -- {slots / acc:.2f} x: {"held" if slots <= 0.6 * acc else "REFUTED"}; the whole '
        f'direct phase below one round -- {phase / whole:.2f} x: {"held" if phase < whole else "REFUTED"}')
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
