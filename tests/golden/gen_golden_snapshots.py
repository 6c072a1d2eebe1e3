"""Generates tests/golden/snapshots_<fixture>.npz and snapshots_<fixture>_pictures.npz: what the REAL reference holds and
plots at its --save-interval stops.

Run in the dev container only:  python tests/golden/gen_golden_snapshots.py
For the two scenes of ``gen_golden.py`` and the four modes {J as a parameter, closed form} x {plain, light model} the
reference's ``sucre.adam(model, md, num_iter=9, batch_size=5, save_dir=tmp, save_interval=4)`` is run with ``save_plots``
wrapped to record (``ref_harness.reference_fit``): it stops after iterations 0, 4 and 8 (sucre.py:153-154).  Per mode
``<mode>`` in param / closed / light / light_closed and stop ``k`` the first file holds

    <mode>_stop<k>_J, <mode>_stop<k>_params       the J and the parameters (9, or 19 with the light model) held at the stop
    <mode>_files                                  the names of all files the run wrote, sorted
    <mode>_J_final, <mode>_params_final, <mode>_trace   what sucre.adam returned, and the per-iteration trace
    <mode>_stop<k>_rms_to_next                    closed form: per-channel RMS distance between the stop's J(theta_k) and the
                                                  J(theta_{k+1}) the reference solved one iteration later -- how far an
                                                  off-by-one is from the held state

plus ``stops``, ``num_iter`` and ``save_interval``, and the second one

    <mode>_stop<k>_rgb, _reconstruction, _vignetting   the 8-bit arrays of the PNGs written there (vignetting: light model)

(two files: float32 images hardly compress, and together they would pass the size a committed file may have).  With J as a
parameter the last iteration of these runs is a stop and nothing follows it, so ``<mode>_J_final`` would repeat
``<mode>_stop8_J``: it is checked to and left out (``helpers.Snapshots`` hands the stop's J out for it).  Outputs only: the
inputs are those of ``<fixture>.npz``.  No reference source is stored.  Generated with torch 2.10.0 CPU, 8 threads.
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import helpers  # noqa: E402
import ref_harness as rh  # noqa: E402
from gen_golden import FIXTURES, quiet  # noqa: E402

NUM_ITER, SAVE_INTERVAL = 9, 4
MODES = {'param': (False, False), 'closed': (True, False), 'light': (False, True), 'light_closed': (True, True)}


def generate(name):
    scene = helpers.Fixture(name).scene   # the stored inputs themselves, not a scene rendered again on this host
    _, md, target = rh.reference_matches(scene, min_cover=1e-6)
    stem = Path(target.name).stem
    out = dict(num_iter=NUM_ITER, save_interval=SAVE_INTERVAL)
    pictures = {}
    for mode, (closed, light) in MODES.items():
        with tempfile.TemporaryDirectory() as tmp:
            fit = quiet(rh.reference_fit, scene, md, target, num_iter=NUM_ITER, use_closed_form=closed, light_model=light,
                        batch_size=5, save_dir=Path(tmp), save_interval=SAVE_INTERVAL, snapshots=range(1, NUM_ITER + 1))
            out[f'{mode}_files'] = np.array(sorted(f.name for f in Path(tmp).iterdir()))
        out.setdefault('stops', np.array(sorted(fit['stops']), np.int64))
        assert sorted(fit['stops']) == out['stops'].tolist()
        for k, stop in fit['stops'].items():
            out[f'{mode}_stop{k}_J'] = stop['J']
            out[f'{mode}_stop{k}_params'] = stop['params']
            assert np.array_equal(stop['J'], fit['snaps'][k + 1], equal_nan=True)
            if closed:   # the J held during iteration k+1 is J(theta_{k+1}); behind the last iteration it is the returned one
                later = fit['snaps'][k + 2] if k + 2 <= NUM_ITER else fit['J']
                out[f'{mode}_stop{k}_rms_to_next'] = helpers.rms_per_channel(stop['J'], later)
            assert np.array_equal(stop['params'], fit['trace'][k, 1:].astype(np.float32))   # theta_{k+1}
            kinds = {n[len(stem) + 1:-len(f'_{k:04d}.png')]: a for n, a in stop['files'].items()}
            assert sorted(kinds) == ['reconstruction', 'rgb'] + (['vignetting'] if light else []), sorted(stop['files'])
            for kind, a in kinds.items():
                pictures[f'{mode}_stop{k}_{kind}'] = a
        if closed:
            out[f'{mode}_J_final'] = fit['J']
        else:
            assert np.array_equal(fit['J'], fit['stops'][NUM_ITER - 1]['J'], equal_nan=True)
        out[f'{mode}_params_final'] = fit['params']
        out[f'{mode}_trace'] = fit['trace']
    path, ppath = HERE / f'snapshots_{name}.npz', HERE / f'snapshots_{name}_pictures.npz'
    np.savez_compressed(path, **out)
    np.savez_compressed(ppath, **pictures)
    print(name, 'stops', out['stops'].tolist(), 'files per mode', [len(out[f'{m}_files']) for m in MODES],
          'sizes', path.stat().st_size, ppath.stat().st_size)


if __name__ == '__main__':
    torch.set_num_threads(8)
    for name in FIXTURES:
        generate(name)
