"""GPU tests of the state the engine holds in the MIDDLE of a fit: SUCRE_FIT_KEEP_J, fits split into several calls, and the
--save-interval snapshots of ``sucre.adam`` and the CLI, against what the reference held and plotted at its own stops
(tests/golden/snapshots_*.npz, gen_golden_snapshots.py: num_iter=9, save_interval=4 -> stops after iterations 0, 4, 8).

At stop k the reference holds theta_{k+1} next to J(theta_k) in closed form (sucre.py:141 solves J before the step of
iteration k, sucre.py:153 plots after it).  The CPU tier pins that reading to the oracle (tests/test_oracle_golden.py) and the
pictures to the host output stage (tests/test_host_logic.py); here the engine is held to both.  Bars are those of the
closed-form tests of tests/test_gpu_parity.py; an off-by-one in either direction is >= 9.5 x the J bar away (asserted from
the fixture in the tests that rely on it).
"""
import copy
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image as PILImage

import helpers
from oracle import oracle

pytestmark = pytest.mark.gpu

RMS_BAR = 1e-4           # per-channel RMS(J) against the reference (tests/test_gpu_parity.py)
PARAM_BAR = 2e-4          # every parameter against the reference, cam2light / sigma included (test_fit_closed_form_mode)
ORACLE_LIGHT = 1e-3       # cam2light, sigma against the ORACLE only: their gradients sit at Adam's eps scale
                          # (test_light_model_closed_form_vs_oracle)
# closed form against the ORACLE, (RMS(J), B / beta / gamma) per kind of workspace, one source test per line
ORACLE_BARS = {
    'f32': (5e-5, 2e-4),       # the plain closed-form kernel's oracle bars, as in the next line and test_float32_colour_store_vs_oracle
    'u16mm': (5e-5, 2e-4),     # test_compact_u16mm_store_vs_oracle_and_golden (oracle fed the quantised ranges)
    'light': (RMS_BAR, 5e-5),  # test_light_model_closed_form_vs_oracle
}
ORACLE_J = {kind: bars[0] for kind, bars in ORACLE_BARS.items()}
ORACLE_WATER = {kind: bars[1] for kind, bars in ORACLE_BARS.items()}
PICTURE_SHARE = 1e-2      # of the 8-bit values of a snapshot picture may differ from the reference's (~30 x what a restatement of
                          # the reference needs, ~19 x below the mildest wrong state: 19 % of a vignetting picture)


def _workspace(scene, kind):
    """A matched workspace of the scene's target: 'f32', 'u16mm' (plain stores), 'light' (light model) or 'fcolour' (float32
    colours, the --image-scale store)."""
    from sucre_amd import engine
    views = engine.device_views_from_scene(scene, 'cuda')
    if kind == 'fcolour':
        views = [v.as_float_colour() for v in views]
    r = engine.Restoration(scene.height, scene.width, len(views), light=kind == 'light',
                           obs_format='u16mm' if kind == 'u16mm' else 'f32', float_colour=kind == 'fcolour')
    r.match(views[scene.target], views)
    return r, views[scene.target]


def _state(r):
    return r.J().cpu().numpy(), r.params().cpu().numpy().copy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


_SAMPLES = {}       # fixture name -> the oracle's samples of its scene
_ORACLE_FITS = {}   # (fixture name, kind, num_iter) -> the oracle's closed-form fit


def _oracle_fit(golden, kind, num_iter):
    """The oracle's closed-form run of ``num_iter`` iterations on the fixture's scene (computed once per session)."""
    key = (golden.name, kind, num_iter)
    if key not in _ORACLE_FITS:
        sc = golden.scene
        if golden.name not in _SAMPLES:
            _SAMPLES[golden.name] = helpers.oracle_scene_samples(sc)[1]
        samples = _SAMPLES[golden.name]
        if kind == 'u16mm':
            samples = oracle.quantize_ranges_u16mm(samples)
        fit = oracle.fit_light if kind == 'light' else oracle.fit
        _ORACLE_FITS[key] = fit(sc.height, sc.width, samples, None, num_iter=num_iter, use_closed_form=True)
    return _ORACLE_FITS[key]


def _check_params(p, ref, water_bar, label, light_bar=None):
    """B / beta / gamma within ``water_bar`` of ``ref``; cam2light / sigma within ``light_bar`` (default: the same bar)."""
    dwater = float(np.abs(p[:9] - ref[:9]).max())
    dlight = float(np.abs(p[9:] - ref[9:]).max()) if len(ref) > 9 else 0.0
    assert len(p) == len(ref) and dwater < water_bar and dlight < (water_bar if light_bar is None else light_bar), (label, dwater, dlight)
    return dwater, dlight


# ---- a. keep_J against the reference's held state ---------------------------------------------------------------------------

@pytest.mark.parametrize('T', [1, 5, 9])
@pytest.mark.parametrize('kind', ['f32', 'u16mm', 'light'])
def test_keep_J_holds_the_state_the_reference_plots(golden, kind, T):
    """``fit(T, use_closed_form=True, keep_J=True)`` must leave J(theta_{T-1}) next to theta_T: the reference's state at its stop
    k = T - 1.  Against the fixture: RMS(J) < RMS_BAR per channel, every parameter -- cam2light / sigma included -- within 2e-4
    (test_fit_closed_form_mode); the millimetre ranges of a u16mm store move J by <= 3.7e-5 RMS and the parameters by <= 2.3e-5
    at these stops (measured with the CPU oracle: quantised against unquantised ranges), so that store is held to the same
    bars and, like test_compact_u16mm_store_vs_oracle_and_golden, to the oracle fed the quantised ranges (5e-5, 2e-4).
    Against the oracle pair (fit(k).J, fit(k+1).params): the closed-form oracle bars of tests/test_gpu_parity.py (cam2light /
    sigma 1e-3 there, against the oracle only).  The same call WITHOUT keep_J must hold J(theta_T): the oracle's fit(T).
    Guard: the reference's own J one iteration later is more than 5 x the bar away in every channel (fixture: >= 9.5 x).
    The test prints the engine's distances to the reference and to the oracle pair for every case."""
    mode = 'light_closed' if kind == 'light' else 'closed'
    snaps = helpers.load_snapshots(golden.name)
    k = T - 1
    assert k in snaps.stops
    assert snaps.rms_to_next(mode, k).min() > 5 * RMS_BAR, (mode, k, snaps.rms_to_next(mode, k))
    r, target = _workspace(golden.scene, kind)
    r.fit_init(target)
    trace = r.fit(T, use_closed_form=True, keep_J=True).cpu().numpy()
    J, p = _state(r)
    label = f'{golden.name} {kind} keep_J T={T}'
    ref_J, ref_p = snaps.J(mode, k), snaps.params(mode, k)
    assert np.array_equal(np.isnan(J), np.isnan(ref_J)), label
    rms = helpers.rms_per_channel(J, ref_J)
    dwater, dlight = float(np.abs(p[:9] - ref_p[:9]).max()), float(np.abs(p[9:] - ref_p[9:]).max()) if kind == 'light' else 0.0
    print(f'{label}: engine vs the REFERENCE at stop {k}: rms(J) {rms} water {dwater:.1e} light {dlight:.1e}')
    assert rms.max() < RMS_BAR, (label, rms)
    _check_params(p, ref_p, PARAM_BAR, label)
    assert np.array_equal(p, trace[-1, 1:1 + len(p)].astype(np.float32)), label            # theta_T is the trace's last row
    # the oracle pair
    Jo = _oracle_fit(golden, kind, k)[0]
    po = _oracle_fit(golden, kind, T)[1]
    rms_o = helpers.rms_per_channel(J, Jo)
    print(f'{label}: engine vs the oracle pair: rms(J) {rms_o} parameters {np.abs(p - po).max():.1e}')
    assert np.array_equal(np.isnan(J), np.isnan(Jo)) and rms_o.max() < ORACLE_J[kind], (label, rms_o)
    _check_params(p, po, ORACLE_WATER[kind], label + ' vs oracle', light_bar=ORACLE_LIGHT)
    # without keep_J: J(theta_T), same parameters
    r.fit_init(target)
    r.fit(T, use_closed_form=True)
    J2, p2 = _state(r)
    assert np.array_equal(p2, p), label
    JT = _oracle_fit(golden, kind, T)[0]
    assert np.array_equal(np.isnan(J2), np.isnan(JT)) and helpers.rms_per_channel(J2, JT).max() < ORACLE_J[kind], label
    if k == snaps.num_iter - 1:   # ... which at the end of the reference's run is what it returned
        assert helpers.rms_per_channel(J2, snaps.final(mode)[0]).max() < RMS_BAR, label


# ---- b. split with keep_J is the unsplit run, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize('kind,closed', [('f32', True), ('u16mm', True), ('light', True), ('fcolour', True), ('light', False)],
                         ids=['closed-f32', 'closed-u16mm', 'closed-light', 'closed-fcolour', 'param-light'])
def test_split_fit_that_keeps_J_is_the_unsplit_fit_bit_for_bit(golden, kind, closed):
    """``fit(1) + fit(4) + fit(4)`` with keep_J, then one ``update_J()`` -- the calls ``sucre.adam`` makes for --save-interval 4
    --num-iter 9 -- against ``fit(9)``: J (NaN mask included), parameters and the concatenated traces, bit for bit.  The two
    launch sequences are the same by construction (the initial update_J only happens at t0 == 0, the J planes are the only
    state carried between calls), so there is no tolerance.  With J as a parameter (light model; the plain case is
    test_fit_is_bitwise_reproducible_and_resumable) keep_J means nothing and no update_J follows."""
    r, target = _workspace(golden.scene, kind)
    r.fit_init(target)
    whole = r.fit(9, use_closed_form=closed).cpu().numpy()
    J, p = _state(r)
    r.fit_init(target)
    parts = [r.fit(n, use_closed_form=closed, keep_J=True) for n in (1, 4, 4)]
    if closed:
        r.update_J()
    Js, ps = _state(r)
    assert r.steps_done == 9
    assert _same_bits(torch.cat(parts).cpu().numpy(), whole), 'traces differ'
    assert _same_bits(ps, p), ('parameters differ', ps, p)
    assert np.array_equal(np.isnan(Js), np.isnan(J)), 'NaN masks differ'
    assert _same_bits(Js, J), ('J differs', helpers.rms_per_channel(Js, J))


# ---- c. split without keep_J ------------------------------------------------------------------------------------------------

def test_split_light_closed_form_fit_without_keep_J_is_the_unsplit_fit_bit_for_bit(golden):
    """Light model, closed form: J is re-solved from zero every iteration, so the update_J a call appends changes nothing the
    next call reads: ``fit(4) + fit(5)`` is ``fit(9)`` bit for bit."""
    r, target = _workspace(golden.scene, 'light')
    r.fit_init(target)
    whole = r.fit(9, use_closed_form=True).cpu().numpy()
    J, p = _state(r)
    r.fit_init(target)
    parts = [r.fit(n, use_closed_form=True) for n in (4, 5)]
    Js, ps = _state(r)
    assert _same_bits(torch.cat(parts).cpu().numpy(), whole) and _same_bits(ps, p) and _same_bits(Js, J)


def test_split_plain_closed_form_fit_without_keep_J_stays_on_the_reference(golden):
    """Plain one-pass kernel: it measures from the J the previous launch left, so after ``fit(4)`` (whose appended update_J
    leaves J(theta_4)) iteration 4 measures from J(theta_4) instead of J(theta_3): the same sums, formed relative to another J,
    i.e. other roundings.  The split run is therefore held to the REFERENCE's trace and returned J at the bars of the unsplit
    run (RMS_BAR, 2e-4, cost 1e-4: test_fit_closed_form_mode), not to the unsplit run's bits; the distance between the two is
    printed."""
    snaps = helpers.load_snapshots(golden.name)
    r, target = _workspace(golden.scene, 'f32')
    r.fit_init(target)
    whole = r.fit(9, use_closed_form=True).cpu().numpy()
    J, p = _state(r)
    r.fit_init(target)
    trace = torch.cat([r.fit(n, use_closed_form=True) for n in (4, 5)]).cpu().numpy()
    Js, ps = _state(r)
    ok = ~np.isnan(J)
    print(f'{golden.name}: closed form, fit(4) + fit(5) vs fit(9): rms(J) {helpers.rms_per_channel(Js, J)}, '
          f'{float((Js[ok] != J[ok]).mean()):.1e} of the values differ, parameters {np.abs(ps - p).max():.1e}, '
          f'trace {np.abs(trace - whole).max():.1e}')
    ref_J, ref_p = snaps.final('closed')
    rt = snaps.trace('closed')
    assert np.array_equal(np.isnan(Js), np.isnan(ref_J))
    assert helpers.rms_per_channel(Js, ref_J).max() < RMS_BAR
    assert np.abs(trace[:, 1:] - rt[:, 1:]).max() < PARAM_BAR and np.abs(trace[:, 0] / rt[:, 0] - 1).max() < 1e-4
    _check_params(ps, ref_p, PARAM_BAR, 'split run')


# ---- d. batch launch --------------------------------------------------------------------------------------------------------

def test_fit_batch_with_keep_J_is_fit_with_keep_J_per_image(golden):
    """``engine.fit_batch(..., use_closed_form=True, keep_J=True)`` on three images of one size (three targets of the scene),
    split 1 + 4 + 4 as ``sucre.adam`` would: after every call every image holds, bit for bit, what ``fit(..., keep_J=True)`` gives
    it alone -- and the first image, the fixture's target, the reference's state of that stop."""
    from sucre_amd import engine
    sc = golden.scene
    snaps = helpers.load_snapshots(golden.name)
    n = len(sc.views)
    targets = [sc.target, sc.target - 1, (sc.target + 1) % n]
    assert len(set(targets)) == 3 and min(targets) >= 0
    rs = []
    for t in targets:
        s = copy.copy(sc)
        s.target = t
        rs.append(_workspace(s, 'f32'))
    alone = []
    for r, target in rs:
        r.fit_init(target)
        states = []
        for steps in (1, 4, 4):
            tr = r.fit(steps, use_closed_form=True, keep_J=True)
            states.append(_state(r) + (tr.cpu().numpy(),))
        alone.append(states)
    for r, target in rs:
        r.fit_init(target)
    done = 0
    for call, steps in enumerate((1, 4, 4)):
        traces = engine.fit_batch([r for r, _ in rs], steps, use_closed_form=True, keep_J=True)
        done += steps
        for i, ((r, _), tr) in enumerate(zip(rs, traces)):
            J, p = _state(r)
            Ja, pa, tra = alone[i][call]
            assert _same_bits(tr.cpu().numpy(), tra) and _same_bits(p, pa) and _same_bits(J, Ja), (call, i, helpers.rms_per_channel(J, Ja))
        J0, p0 = _state(rs[0][0])
        assert snaps.rms_to_next('closed', done - 1).min() > 5 * RMS_BAR
        assert helpers.rms_per_channel(J0, snaps.J('closed', done - 1)).max() < RMS_BAR, call
        _check_params(p0, snaps.params('closed', done - 1), PARAM_BAR, f'batch, call {call}')


# ---- e. sucre.adam with save_dir / save_interval ---------------------------------------------------------------------------------

def _adam_run(scene, mode, tmp, num_iter, save_interval, tag):
    """The reference-style call sequence on the GPU (restore_image's own statements, sucre.py:187-210, without files behind the
    images): match_images, prepare / check / load_matches, SUCRe(...).to('cuda'), adam.  Returns (model, output folder)."""
    from sucre_amd import loader, sucre
    closed, light = helpers.SNAPSHOT_MODES[mode]
    images = [helpers.synth_image(i + 1, v, scene.K, scene.width, scene.height) for i, v in enumerate(scene.views)]
    target = images[scene.target]
    out = Path(tmp) / f'{mode}_{tag}'
    out.mkdir()
    matches_file = loader.MatchesFile(out / 'm.h5', colmap_model=None)
    target.match_images(image_list=images, matches_file=matches_file, device='cuda', light_model=light)
    matches_file.prepare_matches()
    matches_file.check_integrity()
    md = matches_file.load_matches()
    model = sucre.SUCRe(image=target, light_model=light, use_closed_form=closed).to('cuda')
    sucre.adam(sucre=model, matches_data=md, lr=0.05, num_iter=num_iter, batch_size=5,
               save_dir=out if save_interval is not None else None, save_interval=save_interval, device='cuda')
    return model, out


def _model_state(model):
    return model.J.detach().cpu().numpy(), model.water_vector().cpu().numpy()


@pytest.mark.parametrize('mode', list(helpers.SNAPSHOT_MODES))
def test_adam_snapshots_are_the_reference_pictures(golden, tmp_path, mode):
    """``sucre.adam(num_iter=9, save_dir=..., save_interval=4)`` in all four modes against the reference's own run: the files
    written carry exactly the reference's names (``_vignetting_*`` only with the light model); every snapshot PNG differs from
    the reference's at no more than 1e-2 of its values -- by at most one level for ``rgb`` and ``reconstruction``, no level bound
    for ``vignetting`` (the jet table is not smooth per channel) -- where a J one iteration late moves 39-95 % of the rgb values
    and parameters one iteration early 19-40 % of the vignetting values; the returned J and parameters meet the reference's at
    the bars of test_keep_J_holds_the_state_the_reference_plots (RMS_BAR, every parameter 2e-4; J as a parameter without the
    light model: 1e-4 as test_fit_J_parameter_mode); and the returned state is, bit
    for bit, that of ``sucre.adam`` without ``save_dir`` -- for num_iter=9, whose last iteration is a snapshot (the final
    update_J is held back for it), and for num_iter=10, whose last is not.
    The test prints the share of differing values and the largest step of every picture."""
    closed, light = helpers.SNAPSHOT_MODES[mode]
    sc = golden.scene
    snaps = helpers.load_snapshots(golden.name)
    model, out = _adam_run(sc, mode, tmp_path, snaps.num_iter, snaps.save_interval, 'snap')
    assert sorted(f.name for f in out.iterdir() if f.suffix == '.png') == snaps.files(mode)
    stem = Path(sc.views[sc.target].name).stem
    for k in snaps.stops:
        for kind in ('rgb', 'reconstruction') + (('vignetting',) if light else ()):
            got = np.asarray(PILImage.open(out / f'{stem}_{kind}_{k:04d}.png'))
            share, step = helpers.picture_distance(got, snaps.picture(mode, k, kind))
            print(f'{golden.name} {mode} stop {k} {kind}: {share:.1e} of the values differ, by at most {step}')
            assert share <= PICTURE_SHARE, (mode, k, kind, share, step)
            assert kind == 'vignetting' or step <= 1, (mode, k, kind, share, step)
    J, p = _model_state(model)
    ref_J, ref_p = snaps.final(mode)
    assert np.array_equal(np.isnan(J), np.isnan(ref_J))
    rms = helpers.rms_per_channel(J, ref_J)
    print(f'{golden.name} {mode}: returned state vs the REFERENCE: rms(J) {rms} parameters {np.abs(p - ref_p).max():.1e}')
    assert rms.max() < RMS_BAR, (mode, rms)
    _check_params(p, ref_p, PARAM_BAR if closed or light else 1e-4, mode)
    for num_iter in (snaps.num_iter, snaps.num_iter + 1):
        if num_iter != snaps.num_iter:
            model, _ = _adam_run(sc, mode, tmp_path, num_iter, snaps.save_interval, f'snap{num_iter}')
            J, p = _model_state(model)
        plain, _ = _adam_run(sc, mode, tmp_path, num_iter, None, f'plain{num_iter}')
        Jp, pp = _model_state(plain)
        assert _same_bits(p, pp) and _same_bits(J, Jp), (mode, num_iter, helpers.rms_per_channel(J, Jp), np.abs(p - pp).max())
