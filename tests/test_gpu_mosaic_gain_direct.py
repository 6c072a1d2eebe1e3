"""GPU tests of the direct solve of the mosaic's gain compensation (sucre_mosaic_gain_slots / _pairs / _diag, engine.Mosaic,
sucre.mosaic, --mosaic-gain-solve).

The yardstick is tests/mosaic_gain_direct_ref.py, a numpy restatement that shares no code with the engine;
test_mosaic_gain_direct_host.py checks it against plain loops over the definition.  The device state is integer and order-free, so
every comparison of it is EXACT: a cell's slots (sorted by ordinal: which slot an image holds depends on arrival), the overflow flag,
the pair words, the diag.  The solved gains are LAPACK's on both sides, on bit-equal integers: the bar is 2^-20 relative -- anything
larger is a different system, not a different rounding.  The later stages need no new restatement: a run with the flag must equal a
run without gains on the images times their gains.
"""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import mosaic_gain_direct_crafted as chain
import mosaic_gain_direct_ref as dref
from test_gpu_mosaic_gains import FACTORS, GAIN_KEYS, scene_case
from test_gpu_mosaic_surface import same_bits
from sucre_amd import engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DIRECT_KEYS = ('gain_solve', 'gain_direct', 'gain_pair_index', 'gain_pair_words', 'gain_diag', 'gain_excluded_cells', 'gain_shared_cells',
               'gain_kept', 'gain_components', 'gain_prior')
_CACHE = {}


def on_device(hv, hJ):
    views = [engine.DeviceView(depth=v.depth.to(DEV), rgb=v.rgb.to(DEV), K=v.K, R=v.R, t=v.t, name=f'v{i:02d}') for i, v in enumerate(hv)]
    return views, [J.to(DEV) for J in hJ]


def case(key):
    """(views, Js, axes, gsd, the restatement's gains with R = 1) of the chain, the deep scene, or a fan -- made once, never changed."""
    if key not in _CACHE:
        if key == 'deep':
            views, Js, axes, gsd, hv, hJ = scene_case('deep')
        else:
            hv, hJ = chain.survey() if key == 'chain' else chain.fan(*key)
            views, Js = on_device(hv, hJ)
            axes = torch.eye(3)
            gsd = sucre.mosaic_default_gsd([v.depth for v in views], [100.0] * len(views)) if key == 'chain' else 0.04
        _CACHE[key] = (views, Js, axes, gsd, dref.gains(hv, hJ, axes, gsd, 1, chain.LIMIT))
    return _CACHE[key]


def state_by_hand(views, Js, axes, gsd, splits=(), reverse=False, plain=(False, False, False), table=0):
    """begin, splat, span, the first pass, then the slots, the pairs and the diag by the methods -- every phase over the batches cut
    at ``splits`` (in reversed order with ``reverse``), each of the three kernels in its plain form where ``plain`` says so."""
    cuts = [0, *splits, len(views)]
    batches = [(a, lambda a=a, b=b: (views[a:b], Js[a:b])) for a, b in zip(cuts, cuts[1:])]
    if reverse:
        batches = batches[::-1]
    m = engine.Mosaic(axes, gsd, DEV)
    m.add_bounds(views, Js)
    m.begin(gains=1, gain_limit=chain.LIMIT, gain_solve='direct')
    assert m.slot_ord is None and m.gain_pairs_words is None            # allocated only when the slots are asked for
    for first, load in batches:
        m.splat(*load(), first)
    for first, load in batches:
        m.add_span(*load(), first)
    m.gain_pass(batches)
    for first, load in batches:
        m.add_gain_slots(*load(), first, plain=plain[0])
    m.gain_pairs(plain=plain[1], table_entries=table)
    for first, load in batches:
        m.add_gain_diag(*load(), first, plain=plain[2])
    return m


def check_state(m, want, what):
    """``slot_over``, every cell's slots sorted by ordinal, ``pairs`` and ``diag`` of ``m`` against the restatement's, bit for bit."""
    assert (m.Hm, m.Wm) == (want['Hm'], want['Wm']), what
    assert np.array_equal(m.span.cpu().numpy().view(np.uint32), want['span']), (what, 'span')
    over = m.slot_over.cpu().numpy()
    assert m.slot_over.dtype == torch.int32 and np.array_equal(over != 0, want['over']) and set(np.unique(over)) <= {0, 1}, (what, 'over')
    ords = m.slot_ord.cpu().numpy().view(np.uint32)
    order = np.argsort(ords, axis=1, kind='stable')                      # free slots (all ones) last
    sums = np.take_along_axis(m.slot_sum.cpu().numpy(), order[:, :, None], axis=1)
    ok = ~want['over']
    assert np.array_equal(np.take_along_axis(ords, order, axis=1)[ok], want['slot_ord'][ok]), (what, 'slot_ord')
    assert np.array_equal(sums[ok], want['slot_sum'][ok]), (what, 'slot_sum')
    held = ords != dref.FREE                                               # the occupied slots are a prefix of the eight
    assert bool((held[:, :-1] >= held[:, 1:]).all()), (what, 'prefix')
    assert m.gain_pairs_words.dtype == torch.int64 and np.array_equal(m.gain_pairs_words.cpu().numpy(), want['pairs']), (what, 'pairs')
    assert np.array_equal(m.gain_diag().cpu().numpy(), want['diag']), (what, 'diag')
    assert not bool(m.gain_diag_words[:, 4:].any()), (what, 'diag padding')


def relative(got, want):
    return float(np.abs(np.asarray(got, np.float64) / np.asarray(want, np.float64) - 1).max())


# ---- 1, 2. the integer state, exact, on the chain and on real geometry; 5. the solved gains -----------------------------------------------

@pytest.mark.parametrize('key', ['chain', 'deep'])
def test_slots_pairs_and_diag_equal_the_restatement(key):
    """Measured on an MI355X: the solved gains equal the restatement's to the bit on both cases (largest relative difference 0)."""
    views, Js, axes, gsd, want = case(key)
    shared = want['span'][:, 0] < want['span'][:, 1]
    reach = (want['S'][:, :, 0] > 0).sum(axis=0)
    print(f'{key}: {want["Wm"]} x {want["Hm"]} cells, {int(shared.sum())} shared, at most {int(reach.max())} images in one, '
          f'{want["excluded"]} excluded; {int((want["pairs"][:, :, 3] > 0).sum())} pairs; diag n {want["diag"][:, 0].tolist()}')
    # conditions on the restatement, not on the code under test
    assert shared.any() and (~shared & (want['span'][:, 0] != 0xffffffff)).any() and want['excluded'] == 0
    assert int(reach.max()) >= (3 if key == 'deep' else 2) and bool((want['diag'][:, 0] > 0).all())
    m = state_by_hand(views, Js, axes, gsd)
    check_state(m, want, key)
    solved = m.solve_gains_direct().cpu().numpy()
    diff = relative(solved, want['direct'])
    print(f'{key}: solved gains against the restatement\'s: largest relative difference {diff:.3g}')
    assert m.gain_kept == want['kept'] == [] and diff <= 2.0 ** -20
    assert not np.array_equal(want['direct'], np.ones_like(want['direct']))


# ---- 3. overflow ----------------------------------------------------------------------------------------------------------------------------

def test_nine_coincident_views_overflow_every_shared_cell_and_eight_none():
    hv, hJ = chain.fan(1, 0.0)
    hv[0].depth = torch.full((24, 32), chain.PLANE)
    hv[0].rgb = torch.zeros((24, 32, 3), dtype=torch.uint8)
    hJ[0] = torch.rand((24, 32, 3), generator=torch.Generator().manual_seed(3)) + 0.1
    v, J = on_device(hv, hJ)
    for n in (9, 8):
        views, Js = v * n, [J[0] * (0.8 + 0.05 * i) for i in range(n)]
        want = dref.state(hv * n, [x.cpu() for x in Js], torch.eye(3), 0.04)
        shared = int((want['span'][:, 0] < want['span'][:, 1]).sum())
        assert shared > 0 and want['excluded'] == (shared if n == 9 else 0)
        check_state(state_by_hand(views, Js, torch.eye(3), 0.04), want, n)
        got = engine.mosaic_of(views, Js, torch.eye(3), 0.04, gains=1, gain_solve='direct').result()
        assert got['gain_excluded_cells'] == want['excluded'] and type(got['gain_excluded_cells']) is int
        assert got['gain_shared_cells'] == shared and type(got['gain_shared_cells']) is int and got['gain_kept'] == []
        if n == 9:      # nothing is left to solve from: every gain is exactly 1, and nothing overlaps
            assert bool((got['gains'] == 1).all()) and bool((got['gain_direct'] == 1).all()) and not bool(got['gain_diag'].any())
            assert tuple(got['gain_pair_index'].shape) == (0, 2) and got['gain_components'] == 0
        else:
            assert not bool((got['gains'] == 1).all()) and tuple(got['gain_pair_index'].shape) == (36, 2) and got['gain_components'] == 1


@pytest.mark.parametrize('key', [(12, 0.04), (40, 0.012)])
def test_a_fan_of_views_overflows_in_the_middle_only(key):
    views, Js, axes, gsd, want = case(key)
    shared = want['span'][:, 0] < want['span'][:, 1]
    assert 0 < want['excluded'] < int(shared.sum()) and int(want['slot_ord'][want['slot_ord'] != dref.FREE].max()) == key[0] - 1
    check_state(state_by_hand(views, Js, axes, gsd), want, key)
    check_state(state_by_hand(views, Js, axes, gsd, splits=(3, 4, 11), reverse=True, plain=(True, True, True)), want, (key, 'plain'))
    got = engine.mosaic_of(views, Js, axes, gsd, gains=1, gain_solve='direct', batch=5).result()
    assert got['gain_excluded_cells'] == want['excluded'] and got['gain_components'] == dref.components(want['pairs'], want['diag'])
    assert relative(got['gain_direct'].cpu().numpy(), want['direct']) <= 2.0 ** -20


# ---- 4. the same bits in every variant ------------------------------------------------------------------------------------------------------

VARIANTS = [dict(splits=(1, 2, 3, 4, 5)), dict(splits=(5,)), dict(splits=(2, 4), reverse=True), dict(plain=(True, False, False)),
            dict(plain=(False, True, False)), dict(plain=(False, False, True)), dict(table=1), dict(table=2), dict(table=64, splits=(3,))]


@pytest.mark.parametrize('kw', VARIANTS, ids=lambda kw: ' '.join(f'{k}={v}' for k, v in kw.items()))
def test_batches_order_and_atomic_forms_leave_the_same_bits(kw):
    views, Js, axes, gsd, want = case('deep')
    assert int((want['pairs'][:, :, 3] > 0).sum()) > 2                    # more pairs than a table of 1 or 2 entries holds
    check_state(state_by_hand(views, Js, axes, gsd, **kw), want, kw)


def test_the_methods_refuse_what_they_cannot_do(monkeypatch):
    views, Js, axes, gsd, _ = case('deep')
    batches = [(0, lambda: (views, Js))]
    m = engine.Mosaic(axes, gsd, DEV)
    m.add_bounds(views, Js)
    m.begin(gains=1)
    calls = (lambda: m.add_gain_slots(views, Js, 0), lambda: m.gain_pairs(), lambda: m.add_gain_diag(views, Js, 0),
             lambda: m.solve_gains_direct())
    for call in calls:
        with pytest.raises(ValueError, match="was not given gain_solve='direct'"):
            call()
    for bad in ('exact', 1):
        with pytest.raises(ValueError, match='must be one of rounds or direct') as e:
            m.begin(gains=1, gain_solve=bad)
        assert e.value.field == 'gain_solve'
    with pytest.raises(ValueError, match=r'Mosaic.begin: the solve finds the gains of the first round') as e:
        m.begin(gain_solve='direct')
    assert e.value.field == 'gain_solve'
    m.begin(gains=1, gain_solve='direct')
    for call in calls:
        with pytest.raises(ValueError, match='a whole gain pass comes first'):
            call()
    m.splat(views, Js, 0)
    m.add_span(views, Js, 0)
    m.gain_pass(batches)
    for call in calls[1:]:
        with pytest.raises(ValueError, match=r'add_gain_slots\(\) over every image comes first'):
            call()
    assert set(m.result()) & set(DIRECT_KEYS) == set()
    # a device with too little memory: refused before anything is allocated, naming the flag and the images
    monkeypatch.setattr(engine, '_device_free_bytes', lambda device: m.Hm * m.Wm * 292)
    with pytest.raises(ValueError, match=rf'--mosaic-gsd, fewer than {len(views)} images') as e:
        m.add_gain_slots(views, Js, 0)
    assert e.value.field == 'gain_solve' and m.slot_ord is None and m.gain_pairs_words is None
    monkeypatch.undo()
    m.add_gain_slots(views, Js, 0)
    with pytest.raises(ValueError, match=r'gain_pairs\(\) and add_gain_diag\(\) over every image come first'):
        m.solve_gains_direct()
    with pytest.raises(Exception, match='table_entries'):
        m.gain_pairs(table_entries=3)
    m.gain_pairs()
    for call in (lambda: m.gain_pairs(), lambda: m.add_gain_slots(views, Js, 0)):
        with pytest.raises(ValueError, match='already'):
            call()


# ---- 6. the chain through mosaic_of ---------------------------------------------------------------------------------------------------------

def test_the_chain_agrees_after_one_direct_solve_and_only_the_colours_change():
    """Measured on an MI355X: gain x factor spread 0.710339 -> 0.000132755 (bound 2^-6 = 0.015625); RMS disagreement R 0.00997823 ->
    2.25387e-05, G 0.0124699 -> 1.8113e-05, B 0.0087282 -> 0 (the restatement's figures, which the device equals)."""
    views, Js, axes, gsd, want = case('chain')
    rest = dict(blend=0.5, fill=0.1)
    m = engine.mosaic_of(views, Js, axes, gsd, gains=1, gain_limit=chain.LIMIT, gain_solve='direct', **rest)
    got = m.result()
    before, after = chain.spread(torch.ones(chain.N, 3)), chain.spread(got['gains'].cpu())
    rms = got['gain_rms']
    print(f'chain: gain x factor spread {before:.6g} -> {after:.6g} (bound {chain.BOUND:.6g}); RMS disagreement '
          + ' '.join(f'{ch} {float(rms[0, c]):.6g} -> {float(rms[1, c]):.6g}' for c, ch in enumerate('RGB')))
    assert after <= chain.BOUND
    assert bool((rms[1] < rms[0] / 100).all())
    assert np.array_equal(got['gain_sums'].cpu().numpy(), want['sums']) and np.array_equal(rms.numpy(), want['rms'])
    assert same_bits(got['gains'], got['gain_direct']) and relative(got['gains'].cpu().numpy(), want['gains']) <= 2.0 ** -20
    assert got['gain_solve'] == 'direct' and got['gain_prior'] == 2.0 ** -20 and got['gain_components'] == 1 and got['gain_excluded_cells'] == 0
    index = got['gain_pair_index']
    index = index.cpu()
    assert index.dtype == torch.int32
    assert index.tolist() == sorted([[i, i] for i in range(chain.N)] + [[i, i + 1] for i in range(chain.N - 1)])
    assert got['gain_pair_words'].dtype == torch.int64 and np.array_equal(
        got['gain_pair_words'].cpu().numpy(), want['pairs'][index[:, 0].numpy(), index[:, 1].numpy()])
    assert np.array_equal(got['gain_diag'].cpu().numpy(), want['diag'])
    # every key that is no J keeps the bytes of a run without gains; every J is that of a run on J x gain
    was = engine.mosaic_of(views, Js, axes, gsd, **rest).result()
    scaled = engine.mosaic_of(views, [J * got['gains'][i] for i, J in enumerate(Js)], axes, gsd, **rest).result()
    assert list(got) == list(was) + list(GAIN_KEYS) + list(DIRECT_KEYS)
    for k, v in was.items():
        if not torch.is_tensor(v):
            assert got[k] == v, k
        elif k.startswith('J'):
            assert same_bits(got[k], scaled[k]) and not same_bits(got[k], v), k
        else:
            assert same_bits(got[k], v), k


def test_rounds_is_today_s_path_and_more_rounds_run_from_the_direct_table():
    views, Js, axes, gsd, _ = case('deep')
    today = engine.mosaic_of(views, Js, axes, gsd, gains=2, blend=0.5, batch=4).result()
    for solve in ('rounds', None):
        got = engine.mosaic_of(views, Js, axes, gsd, gains=2, blend=0.5, batch=4, gain_solve=solve).result()
        assert list(got) == list(today)
        for k, v in today.items():
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, (solve, k)
    # R = 2 with the direct solve: the second round's solve is the rounds', from the direct table (the restatement's flow)
    hv, hJ = scene_case('deep')[4:6]
    want = dref.gains(hv, hJ, axes, gsd, 2, 2.0)
    got = engine.mosaic_of(views, Js, axes, gsd, gains=2, batch=4, gain_solve='direct').result()
    assert tuple(got['gain_sums'].shape) == (3, len(views), 10) and np.array_equal(got['gain_sums'][0].cpu().numpy(), want['sums'][0])
    assert relative(got['gain_direct'].cpu().numpy(), want['direct']) <= 2.0 ** -20
    assert relative(got['gains'].cpu().numpy(), want['gains']) <= 2.0 ** -18       # one more float32 table and quantised pass on top
    assert not same_bits(got['gains'], got['gain_direct'])


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def direct_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_gain_direct_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    rest = ['--mosaic-blend', '0.5', '--mosaic-surface', '0.005', '--mosaic-gains', '2']
    runs = {'gains': rest, 'rounds': rest + ['--mosaic-gain-solve', 'rounds'], 'direct': rest + ['--mosaic-gain-solve', 'direct']}
    printed = {}
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        for i, path in enumerate(sorted(restored.glob('*.pt'))):      # the images disagree by known factors
            data = torch.load(path)
            if isinstance(data, dict) and 'J' in data:
                data['J'] = (data['J'] * torch.tensor(FACTORS[i % len(FACTORS)]).to(data['J'].device)).contiguous()
                torch.save(data, path)
        for name, extra in runs.items():
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                sucre.main(base + ['--output-dir', str(root / name), '--mosaic', str(restored)] + extra)
            printed[name] = text.getvalue()
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, scene, restored, printed, base


LINE = re.compile(r'^mosaic gain solve direct: (\d+) overlapping pairs among (\d+) images in (\d+) connected groups; (\d+) of (\d+) shared cells '
                  r'hold more than 8 images and are left out$')


def test_cli_writes_what_the_engine_computes_and_prints_one_more_line(direct_run):
    from sucre_amd import sfm
    root, scene, restored, printed, _ = direct_run
    names = [v.name for v in scene.views]
    model = sfm.COLMAPModel(root / 'model', root / 'images', root / 'depth')
    views = [model[n].device_view(DEV) for n in names]
    Js = [torch.load((restored / n).with_suffix('.pt'))['J'].to(DEV) for n in names]
    axes = sucre.mosaic_axes(list(model[n] for n in names))
    gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
    m = engine.mosaic_of(views, Js, axes, gsd, blend=0.5, surface=0.005, gains=2, gain_solve='direct', batch=4)
    got, was, rounds = (torch.load(root / name / 'mosaic.pt') for name in ('direct', 'gains', 'rounds'))
    assert set(got) - set(was) == set(DIRECT_KEYS) and not set(was) - set(got)
    for k, v in m.result().items():
        assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert got['gain_solve'] == 'direct' and got['gain_direct'].dtype == torch.float32 and tuple(got['gain_direct'].shape) == (len(names), 3)
    assert got['gain_pair_index'].dtype == torch.int32 and got['gain_pair_words'].dtype == torch.int64 and got['gain_diag'].dtype == torch.int64
    assert tuple(got['gain_pair_words'].shape) == (len(got['gain_pair_index']), 4) and tuple(got['gain_diag'].shape) == (len(names), 4)
    assert sorted(p.name for p in (root / 'direct').iterdir()) == sorted(p.name for p in (root / 'gains').iterdir())
    for k, v in was.items():      # every key that is no J or gain keeps its bytes
        if not k.startswith('J') and not k.startswith('gain'):
            assert same_bits(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert not same_bits(got['gains'], was['gains'])
    # --mosaic-gain-solve rounds is the run without the flag, file for file and key for key
    assert list(rounds) == list(was) and printed['rounds'] == printed['gains']
    for k, v in was.items():
        assert same_bits(rounds[k], v) if torch.is_tensor(v) else rounds[k] == v, k
    for p in (root / 'gains').iterdir():
        if p.name != 'mosaic.pt':
            assert p.read_bytes() == (root / 'rounds' / p.name).read_bytes(), p.name
    lines, lines_was = printed['direct'].splitlines(), printed['gains'].splitlines()
    at = next(i for i, line in enumerate(lines) if line.startswith('mosaic gains of ')) + 1
    hit = LINE.match(lines[at])
    assert hit, lines[at]
    assert len(lines) == len(lines_was) + 1 and lines[at + 1:] == lines_was[at:] and 'gain solve' not in printed['gains']
    index, span = got['gain_pair_index'], m.span.cpu().numpy().view(np.uint32)
    assert hit.groups() == (str(int((index[:, 0] < index[:, 1]).sum())), str(int((got['gain_diag'][:, 0] > 0).sum())),
                            str(got['gain_components']), str(got['gain_excluded_cells']), str(int((span[:, 0] < span[:, 1]).sum())))
    assert got['gain_shared_cells'] == int((span[:, 0] < span[:, 1]).sum()) and got['gain_kept'] == []
    assert int(hit.group(1)) > 0 and bool((got['gain_rms'][1] < got['gain_rms'][0]).all())


def test_cli_refuses_a_lone_flag_and_a_bad_value(direct_run):
    root, _, restored, _, base = direct_run
    out = ['--output-dir', str(root / 'refused')]
    for extra, code in ((['--mosaic-gain-solve', 'direct'], '--mosaic-gain-solve: only with --mosaic-gains R'),
                        (['--mosaic', str(restored), '--mosaic-gain-solve', 'direct'], '--mosaic-gain-solve: only with --mosaic-gains R'),
                        (['--mosaic', str(restored), '--mosaic-gains', '2', '--mosaic-gain-solve', 'exact'],
                         '--mosaic-gain-solve: S must be rounds or direct, not exact')):
        with pytest.raises(SystemExit) as e:
            sucre.main(base + out + extra)
        assert e.value.code == code
    assert not (root / 'refused').exists()
