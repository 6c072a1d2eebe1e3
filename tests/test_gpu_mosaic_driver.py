"""GPU tests of what the mosaic's host side hands out, whatever drives the phases: the keys of ``Mosaic.result()`` with their shapes,
dtypes and empty values, the files, keys and printed lines of the command line, and the order of its calls -- in the six
combinations of --mosaic-blend, --mosaic-feather and --mosaic-fill.  Every key set, file list and call sequence is written out
here.  The scene is the small survey of test_gpu_mosaic.py (6 images of 96x64)."""
import contextlib
import io
import os
import re

import pytest
import torch

from sucre_amd import engine, sucre, synth
from test_gpu_mosaic import DEV, views_of

pytestmark = pytest.mark.gpu

BLEND, FEATHER, FILL = 0.5, 8, 0.05
COMBINATIONS = {'plain': {}, 'blend': {'blend': BLEND}, 'blend_feather': {'blend': BLEND, 'feather': FEATHER}, 'fill': {'fill': FILL},
                'blend_fill': {'blend': BLEND, 'fill': FILL}, 'all': {'blend': BLEND, 'feather': FEATHER, 'fill': FILL}}

NAN = float('nan')
# key -> (trailing shape, dtype, value of a cell without a source; None: see the fill's check)
BEST = {'J': ((3,), torch.float32, NAN), 'raw': ((3,), torch.uint8, 0), 'source': ((), torch.int32, -1), 'pixel': ((), torch.int32, -1),
        'range': ((), torch.float32, NAN)}
BLENDED = {'J_blend': ((3,), torch.float32, NAN), 'raw_blend': ((3,), torch.uint8, 0), 'weight': ((), torch.float32, 0),
           'samples': ((), torch.int32, 0)}
FILLED = {'fill_level': ((), torch.int32, None), 'J_filled': ((3,), torch.float32, None), 'raw_filled': ((3,), torch.uint8, None)}
BLEND_FILLED = {'J_blend_filled': ((3,), torch.float32, None), 'raw_blend_filled': ((3,), torch.uint8, None)}
TENSORS = {'plain': BEST, 'blend': {**BEST, **BLENDED}, 'blend_feather': {**BEST, **BLENDED}, 'fill': {**BEST, **FILLED},
           'blend_fill': {**BEST, **BLENDED, **FILLED, **BLEND_FILLED}, 'all': {**BEST, **BLENDED, **FILLED, **BLEND_FILLED}}
RESULT_KEYS = {
    'plain': ['J', 'raw', 'source', 'pixel', 'range'],
    'blend': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples'],
    'blend_feather': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'feather'],
    'fill': ['J', 'raw', 'source', 'pixel', 'range', 'fill_level', 'J_filled', 'raw_filled'],
    'blend_fill': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'fill_level', 'J_filled', 'raw_filled',
                   'J_blend_filled', 'raw_blend_filled'],
    'all': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'feather', 'fill_level', 'J_filled',
            'raw_filled', 'J_blend_filled', 'raw_blend_filled'],
}


def holds(t, value):
    return bool(torch.isnan(t).all()) if value != value else bool((t == value).all())


@pytest.mark.parametrize('name', list(COMBINATIONS))
def test_result_holds_these_keys_with_these_shapes_dtypes_and_empty_values(name):
    views, Js, axes, gsd = views_of('survey')
    gsd = gsd * 0.5      # half the default cell: about 600 of the 8800 cells stay empty
    m = engine.mosaic_of(views, Js, axes, gsd, batch=4, **COMBINATIONS[name])      # two calls per phase: four images and two
    out = m.result()
    assert list(out) == RESULT_KEYS[name]
    if 'feather' in out:
        assert out['feather'] == FEATHER and type(out['feather']) is int
    empty = out['source'] < 0
    assert 0 < int(empty.sum()) < empty.numel()
    for key, (tail, dtype, value) in TENSORS[name].items():
        t = out[key]
        assert tuple(t.shape) == (m.Hm, m.Wm) + tail and t.dtype == dtype and t.device == torch.device(DEV) and t.is_contiguous(), key
        if value is not None:
            assert holds(t[empty], value), key
    if 'fill_level' in out:
        level = out['fill_level']
        assert bool((level[~empty] == 0).all()) and bool(((level[empty] == -1) | ((level[empty] >= 1) & (level[empty] <= m.fill_levels))).all())
        assert 0 < int((level > 0).sum())
        left = level < 0
        for J, raw in (('J_filled', 'raw_filled'), ('J_blend_filled', 'raw_blend_filled'))[:2 if 'blend' in COMBINATIONS[name] else 1]:
            assert holds(out[J][left], NAN) and holds(out[raw][left], 0)
            assert not bool(torch.isnan(out[J][level > 0]).any())


# ---- the command line ---------------------------------------------------------------------------------------------------------------

REAL_MOSAIC = engine.Mosaic


class Spy(REAL_MOSAIC):
    """Records ``(name, ordinal of the batch's first image or None, number of images or None)`` and then does what ``Mosaic`` does."""
    log = []


def _spied(name):
    def method(self, *args, **kwargs):
        walks = name in ('add_bounds', 'splat', 'resolve', 'gather', 'accumulate')
        first = (args[2] if len(args) > 2 else kwargs.get('first_ordinal')) if walks and name != 'add_bounds' else None
        Spy.log.append((name, first, len(args[0]) if walks else None))
        return getattr(REAL_MOSAIC, name)(self, *args, **kwargs)
    return method


for _name in ('__init__', 'add_bounds', 'begin', 'splat', 'resolve', 'gather', 'accumulate', 'normalize', 'fill'):
    setattr(Spy, _name, _spied(_name))


@pytest.fixture(scope='module')
def cli_runs(tmp_path_factory):
    """The survey on disk, restored with its true water, then --mosaic in the six combinations under a cache budget of one and a
    half restored images: six batches of one image, every file read again in every phase."""
    root = tmp_path_factory.mktemp('mosaic_driver_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    flags = {'blend': '--mosaic-blend', 'feather': '--mosaic-feather', 'fill': '--mosaic-fill'}
    printed, calls = {}, {}
    saved = {k: os.environ.pop(k, None) for k in ('WORLD_SIZE', 'SUCRE_CONSISTENCY_CACHE_GB')}
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        os.environ['SUCRE_CONSISTENCY_CACHE_GB'] = str(1.5 * 96 * 64 * 12 / 2 ** 30)
        engine.Mosaic = Spy
        for name, options in COMBINATIONS.items():
            Spy.log = []
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                sucre.main(base + ['--output-dir', str(root / name), '--mosaic', str(restored), '--mosaic-gsd', '0.04']
                           + [x for k, v in options.items() for x in (flags[k], str(v))])
            printed[name], calls[name] = text.getvalue(), Spy.log
    finally:
        engine.Mosaic = REAL_MOSAIC
        os.environ.pop('SUCRE_CONSISTENCY_CACHE_GB', None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return root, scene, printed, calls


BEST_FILES = ['mosaic.png', 'mosaic.pt', 'mosaic_raw.png', 'mosaic_source.png']
BLEND_FILES = ['mosaic_blend.png', 'mosaic_blend_raw.png']
FILL_FILES = ['mosaic_filled.png', 'mosaic_filled_mask.png', 'mosaic_raw_filled.png']
BLEND_FILL_FILES = ['mosaic_blend_filled.png', 'mosaic_blend_raw_filled.png']
FILES = {'plain': BEST_FILES, 'blend': BEST_FILES + BLEND_FILES, 'blend_feather': BEST_FILES + BLEND_FILES, 'fill': BEST_FILES + FILL_FILES,
         'blend_fill': BEST_FILES + BLEND_FILES + FILL_FILES + BLEND_FILL_FILES, 'all': BEST_FILES + BLEND_FILES + FILL_FILES + BLEND_FILL_FILES}
META = ['axes', 'gsd', 'lo', 'images', 'n_filled', 'per_image']
PT_KEYS = {
    'plain': ['J', 'raw', 'source', 'pixel', 'range'] + META,
    'blend': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples'] + META + ['blend'],
    'blend_feather': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'feather'] + META + ['blend'],
    'fill': ['J', 'raw', 'source', 'pixel', 'range', 'fill_level', 'J_filled', 'raw_filled'] + META + ['fill', 'fill_levels'],
    'blend_fill': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'fill_level', 'J_filled', 'raw_filled',
                   'J_blend_filled', 'raw_blend_filled'] + META + ['blend', 'fill', 'fill_levels'],
    'all': ['J', 'raw', 'source', 'pixel', 'range', 'J_blend', 'raw_blend', 'weight', 'samples', 'feather', 'fill_level', 'J_filled',
            'raw_filled', 'J_blend_filled', 'raw_blend_filled'] + META + ['blend', 'fill', 'fill_levels'],
}
NUMBER = r'[0-9.e+-]+'
LINE = {
    'mosaic': rf'mosaic of 6 images: \d+ x \d+ cells of 0\.04 m, \d+ filled \(\d+\.\d %\), \d+ empty; largest share img_\S+ \(\d+\.\d %\)',
    'blend': rf'mosaic blend of depth 0\.5 m: \d+ samples, \d+\.\d\d per filled cell on average, \d+ at most; '
             rf'\d+\.\d % of the filled cells blend more than one sample',
    'feather': rf'mosaic feather of 8 px: \d+\.\d % of the samples within 8 px of an edge; smallest weight sum in a filled cell {NUMBER}',
    'fill': r'mosaic fill of 0\.05 m \(\d+ levels\): \d+ cells filled, \d+ left empty; deepest level \d+',
}
LINES = {'plain': ['mosaic'], 'blend': ['mosaic', 'blend'], 'blend_feather': ['mosaic', 'blend', 'feather'], 'fill': ['mosaic', 'fill'],
         'blend_fill': ['mosaic', 'blend', 'fill'], 'all': ['mosaic', 'blend', 'feather', 'fill']}


@pytest.mark.parametrize('name', list(COMBINATIONS))
def test_cli_writes_these_files_and_keys_and_prints_these_lines(cli_runs, name):
    root, scene, printed, _ = cli_runs
    assert sorted(p.name for p in (root / name).iterdir()) == sorted(FILES[name])
    got = torch.load(root / name / 'mosaic.pt')
    assert list(got) == PT_KEYS[name]
    Hm, Wm = got['source'].shape
    for key, (tail, dtype, _) in TENSORS[name].items():
        assert tuple(got[key].shape) == (Hm, Wm) + tail and got[key].dtype == dtype and got[key].device.type == 'cpu', key
    assert got['images'] == [v.name for v in scene.views] and type(got['gsd']) is float and type(got['n_filled']) is int
    for key, kind, value in (('blend', float, BLEND), ('feather', int, FEATHER), ('fill', float, FILL)):
        if key in COMBINATIONS[name]:
            assert type(got[key]) is kind and got[key] == value
    if 'fill' in COMBINATIONS[name]:
        assert type(got['fill_levels']) is int and got['fill_levels'] >= 1
    lines = printed[name].splitlines()
    assert lines[0] == 'Loading COLMAP model.' and len(lines) == 2 + len(LINES[name]) and lines[1].startswith('--mosaic: the restored images of ')
    for line, kind in zip(lines[2:], LINES[name]):
        assert re.fullmatch(LINE[kind], line), (kind, line)


NEW = [('__init__', None, None)]
BOUNDS = [('add_bounds', None, 1), ('add_bounds', None, 1), ('add_bounds', None, 1), ('add_bounds', None, 1), ('add_bounds', None, 1),
          ('add_bounds', None, 1)]
BEGIN = [('begin', None, None)]
SPLAT = [('splat', 0, 1), ('splat', 1, 1), ('splat', 2, 1), ('splat', 3, 1), ('splat', 4, 1), ('splat', 5, 1)]
RESOLVE = [('resolve', 0, 1), ('resolve', 1, 1), ('resolve', 2, 1), ('resolve', 3, 1), ('resolve', 4, 1), ('resolve', 5, 1)]
GATHER = [('gather', 0, 1), ('gather', 1, 1), ('gather', 2, 1), ('gather', 3, 1), ('gather', 4, 1), ('gather', 5, 1)]
ACCUMULATE = [('accumulate', 0, 1), ('accumulate', 1, 1), ('accumulate', 2, 1), ('accumulate', 3, 1), ('accumulate', 4, 1), ('accumulate', 5, 1)]
NORMALIZE = [('normalize', None, None)]
FILLS = [('fill', None, None)]


def test_cli_runs_every_phase_over_every_batch_before_the_next_phase_starts(cli_runs):
    _, _, _, calls = cli_runs
    assert calls['all'] == NEW + BOUNDS + BEGIN + SPLAT + RESOLVE + GATHER + ACCUMULATE + NORMALIZE + FILLS
    assert calls['plain'] == NEW + BOUNDS + BEGIN + SPLAT + RESOLVE + GATHER
    assert calls['blend_fill'] == calls['all'] and calls['blend'] == calls['blend_feather'] == calls['all'][:-1]
    assert calls['fill'] == calls['plain'] + FILLS


def test_cli_takes_the_shallowest_blend_depth_of_the_range(cli_runs):
    """--mosaic-blend 1e-6, the lower end: H becomes float32(1e-6), which lies below 1e-6, and ``Mosaic.begin`` checks it again."""
    root, scene, _, _ = cli_runs
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        with contextlib.redirect_stdout(io.StringIO()) as text:
            sucre.main(base + ['--output-dir', str(root / 'shallowest'), '--mosaic', str(root / 'restored'), '--mosaic-gsd', '0.04', '--mosaic-blend', '1e-6'])
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    got = torch.load(root / 'shallowest' / 'mosaic.pt')
    assert list(got) == PT_KEYS['blend'] and got['blend'] == float(torch.tensor(1e-6, dtype=torch.float32)) < 1e-6
    assert text.getvalue().splitlines()[-1].startswith('mosaic blend of depth 1e-06 m: ')
    plain = torch.load(root / 'plain' / 'mosaic.pt')
    assert all(torch.equal(got[k], plain[k]) for k in ('source', 'pixel', 'raw'))
    assert bool((got['samples'][got['source'] >= 0] >= 1).all())
