"""GPU tests of the mosaic's hole filling (sucre_mosaic_fill_pull / _push, engine.Mosaic.fill, sucre.mosaic, --mosaic-fill).

The yardstick is tests/mosaic_fill_ref.py, a numpy restatement that shares no code with the engine (float32, one operation per
line); test_mosaic_fill_host.py checks it on grids filled by hand.  Every comparison is EXACT: the three outputs and every record of
the pyramid, bit for bit -- the fill is a fixed chain of IEEE operations per cell.
"""
import contextlib
import ctypes as C
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mosaic_fill_ref as fref
from sucre_amd import _lib, engine, sucre, synth

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BEST = ('source', 'pixel', 'range', 'J', 'raw')
BLENDED = ('J_blend', 'raw_blend', 'weight', 'samples')
FILLED = ('J_filled', 'raw_filled', 'fill_level')
NAN = float('nan')


def same_bits(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def random_grid(H, W, seed, share):
    """Random colours in (-1, 2) and bytes on ``share`` of the cells; NaN, 0 and -1 elsewhere, as a mosaic leaves its empty cells."""
    rng = np.random.default_rng(seed)
    valid = rng.random((H, W)) < share
    J = (rng.random((H, W, 3), dtype=np.float32) * np.float32(3) - np.float32(1)).astype(np.float32)
    raw = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    J[~valid], raw[~valid] = NAN, 0
    return J, raw, np.where(valid, rng.integers(0, 9, (H, W)), -1).astype(np.int32)


class DeviceFill:
    """The three entries called directly on device copies of a grid."""

    def __init__(self, J, raw, source, L):
        self.lib = _lib.load()
        self.H, self.W = source.shape
        self.L = L
        self.J, self.raw, self.source = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (J, raw, source))
        n = self.lib.sucre_mosaic_fill_bytes(self.H, self.W, L)
        assert n == fref.pyramid_bytes(self.H, self.W, L) and n > 0
        self.pyramid = torch.full((n,), 0xa5, dtype=torch.uint8, device=DEV)     # junk: every record must be written
        self.out = {'J_filled': torch.full((self.H, self.W, 3), 7.0, device=DEV), 'raw_filled': torch.full((self.H, self.W, 3), 77, dtype=torch.uint8, device=DEV),
                    'fill_level': torch.full((self.H, self.W), 77, dtype=torch.int32, device=DEV)}

    def _base(self):
        return (self.H, self.W, self.L, C.c_void_p(self.J.data_ptr()), C.c_void_p(self.raw.data_ptr()), C.c_void_p(self.source.data_ptr()),
                C.c_void_p(self.pyramid.data_ptr()))

    def pull(self):
        with torch.cuda.device(DEV):
            _lib.check(self.lib.sucre_mosaic_fill_pull(*self._base(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def push(self):
        with torch.cuda.device(DEV):
            _lib.check(self.lib.sucre_mosaic_fill_push(*self._base(), *[C.c_void_p(self.out[k].data_ptr()) for k in FILLED],
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def records(self):
        """The levels 1..L as (cells, 8) float32, the alignment's padding left out."""
        raw, at, out = self.pyramid.cpu().numpy(), 0, []
        for h, w in fref.level_sizes(self.H, self.W, self.L)[1:]:
            out.append(raw[at:at + h * w * 32].view(np.float32).reshape(h * w, 8).copy())
            at += (h * w * 32 + 255) // 256 * 256
        return out


def check_grid(J, raw, source, L, what):
    want = fref.fill(J, raw, source, L)
    d = DeviceFill(J, raw, source, L)
    d.pull()
    d.push()
    torch.cuda.synchronize()
    level = want['fill_level']
    print(f'{what}: {source.shape[1]} x {source.shape[0]} cells, L = {L}: {int((level == 0).sum())} measured, {int((level > 0).sum())} filled, '
          f'{int((level < 0).sum())} left empty, deepest level {int(level.max())}')
    for k in FILLED:
        got = d.out[k].cpu().numpy()
        assert same_bits(got, want[k]), (what, k, int((got.view(np.uint8) != want[k].view(np.uint8)).sum()))
    for l, (got, rec) in enumerate(zip(d.records(), want['pyramid']), 1):
        assert np.array_equal(got.view(np.uint32), rec.view(np.uint32)), (what, 'level', l)
    # the inputs are read, never written
    assert same_bits(d.J, J) and same_bits(d.raw, raw) and same_bits(d.source, source)
    return want, d


SHAPES = [(1, 1, 1, 1.0), (1, 1, 1, 0.0), (1, 9, 1, 0.3), (1, 9, 4, 0.12), (5, 1, 2, 0.3), (5, 1, 3, 0.5),
          (37, 53, 1, 0.3), (37, 53, 2, 0.05), (37, 53, 3, 0.02),
          (64, 64, 6, 0.002),        # level 6 is 1x1
          (257, 129, 4, 0.01)]       # odd at every level -- 129x65, 65x33, 33x17, 17x9 --, several workgroups each way at level 0


@pytest.mark.parametrize('H, W, L, share', SHAPES, ids=[f'{H}x{W}-L{L}-{share}' for H, W, L, share in SHAPES])
def test_random_grids_equal_the_reference(H, W, L, share):
    J, raw, source = random_grid(H, W, 1000 * H + 10 * W + L, share)
    if share == 1.0:
        assert (source >= 0).all()
    want, _ = check_grid(J, raw, source, L, 'random grid')
    if H * W > 1000:
        assert (want['fill_level'] > 0).any() and (want['fill_level'] == 0).any()
    if (H, W, L) == (64, 64, 6):
        assert (want['fill_level'] >= 0).all() and int(want['fill_level'].max()) >= 5   # 1x1 reached: nothing stays empty
    if (H, W, L) == (37, 53, 1):
        assert (want['fill_level'] < 0).any()


def test_all_cells_valid_gives_the_inputs_back():
    J, raw, source = random_grid(37, 53, 5, 2.0)
    want, d = check_grid(J, raw, source, 3, 'all valid')
    assert same_bits(d.out['J_filled'], J) and same_bits(d.out['raw_filled'], raw) and not bool(d.out['fill_level'].any())


def test_no_cell_valid_gives_nan_zero_and_minus_one():
    J, raw, source = random_grid(37, 53, 6, -1.0)
    want, d = check_grid(J, raw, source, 3, 'none valid')
    assert bool((d.out['fill_level'] == -1).all()) and not bool(d.out['raw_filled'].any())
    assert bool((d.out['J_filled'].view(torch.int32) == 0x7fc00000).all())
    assert not any(r.any() for r in d.records())


@pytest.mark.parametrize('L', [1, 3, 6])
def test_one_valid_cell(L):
    J, raw, source = random_grid(37, 53, 7, -1.0)
    J[20, 31], raw[20, 31], source[20, 31] = (0.3, 0.7, 1.1), (1, 128, 255), 4
    want, d = check_grid(J, raw, source, L, 'one valid cell')
    filled = want['fill_level'] > 0
    assert filled.any() and (L < 6 or filled.sum() == 37 * 53 - 1)
    # one colour in every sum: a filled cell holds it to a rounding or two of S / A, and its byte exactly
    assert np.abs(want['J_filled'][filled] - np.float32([0.3, 0.7, 1.1])).max() < 1e-6
    assert (want['raw_filled'][filled] == np.uint8([1, 128, 255])).all()


def test_checkerboard():
    J, raw, source = random_grid(37, 53, 8, 2.0)
    yy, xx = np.mgrid[0:37, 0:53]
    black = (yy + xx) % 2 == 1
    J[black], raw[black], source[black] = NAN, 0, -1
    want, _ = check_grid(J, raw, source, 2, 'checkerboard')
    assert (want['fill_level'][black] == 1).all()


def test_measured_cells_with_special_values_are_kept_and_only_finite_ones_contribute():
    """-0.0 is a colour like any other (and enters the sums as the IEEE rules say); a measured cell with an infinity or a NaN in
    one channel contributes nothing -- its neighbours are filled from the others -- and is itself copied bit for bit."""
    J, raw, source = random_grid(37, 53, 9, 0.05)
    # a block with nothing in it but one cell with an infinity: the holes next to that cell, 12 = 3 x 2^L cells or more from every
    # other measured cell, must stay empty
    J[0:16, 0:20], raw[0:16, 0:20], source[0:16, 0:20] = NAN, 0, -1
    special = {(3, 5): (float('inf'), 0.5, 0.25), (20, 25): (-0.0, 0.5, 0.25), (10, 30): (0.5, -float('inf'), 0.25), (11, 40): (0.5, 0.25, NAN),
               (30, 2): (-0.0, -0.0, -0.0), (36, 52): (NAN, NAN, NAN)}
    for (y, x), j in special.items():
        J[y, x], raw[y, x], source[y, x] = j, (200, 100, 50), 1
    J[12, 40] = np.uint32(0xffc12345).view(np.float32)     # a NaN with a payload and a sign, measured
    raw[12, 40], source[12, 40] = (1, 2, 3), 2
    want, d = check_grid(J, raw, source, 2, 'special values')
    got = {k: v.cpu().numpy() for k, v in d.out.items()}
    measured = source >= 0
    assert np.array_equal(got['J_filled'][measured].view(np.uint32), J[measured].view(np.uint32))
    assert np.array_equal(got['raw_filled'][measured], raw[measured]) and not got['fill_level'][measured].any()
    assert got['J_filled'][12, 40].view(np.uint32).tolist() == [0xffc12345] * 3
    assert got['fill_level'][3, 6] == -1 and got['fill_level'][2, 5] == -1      # next to the infinity, with nothing else within reach
    filled = got['fill_level'] > 0
    assert filled.any() and np.isfinite(got['J_filled'][filled]).all()


def test_pull_and_push_twice_on_one_pyramid_give_the_same_bits():
    J, raw, source = random_grid(257, 129, 11, 0.01)
    d = DeviceFill(J, raw, source, 4)
    d.pull()
    d.push()
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in d.out.items()}
    records = d.records()
    for v in d.out.values():
        v.fill_(55)
    d.pull()
    d.push()
    torch.cuda.synchronize()
    assert all(same_bits(first[k], d.out[k]) for k in FILLED)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(records, d.records()))
    # and a push alone on the pushed pyramid: its filled cells have w = 1 by now and are left alone
    d.push()
    torch.cuda.synchronize()
    assert all(same_bits(first[k], d.out[k]) for k in FILLED)


# ---- the engine on a survey with real holes ---------------------------------------------------------------------------------------
_SURVEY = {}


def survey():
    """(views, Js, axes, a quarter of the default gsd) of synth.make_survey(96, 64, 3, 2) -- made once and never changed."""
    if not _SURVEY:
        scene = synth.make_survey(96, 64, 3, 2)
        views = engine.device_views_from_scene(scene, DEV)
        g = torch.Generator().manual_seed(77)
        Js = []
        for v in views:
            H, W = v.depth.shape
            J = torch.rand((H, W, 3), generator=g) * 0.98 + 0.01
            J[5:15, 20:40] = NAN      # a patch without a restored colour
            Js.append(J.to(DEV))
        axes = sucre.mosaic_axes(views)
        gsd = sucre.mosaic_default_gsd([v.depth for v in views], [float(v.K[0, 0]) for v in views])
        _SURVEY.update(views=views, Js=Js, axes=axes, gsd=np.float32(gsd * np.float32(0.25)))
    return _SURVEY['views'], _SURVEY['Js'], _SURVEY['axes'], _SURVEY['gsd']


@pytest.mark.parametrize('blend', [None, 0.5], ids=['best view', 'with a blend'])
def test_engine_fill_equals_the_reference_and_leaves_the_other_outputs_alone(blend):
    views, Js, axes, gsd = survey()
    R = 6 * float(gsd)       # 8 gsd >= R > 4 gsd: three levels
    plain = engine.mosaic_of(views, Js, axes, gsd, blend=blend)
    m = engine.mosaic_of(views, Js, axes, gsd, blend=blend, fill=R)
    assert (m.Hm, m.Wm) == (plain.Hm, plain.Wm)
    assert m.fill_levels == 3 == engine.mosaic_fill_levels(R, gsd, m.Hm, m.Wm) and m.fill_reach == R
    before, got = plain.result(), m.result()
    old = BEST + (BLENDED if blend is not None else ())
    new = FILLED + (('J_blend_filled', 'raw_blend_filled') if blend is not None else ())
    assert set(before) == set(old) and set(got) == set(old) | set(new)
    for k in old:
        assert same_bits(before[k], got[k]), k
    host = {k: v.cpu().numpy() for k, v in got.items()}
    holes = int((host['source'] < 0).sum())
    assert holes > 0.2 * m.Hm * m.Wm       # a quarter of the default gsd: real holes
    want = fref.fill(host['J'], host['raw'], host['source'], 3)
    for k in FILLED:
        assert same_bits(host[k], want[k]), k
    closed = int((host['fill_level'] > 0).sum())
    print(f'{m.Wm} x {m.Hm} cells, {holes} holes, {closed} closed at L = 3, {int((host["fill_level"] < 0).sum())} left')
    assert closed > 0.5 * holes
    if blend is not None:
        want = fref.fill(host['J_blend'], host['raw_blend'], host['source'], 3)
        assert same_bits(host['J_blend_filled'], want['J_filled']) and same_bits(host['raw_blend_filled'], want['raw_filled'])
    again = engine.mosaic_of(views, Js, axes, gsd, blend=blend, fill=R)
    assert all(same_bits(again.result()[k], got[k]) for k in new)


def test_fill_refuses_what_it_cannot_do():
    views, Js, axes, gsd = survey()
    m = engine.Mosaic(axes, gsd, DEV)
    with pytest.raises(ValueError, match='begin'):
        m.fill(1.0)
    m.begin(bounds=(0.0, 0.0, 1.0, 1.0))
    for bad in (0.0, 9e-7, 1.1e6, NAN, float('inf')):
        with pytest.raises(ValueError, match='fill reach R'):
            m.fill(bad)
        assert m.pyramid is None and set(m.result()) == set(BEST)     # refused before anything is allocated
    assert m.fill(1e6) == engine.mosaic_fill_levels(1e6, gsd, m.Hm, m.Wm)     # an empty mosaic: nothing to fill from
    torch.cuda.synchronize()
    assert bool((m.result()['fill_level'] == -1).all())


# ---- the command line -------------------------------------------------------------------------------------------------------------
CLI_GSD, CLI_FILL, CLI_BLEND = 0.02, 0.1, 0.5     # a quarter of this survey's default gsd (about 0.08 m); 8 gsd >= R > 4 gsd


@pytest.fixture(scope='module')
def fill_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('mosaic_fill_survey')
    scene = synth.make_survey(96, 64, 3, 2)
    synth.write_to_disk(scene, root)
    torch.save({'B': torch.tensor(synth.GT_B).view(3, 1), 'beta': torch.tensor(synth.GT_BETA).view(3, 1),
                'gamma': torch.tensor(synth.GT_GAMMA).view(3, 1)}, root / 'true_water.pt')
    base = ['--image-dir', str(root / 'images'), '--depth-dir', str(root / 'depth'), '--model-dir', str(root / 'model'),
            '--image-ids', '1', str(len(scene.views) + 1)]
    restored = root / 'restored'
    runs = {'plain': [], 'filled': ['--mosaic-fill', str(CLI_FILL)], 'blend': ['--mosaic-blend', str(CLI_BLEND)],
            'blend_filled': ['--mosaic-blend', str(CLI_BLEND), '--mosaic-fill', str(CLI_FILL)]}
    printed = {}
    saved = os.environ.pop('WORLD_SIZE', None)
    try:
        sucre.main(base + ['--output-dir', str(restored), '--apply-water', str(root / 'true_water.pt')])
        for name, extra in runs.items():
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                sucre.main(base + ['--output-dir', str(root / name), '--mosaic', str(restored), '--mosaic-gsd', str(CLI_GSD)] + extra)
            printed[name] = text.getvalue()
    finally:
        if saved is not None:
            os.environ['WORLD_SIZE'] = saved
    return root, printed


def test_cli_writes_the_new_files_and_leaves_the_old_ones_alone(fill_run):
    from PIL import Image as PILImage
    root, printed = fill_run
    old = ['mosaic.png', 'mosaic.pt', 'mosaic_raw.png', 'mosaic_source.png']
    new = ['mosaic_filled.png', 'mosaic_filled_mask.png', 'mosaic_raw_filled.png']
    blend = ['mosaic_blend.png', 'mosaic_blend_raw.png']
    assert sorted(p.name for p in (root / 'plain').iterdir()) == old
    assert sorted(p.name for p in (root / 'filled').iterdir()) == sorted(old + new)
    assert sorted(p.name for p in (root / 'blend').iterdir()) == sorted(old + blend)
    assert sorted(p.name for p in (root / 'blend_filled').iterdir()) == sorted(old + new + blend + ['mosaic_blend_filled.png', 'mosaic_blend_raw_filled.png'])
    for without, with_fill in (('plain', 'filled'), ('blend', 'blend_filled')):
        for p in (root / without).iterdir():
            if p.suffix == '.png':
                assert p.read_bytes() == (root / with_fill / p.name).read_bytes(), p.name
        was, got = torch.load(root / without / 'mosaic.pt'), torch.load(root / with_fill / 'mosaic.pt')
        extra = set(FILLED) | {'fill', 'fill_levels'} | ({'J_blend_filled', 'raw_blend_filled'} if without == 'blend' else set())
        assert set(got) - set(was) == extra and not set(was) - set(got)
        for k, v in was.items():
            assert same_bits(v, got[k]) if torch.is_tensor(v) else v == got[k], k
        # the lines: those of the run without the flag, then one more, which matches the tensors
        lines_was, lines = printed[without].splitlines(), printed[with_fill].splitlines()
        assert lines[:len(lines_was)] == lines_was and len(lines) == len(lines_was) + 1
        level = got['fill_level']
        assert got['fill'] == CLI_FILL and got['fill_levels'] == 3 == engine.mosaic_fill_levels(CLI_FILL, got['gsd'], *level.shape)
        assert lines[-1] == (f'mosaic fill of {CLI_FILL:.6g} m (3 levels): {int((level > 0).sum())} cells filled, {int((level < 0).sum())} left empty; '
                             f'deepest level {int(level.max())}')
        assert int((level > 0).sum()) > 1000 and int(level.max()) in (1, 2, 3)
        want = fref.fill(got['J'].numpy(), got['raw'].numpy(), got['source'].numpy(), 3)
        for k in FILLED:
            assert same_bits(got[k], want[k]), k
        out = root / with_fill
        assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic_raw_filled.png')), got['raw_filled'].numpy())
        mask = np.where(level.numpy() == 0, 255, np.where(level.numpy() > 0, 128, 0)).astype(np.uint8)
        assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic_filled_mask.png')), mask)
        assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic_filled.png')),
                              np.asarray(sucre.SUCRe.plot_J(SimpleNamespace(J=got['J_filled'], stretch=None))))
        if without == 'blend':
            want = fref.fill(got['J_blend'].numpy(), got['raw_blend'].numpy(), got['source'].numpy(), 3)
            assert same_bits(got['J_blend_filled'], want['J_filled']) and same_bits(got['raw_blend_filled'], want['raw_filled'])
            assert np.array_equal(np.asarray(PILImage.open(out / 'mosaic_blend_raw_filled.png')), got['raw_blend_filled'].numpy())
    assert 'mosaic fill' not in printed['plain'] and 'mosaic fill' not in printed['blend']
