"""GPU tests of the workspace contract: no result may depend on what a buffer held when it was handed to the library.

Every buffer the engine hands over is ``torch.empty`` (the workspace ``ws``, the extension workspace ``lws``, the residual scratch and
its outputs, the group buffer, the batch table, the select scratch, every export target), the library never clears one, and the
pool (``engine.acquire_restoration``) lays the same bytes out again for every target's own view count and mode.  Two mechanisms
put that under test, on problems whose layouts differ in every direction:

  A  every ``torch.empty`` of ``sucre_amd.engine`` returns a device tensor filled with one byte: 0x00 (the baseline), 0xFF (NaN
     as a float, all ones as an integer) and 0x3F (0.747 as a float -- it passes every ``z > 0`` guard, which a NaN fails --,
     16191 as a uint16);
  B  one shared buffer per workspace role, through which all problems run in a fixed order and then in the reverse order: every
     problem finds the bytes of two different predecessors of other shapes, modes and formats under its own layout.

Every run must equal the 0x00 run of its problem BIT FOR BIT -- counts, kept views, the store's format words, every exported
plane, the integrity verdict, the trace, the parameters, J, the three residual tensors, and all of the fit's once more after a
second ``fit`` call (a resumed fit).  No tolerance.  The 0x00 runs of P1, P2 and P8 are held to the CPU oracle with the bars of
tests/test_gpu_api.py::test_survey_of_images_reuses_one_workspace (P1) and of
tests/test_gpu_parity.py::test_six_hundred_views_of_a_small_image (P2, P8), P1's residuals to the float64 sums of
tests/test_gpu_residuals.py; the other modes are anchored by their own tests on fresh buffers.


Who writes what first (the audit behind these tests; csrc/layout.h ``Layout``, csrc/light.hip ``LightLayout``)
--------------------------------------------------------------------------------------------------------------
Notation: region | first writer | first reader | what guards a partial write.  n = the call's own n_views; "all" = every element
the reader can reach is written by the first writer.

match -> finalize (sucre_match_views*, sucre_finalize_matches*)
  obs            | match_kernel: the WHOLE chunk (256 ranges, 768 colour bytes) of every (tile, view) pair with a match
                 | scatter_kernel, export_view*, integrity_scan, residual_kernel | cnt > 0 (pair without a match: chunk never
                 | written, never read); inside a written chunk an empty slot is range 0 (z > 0 tests, pmask bits)
  cnt, vbits,    | match_kernel, every (tile, view) pair of [k0, k1), with or without a match (zrange: the neutral pair
  zrange         | 0xffffffff / 0 except in the wave's last view) | view_partial_kernel, pixel_count_kernel | all
  view_partial,  | view_partial_kernel (every row, every view)  | view_total_kernel | all
  zpart          |
  view_count,    | view_total_kernel | compaction (keep_words), engine read-back, integrity_verdict | all
  view_keep,     |
  n_obs,         |
  n_obs_total,   |
  range span     |
  pmask, pcount  | pixel_count_kernel: every slot of every tile, every mask word | permute / strip_levels / scatter | all
  blockhist      | pixel_count_kernel: bins 0 .. num_bins(n) - 1 of every tile | bin_scan_kernel (the same bins) | num_bins(n)
  bin_totals     | bin_scan_kernel: one per bin | permute_kernel, strip_table_kernel (t < bins) | num_bins(n)
  perm, invperm  | permute_kernel: a permutation of all n_tiles * 256 slots | strip_levels, scatter, fit_init, export_J, residual | all
  strip_meta     | strip_table_kernel (n < 255) or strip_levels_kernel + strip_offset_kernel (n >= 255) | scatter, plan, light | all
    (n >= 255: the histogram space is reused for the sorted tiles' totals and offsets: strip_levels_kernel writes every total,
    tile_offset_kernel every offset, before strip_offset_kernel reads them)
  total levels + | strip_table_kernel / tile_offset_kernel (decide_store_format) from the span view_total_kernel left | scatter, plan, every fit
  format words   | kernel | one thread, unconditionally
  comp (+ ext    | scatter_kernel: for every strip, all 64 lanes write all ceil(levels / 4) chunks (zeros past a pixel's last
  comp planes)   | observation); kStoreZ26: bits 24-25 of a short last chunk are OR-ed into words tail_bits_clear_kernel has zeroed
                 | | fit kernels through the plan | the plan lists exactly levels; the padding of a 26-bit strip is never copied
  plan, plan     | plan_kernel: the items of every strip of every wave, kAhead trailing items and one spare; count for EVERY wave
  strips, count  | | fit / batch / group kernels | plan_count (a wave without a strip reads none of its stride; batch_view reads the
                 | head of such a stride and never uses it: n_mine == 0)
import -> finalize (sucre_import_view*)
  obs            | clear_view_kernel: the RANGE plane of view k in every tile, then import_view_kernel: range, colours (and
                 | extension planes) of the listed pixels | count_view_kernel (ranges only) | z > 0: colours and extension planes
                 | of an unlisted slot are whatever was there and are never read (scatter follows pmask, exports and residuals
                 | test z > 0)
  cnt, vbits,    | count_view_kernel, every tile of view k | as above | all -- for the views that were imported: the caller imports
  zrange         | every view 0 .. n - 1 before finalising (engine.import_matches does)
fit_init -> fit (sucre_fit_init*, sucre_fit_run*, sucre_update_J*)
  state          | fit_init_kernel: J, exp_avg, exp_avg_sq of every sorted slot (NaN J where depth <= 0 or outside the image)
                 | fit kernels (J plane, moments), export_J, residual | all
  params (ws)    | fit_init_kernel (27 floats) | fit kernels, water_step | all
  ticket         | fit_init_kernel zeroes (1 + n_groups) * 16 words; arrive_last re-arms | arrive_last | all
  partials       | every workgroup of a fit launch, ten values | reduce_group (b < n_blocks) | grid = n_blocks
  gpartials      | reduce_group, every group | reduce_total (g < n_groups) | all
  sums           | reduce_total | water_step, host all-reduce | all
lws (light model / float32 colours)
  ext dense,     | as obs / comp above (match_kernel<kExt>, import_view_kernel, scatter_kernel<kExt>) | scatter, light_grad_kernel,
  ext comp (x2)  | export_view_ext, residual_kernel | cnt > 0 and z > 0, as for obs
  params, geom,  | light_init_kernel (57 floats, geometry, twists) via the staged copy in the sums area | light_grad_kernel,
  dexp           | light_step | all
  partials, sums | light_grad_kernel (19 per workgroup), light_tail_kernel | light_reduce | grid of the launch
  deal           | light_deal_kernel: count of every wave, strips [0, count) | light_grad_kernel | count
residuals (sucre_fit_residuals*), after either sequence
  scratch head   | light_geometry_kernel (light variants only) | residual_kernel<Light> | all
  scratch cells  | residual_kernel: cell (view, tile) for every kept view with cnt > 0 | residual_view_sum_kernel | the same two
                 | tests (view_keep, cnt) decide what is read; other cells are never written and never read
  count, ssr     | residual_kernel: every pixel inside the image | caller | all
  view_stats     | residual_view_sum_kernel: every view (zeros for one not kept) | caller | all
group init / iter / finish (sucre_group_*, sucre_light_group_*)
  header         | group_init_kernel: both water states, sums, tickets; light_init_kernel: parameters, geometry, twists
                 | group_iter_kernel prologue, group_finish_kernel, light_group_step_kernel | all (the light group's sums are read in
                 | the first step launch before anyone wrote them, into LDS, and not used: apply = 0)
  image table    | group_set_image_kernel / light_group_set_image_kernel, one entry per image | the iteration kernels | n_images
  partials,gpart | as in the single-image fit | | grid
batch (sucre_fit_run_batch)
  table          | batch_set_kernel, n_images entries | batch_iter_kernel, batch_tail_kernel | n_images
  (every image's partials, gpartials, sums, ticket: as in its own fit; the arrival counter is image 0's first ticket)
check_store, exports: verdict and scratch are cleared by the call itself (hipMemsetAsync); export kernels write every pixel inside
  the image.

No region is read before it is written in a way that reaches a result; the tests below hold the library to that.  (P11's group
problems have no second ``fit`` call: a group runs its iterations once.)
"""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import helpers
import test_gpu_residuals as resid
from oracle import oracle
from sucre_amd import _lib, engine, synth
from sucre_amd import dist as sdist

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FILLS = (0x00, 0xFF, 0x3F)


# ---- mechanism A: what sucre_amd.engine calls torch -----------------------------------------------------------------------------
class FilledTorch:
    """``torch`` as ``sucre_amd.engine`` sees it: ``empty`` returns device tensors filled with one byte, the rest is torch's own."""

    def __init__(self, fill):
        self.fill, self.filled = int(fill), 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.is_cuda and t.numel():
            t.view(-1).view(torch.uint8).fill_(self.fill)   # on the current stream, ahead of whatever the engine queues next
            self.filled += 1
        return t


class filled_engine:
    """``with filled_engine(0x3F):`` -- ``sucre_amd.engine``'s name ``torch`` is a ``FilledTorch`` inside the block (monkeypatch's own
    context: undone at its end; nothing else in the process sees it)."""

    def __init__(self, fill):
        self.fill = fill

    def __enter__(self):
        self.ctx = pytest.MonkeyPatch.context()
        mp = self.ctx.__enter__()
        self.wrapper = FilledTorch(self.fill)
        mp.setattr(engine, 'torch', self.wrapper)
        return self.wrapper

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


# ---- the problems -----------------------------------------------------------------------------------------------------------------
SCENES = {
    # 7 views, 5 x 4 tiles, partial in both directions; view 5 matches nothing, view 1 is dropped by min_cover = 0.7; 41 empty pixels
    's75': (lambda: synth.make_scene(75, 52, 5, seed=11, far_views=1), 0.7),
    # 71 views: two mask words, per-pixel counts up to 68
    's71': (lambda: synth.make_scene(48, 32, 70, seed=3), 1e-6),
    # 260 views: the strip_levels / tile_offset / strip_offset path of the compaction; a pixel with 260 observations, 18 with none
    's260': (lambda: synth.make_scene(48, 32, 259, seed=5, spacing=0.004), 1e-6),
    # ranges that span more than 2^24 float32 bit patterns
    'deep': (lambda: synth.make_deep_scene(96, 64, 8, seed=0), 1e-6),
}
_scene_cache: dict = {}


def scene_of(key):
    """(scene, min_cover, device views) -- made once."""
    if key not in _scene_cache:
        make, min_cover = SCENES[key]
        scene = make()
        views = engine.device_views_from_scene(scene, DEV)
        _scene_cache[key] = (scene, min_cover, views)
    return _scene_cache[key]


@dataclass(frozen=True)
class Case:
    id: str
    scene: str
    kw: tuple = ()             # Restoration keyword arguments, as items
    closed: bool = False
    T: int = 8
    source: str = 'match'      # 'match', 'import' (the oracle's lists), 'import-ext' (with the camera points as extension planes),
                               # 'import-colour' (no uint8 colours: float32 ones as extension planes)
    images: int = 1            # > 1: the scene that many times (P11)
    driver: str = 'fit'        # 'fit', 'batch' (engine.fit_batch), 'group' (engine.HipWaterGroup)


def _kw(**kw):
    return tuple(sorted(kw.items()))


CASES = [
    Case('P1-f32-param', 's75'),
    Case('P2-f32-closed', 's75', closed=True),
    Case('P3-u16mm', 's75', _kw(obs_format='u16mm')),
    Case('P4-f32plain', 's75', _kw(obs_format='f32plain')),
    Case('P4-f32z26', 's75', _kw(obs_format='f32z26')),
    Case('P5-light-param', 's75', _kw(light=True)),
    Case('P5-light-closed', 's75', _kw(light=True), closed=True),
    Case('P6-fcolour', 's75', _kw(float_colour=True)),
    Case('P6-light-fcolour', 's75', _kw(light=True, float_colour=True)),
    Case('P7-import', 's75', source='import'),
    Case('P7-import-ext', 's75', _kw(light=True), source='import-ext'),
    Case('P7-import-colour', 's75', _kw(float_colour=True), source='import-colour'),
    Case('P8-71-param', 's71'),
    Case('P8-71-closed', 's71', closed=True),
    Case('P9-260-f32', 's260', T=4),
    Case('P9-260-f32z26', 's260', _kw(obs_format='f32z26'), T=4),
    Case('P10-deep-f32', 'deep'),
    Case('P10-deep-f32z26', 'deep', _kw(obs_format='f32z26')),
    Case('P11-batch2-param', 's75', images=2, driver='batch'),
    Case('P11-batch2-closed', 's75', images=2, driver='batch', closed=True),
    Case('P11-batch3-param', 's75', images=3, driver='batch'),
    Case('P11-batch3-closed', 's75', images=3, driver='batch', closed=True),
    Case('P11-group2-param', 's75', images=2, driver='group'),
    Case('P11-group2-closed', 's75', images=2, driver='group', closed=True),
    Case('P11-lightgroup2-param', 's75', _kw(light=True), images=2, driver='group'),
    Case('P11-lightgroup2-closed', 's75', _kw(light=True), images=2, driver='group', closed=True),
]
CASE = {c.id: c for c in CASES}
# mechanism B: neighbours in this order differ in scene, view count, mode or format
ORDER = ['P1-f32-param', 'P9-260-f32z26', 'P5-light-closed', 'P8-71-param', 'P3-u16mm', 'P10-deep-f32z26', 'P11-batch3-param',
         'P6-light-fcolour', 'P9-260-f32', 'P7-import-ext', 'P2-f32-closed', 'P11-lightgroup2-param', 'P8-71-closed', 'P4-f32z26',
         'P10-deep-f32', 'P11-group2-closed', 'P6-fcolour', 'P7-import', 'P11-batch2-closed', 'P5-light-param', 'P4-f32plain',
         'P11-group2-param', 'P11-batch2-param', 'P7-import-colour', 'P11-lightgroup2-closed', 'P11-batch3-closed']
assert sorted(ORDER) == sorted(CASE)
MAX_IMAGES = max(c.images for c in CASES)


def _bytes(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _oracle_lists(scene, source):
    """The oracle's match lists of every view as ``import_matches`` takes them (tests/test_gpu_residuals.py::test_imported_store);
    'import-ext': with the camera points as a fifth element; 'import-colour': no uint8 colours, the float32 ones as the fifth."""
    lists = []
    for cover, u1, v1, cP, I in resid.scene_observations(scene):
        z = np.sqrt(cP[0] * cP[0] + cP[1] * cP[1] + cP[2] * cP[2])
        u, v, zt = torch.tensor(u1, dtype=torch.int16), torch.tensor(v1, dtype=torch.int16), torch.tensor(z)
        rgb = torch.tensor(np.rint(I.T * 255).astype(np.uint8))
        if source == 'import-ext':
            lists.append((u, v, zt, rgb, torch.tensor(np.ascontiguousarray(cP, dtype=np.float32))))
        elif source == 'import-colour':
            lists.append((u, v, zt, None, torch.tensor(np.ascontiguousarray(I, dtype=np.float32))))
        else:
            lists.append((u, v, zt, rgb))
    return lists


def store_yield(r):
    """What matching (or an import) and the finalize pass left: as bytes."""
    out = {'view_counts': _bytes(r.view_counts()), 'view_keep': _bytes(r.view_keep()), 'n_obs': _bytes(r.n_obs_device()),
           'store_format': _bytes(r.store_format())}
    planes = [r.export_view(k) for k in range(r.n_views)]
    out['export_z'] = _bytes(torch.stack([z for z, _ in planes]))
    out['export_rgb'] = _bytes(torch.stack([c for _, c in planes]))
    if r.lws is not None:
        out['export_ext'] = _bytes(torch.stack([r.export_view_ext(k) for k in range(r.n_views)]))
    out['check_store'] = _bytes(r.check_store())
    return out


def fit_yield(r, trace, tag):
    count, ssr, stats = r.residuals()
    J = r.J()
    valid = engine.count_valid(J)
    assert valid > 0
    ranks = engine.select_ranks(J, [0, valid // 100, valid // 2, valid - 1])   # (the select scratch is an uninitialised buffer too)
    return {f'{tag}/trace': _bytes(trace), f'{tag}/params': _bytes(r.params()), f'{tag}/J': _bytes(J),
            f'{tag}/res_count': _bytes(count), f'{tag}/res_ssr': _bytes(ssr), f'{tag}/res_stats': _bytes(stats),
            f'{tag}/order_statistics': _bytes(ranks)}


def run_case(case, place=None):
    """Runs one problem from allocation to the resumed fit; returns (everything it yields as {name: bytes}, its restorations).
    ``place(r, i)``: called on image i's fresh Restoration before anything is queued on it (mechanism B moves its buffers)."""
    scene, min_cover, views = scene_of(case.scene)
    kw = dict(case.kw)
    if kw.get('float_colour'):
        views = [v.as_float_colour() for v in views]
    target = views[scene.target]
    out, rs = {}, []
    for i in range(case.images):
        r = engine.Restoration(scene.height, scene.width, len(views), device=DEV, **kw)
        if place is not None:
            place(r, i)
        if case.source == 'match':
            r.match(target, views, min_cover=min_cover)
        else:
            r.import_matches(target, _oracle_lists(scene, case.source), min_cover=min_cover)
        out.update({f'image{i}/{k}': v for k, v in store_yield(r).items()})
        r.fit_init(target)
        rs.append(r)
    width = 20 if kw.get('light') else 10
    if case.driver == 'fit':
        r = rs[0]
        out.update(fit_yield(r, r.fit(case.T, use_closed_form=case.closed), 'image0/fit'))
        out.update(fit_yield(r, r.fit(3, use_closed_form=case.closed), 'image0/resumed'))
    elif case.driver == 'batch':
        for tag, T in (('fit', case.T), ('resumed', 3)):
            traces = engine.fit_batch(rs, T, use_closed_form=case.closed)
            for i, (r, t) in enumerate(zip(rs, traces)):
                out.update(fit_yield(r, t, f'image{i}/{tag}'))
    else:
        trace = torch.zeros((case.T, width), dtype=torch.float64, device=DEV)
        sdist.fit_shared_water(engine.HipWaterGroup(rs, use_closed_form=case.closed, trace=trace), case.T)
        for i, r in enumerate(rs):
            out.update(fit_yield(r, trace, f'image{i}/fit'))
    torch.cuda.synchronize()
    return out, rs


def assert_same_bits(got, want, label):
    assert sorted(got) == sorted(want), label
    differing = []
    for k in want:
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            differing.append((k, int((a != b).sum()) if a.size == b.size else 'another size', b.size))
    assert not differing, f'{label}: (name, bytes that differ, bytes) {differing}'


@pytest.fixture(scope='module')
def baseline():
    """Every problem on buffers that were all zeros (mechanism A, 0x00)."""
    runs = {}
    for case in CASES:
        with filled_engine(0x00) as w:
            runs[case.id], _ = run_case(case)
        assert w.filled > 0, 'the wrapper was not in effect'
    return runs


def _array(run, name, dtype, shape):
    return np.frombuffer(run[name], dtype=dtype).reshape(shape)


# ---- the problems are what they are said to be ------------------------------------------------------------------------------------
def test_problems_have_the_edges_they_were_chosen_for(baseline):
    scene, _, _ = scene_of('s75')
    b = baseline['P1-f32-param']
    counts, keep = _array(b, 'image0/view_counts', np.int64, -1), _array(b, 'image0/view_keep', np.int32, -1)
    assert len(counts) == 7 and counts[5] == 0 and counts[1] > 0, 'one view matches nothing'
    assert keep.tolist() == [1, 0, 1, 1, 1, 0, 1], 'one view with matches is dropped by the cover rule'
    n = _array(b, 'image0/fit/res_count', np.int32, (52, 75))
    assert (n == 0).sum() == 41 and n.max() == 5
    assert _array(b, 'image0/check_store', np.int32, -1).tolist() == [0] * 7
    n = _array(baseline['P8-71-param'], 'image0/fit/res_count', np.int32, (32, 48))
    assert n.max() == 68, 'counts beyond one 64-bit mask word'
    n = _array(baseline['P9-260-f32'], 'image0/fit/res_count', np.int32, (32, 48))
    assert n.max() == 260 and (n == 0).sum() == 18, 'more views than count bins; empty pixels'
    assert _array(baseline['P9-260-f32z26'], 'image0/store_format', np.uint32, -1)[0] == _lib.STORE_Z26
    for cid, want in (('P10-deep-f32', _lib.STORE_F32), ('P10-deep-f32z26', _lib.STORE_Z26)):
        word = _array(baseline[cid], 'image0/store_format', np.uint32, -1)
        lo, hi = int(word[2]), int(word[3])
        assert 0xfffffd < hi - lo <= 0x3fffffd, 'the deep scene spans more than 2^24 and less than 2^26 range bit patterns'
        assert int(word[0]) == want and int(word[1]) == (lo - 1 if want == _lib.STORE_Z26 else 0)
    assert _array(baseline['P3-u16mm'], 'image0/store_format', np.uint32, -1)[0] == _lib.STORE_U16MM
    assert _array(baseline['P4-f32plain'], 'image0/store_format', np.uint32, -1)[0] == _lib.STORE_F32
    assert _array(baseline['P4-f32z26'], 'image0/store_format', np.uint32, -1)[0] == _lib.STORE_Z26
    assert _array(b, 'image0/store_format', np.uint32, -1)[0] == _lib.STORE_Z24
    # imported lists and the match kernel fill the same store
    for k in ('view_counts', 'view_keep', 'n_obs', 'export_z', 'export_rgb'):
        assert baseline['P7-import'][f'image0/{k}'] == b[f'image0/{k}'], k


# ---- the anchor: the 0x00 runs against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', ['P1-f32-param', 'P2-f32-closed', 'P8-71-param', 'P8-71-closed'])
def test_zero_filled_runs_against_the_oracle(baseline, cid):
    case = CASE[cid]
    scene, min_cover, _ = scene_of(case.scene)
    H, W, T = scene.height, scene.width, case.T
    b = baseline[cid]
    per_view, samples = helpers.oracle_scene_samples(scene, min_cover)
    assert _array(b, 'image0/view_counts', np.int64, -1).tolist() == [len(m) for _, _, m in per_view]
    assert (_array(b, 'image0/view_keep', np.int32, -1) != 0).tolist() == [k for _, k, _ in per_view]
    J, tr = _array(b, 'image0/fit/J', np.float32, (H, W, 3)), _array(b, 'image0/fit/trace', np.float64, (T, 10))
    tgt = scene.views[scene.target]
    J0 = None if case.closed else oracle.init_J(tgt.rgb_u8.numpy(), tgt.depth_f32().numpy())
    Jo, po, to = oracle.fit(H, W, samples, J0, num_iter=T, use_closed_form=case.closed)
    rms, dpar = helpers.rms_per_channel(J, Jo).max(), np.abs(tr[:, 1:] - to[:, 1:]).max()
    dcost0, dcost = abs(tr[0, 0] / to[0, 0] - 1), np.abs(tr[:, 0] / to[:, 0] - 1).max()
    print(f'{cid}: rms(J) {rms:.2e}, max |d params| {dpar:.2e}, rel d cost first row {dcost0:.2e}, all rows {dcost:.2e}')
    assert np.array_equal(np.isnan(J), np.isnan(Jo))
    if cid == 'P1-f32-param':   # test_survey_of_images_reuses_one_workspace's bars
        assert rms < 1e-5
        assert dpar < 1e-5
    else:                       # test_six_hundred_views_of_a_small_image's bars
        assert rms < (1e-4 if case.closed else 1e-5)
        assert dpar < (2e-4 if case.closed else 1e-5)
        assert dcost0 < 2e-6
        assert dcost < (1e-4 if case.closed else 1e-5)


def test_zero_filled_residuals_against_the_float64_sums(baseline):
    case = CASE['P1-f32-param']
    scene, min_cover, _ = scene_of(case.scene)
    with filled_engine(0x00):
        run, (r,) = run_case(case)
        assert_same_bits(run, baseline[case.id], 'P1 run again')
        resid.check_against_reference('P1 on zero-filled buffers', r, resid.scene_observations(scene), min_cover=min_cover)


# ---- mechanism A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', FILLS[1:], ids=lambda f: f'0x{f:02X}')
@pytest.mark.parametrize('cid', [c.id for c in CASES])
def test_filled_allocations_change_no_bit(baseline, cid, fill):
    with filled_engine(fill) as w:
        run, _ = run_case(CASE[cid])
    assert w.filled > 0
    assert_same_bits(run, baseline[cid], f'{cid} on buffers filled with 0x{fill:02X}')


# ---- mechanism B ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def behind_predecessors():
    """All problems through one shared buffer per role (image i's workspace, image i's extension workspace), in ORDER and then in
    the reverse order: {(problem, direction): what it yielded}."""
    lib = _lib.load()
    ws_bytes = lws_bytes = 0
    for case in CASES:
        scene, _, views = scene_of(case.scene)
        kw = dict(case.kw)
        H, W, n = scene.height, scene.width, len(views)
        ws_bytes = max(ws_bytes, lib.sucre_workspace_bytes(H, W, n))
        if kw.get('light') or kw.get('float_colour'):
            both = kw.get('light') and kw.get('float_colour')
            lws_bytes = max(lws_bytes, lib.sucre_light_workspace_bytes_ext(H, W, n, _lib.EXT_POINTS_COLOUR) if both
                            else lib.sucre_light_workspace_bytes(H, W, n))
    assert 0 < ws_bytes < 20e6 and 0 < lws_bytes < 20e6
    shared_ws = [torch.full((ws_bytes,), 0x3F, dtype=torch.uint8, device=DEV) for _ in range(MAX_IMAGES)]
    shared_lws = [torch.full((lws_bytes,), 0x3F, dtype=torch.uint8, device=DEV) for _ in range(MAX_IMAGES)]
    assert all(t.data_ptr() % 256 == 0 for t in shared_ws + shared_lws)

    def place(r, i):
        assert r.ws.numel() <= ws_bytes
        r.ws = shared_ws[i][:r.ws.numel()]
        if r.lws is not None:
            assert r.lws.numel() <= lws_bytes
            r.lws = shared_lws[i][:r.lws.numel()]

    runs = {}
    for direction, order in (('forward', ORDER), ('reverse', ORDER[::-1])):
        for cid in order:
            runs[cid, direction], rs = run_case(CASE[cid], place)
            del rs
    return runs


@pytest.mark.parametrize('direction', ['forward', 'reverse'])
@pytest.mark.parametrize('cid', [c.id for c in CASES])
def test_a_predecessor_of_another_shape_changes_no_bit(baseline, behind_predecessors, cid, direction):
    order = ORDER if direction == 'forward' else ORDER[::-1]
    i = order.index(cid)
    before = order[i - 1] if i else ('the 0x3F fill' if direction == 'forward' else ORDER[-1])
    assert_same_bits(behind_predecessors[cid, direction], baseline[cid], f'{cid} in the bytes {before} left behind')


# ---- the pool, as the command line uses it ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('modes', [(False,) * 5, (True, False, True, False, True)], ids=['J-parameter', 'alternating'])
def test_pooled_workspace_equals_a_fresh_one_of_exactly_that_size(modes):
    """Five targets of one survey with 5, 7, 8, 6 and 5 views through ``acquire_restoration``: one workspace of capacity 8, laid out
    again for every target's own view count (and, alternating, for another J mode) -- each result is the bits a fresh
    ``Restoration`` of exactly that size gives."""
    survey = synth.make_survey(80, 48, 5, 4, seed=9)
    dev_views = engine.device_views_from_scene(survey, DEV)
    engine.release_pool()
    try:
        pooled = None
        for (idx, k), closed in zip(((6, 4), (7, 6), (13, 7), (0, 5), (19, 4)), modes):
            n = k + 1
            views = [dev_views[q] for q in survey.neighbours(idx, k)]
            assert len(views) == n
            r = engine.acquire_restoration(48, 80, n, DEV)
            assert pooled is None or r is pooled, 'one workspace serves all five targets'
            pooled = r
            assert r.capacity == 8
            got = {}
            for tag, x in (('pooled', r), ('fresh', engine.Restoration(48, 80, n, device=DEV))):
                x.match(dev_views[idx], views)
                assert x.n_views == n
                out = store_yield(x)
                x.fit_init(dev_views[idx])
                out.update(fit_yield(x, x.fit(8, use_closed_form=closed), 'fit'))
                out.update(fit_yield(x, x.fit(3, use_closed_form=closed), 'resumed'))
                got[tag] = out
            assert_same_bits(got['pooled'], got['fresh'], f'target {idx} with {n} views, {"closed form" if closed else "J-parameter"}')
    finally:
        engine.release_pool()
