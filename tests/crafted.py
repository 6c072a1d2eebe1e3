"""Observation stores built from a COUNT MAP instead of from matching, and the checks that hold a backend to them.

``synth.make_scene`` + real matching give smooth count maps: the 64 pixels of a strip have nearly equal counts, a wave of the
counting sort meets a handful of bins, ``full`` is close to ``levels``.  Here every pixel's observation set is chosen freely
(``engine.Restoration.import_matches``), so the histograms are the ones that break a plan: a strip from 1 to n_views levels, 64
distinct bins in a wave, every tail length, a class of exactly 64 m pixels, views on the mask-word boundaries, 254 / 255 / 256
views, kMaxViews.  At chosen parameters the model is exact small-integer arithmetic, so one observation lost, duplicated or
misplaced moves a result by 1/(n+1) relative instead of by rounding noise.

A *backend* is a callable ``backend(ls, params0, J0, T=0, lr=0.05, closed=False) -> Result`` that imports the list set ``ls``
and runs ``update_J`` (T = 0) or T iterations: ``oracle_backend`` (the CPU oracle, tests/test_crafted_host.py) and
``EngineBackend`` (the HIP engine, tests/test_gpu_crafted.py) run the same assertions.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import helpers  # noqa: F401  (puts the repository root on sys.path)
import model64
from oracle import oracle

M_LO, M_HI, M_NARROW = 717, 8192, 2800     # ranges are m / 1024, exact in float32, and sqrt(fl(z*z)) == z
PARAMS_A = np.array([0.1, 0, 0, 0.1, 0, 0, 0.1, 0, 0], np.float32)   # check (a): in G and B, a = 1 and y = I


# ---- the store -----------------------------------------------------------------------------------------------------------------
class Geometry:
    """What stays between rounds: which view sees which pixel at which range.  Observations are concatenated view by view,
    each view's in row-major pixel order (``off[k] .. off[k+1]``)."""

    def __init__(self, H, W, n_views, min_cover, view, px, z, cP=None):
        self.H, self.W, self.n_views, self.min_cover = int(H), int(W), int(n_views), float(min_cover)
        self.view, self.px = np.asarray(view, np.int64), np.asarray(px, np.int64)
        assert np.all(np.diff(self.view) >= 0)
        self.z = np.asarray(z, np.float32)
        self.cP = None if cP is None else np.asarray(cP, np.float32)      # (N, 3): light-model camera points, z = ||cP||
        self.counts = np.bincount(self.view, minlength=self.n_views).astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.kept = self.counts / (self.W * self.H) > self.min_cover      # sfm.py:136, applied HERE: the oracle sees kept views only
        self.u1, self.v1 = (self.px % self.W).astype(np.int16), (self.px // self.W).astype(np.int16)
        self._dev = {}
        key = self.view * (self.H * self.W) + self.px
        assert len(np.unique(key)) == len(key), 'a view sees a pixel at most once'

    @property
    def obs_kept(self):
        return self.kept[self.view]

    @property
    def n_obs(self):
        return int(self.counts[self.kept].sum())

    def count_map(self):
        """(H,W) observations per pixel over the kept views."""
        return np.bincount(self.px[self.obs_kept], minlength=self.H * self.W).reshape(self.H, self.W)

    def local(self):
        return np.arange(len(self.view)) - self.off[self.view]


@dataclass
class ListSet:
    """One round: a geometry and its colours -- uint8 (N,3), or float32 (N,3) for a float-colour store."""
    geom: Geometry
    rgb: np.ndarray | None = None
    fcol: np.ndarray | None = None

    def I(self):
        if self.fcol is not None:
            return self.fcol
        return (self.rgb.astype(np.float64) / 255.0).astype(np.float32)     # loader.py:157-163

    def samples(self, quantize=False):
        """The oracle's samples of the KEPT views: (u1, v1, cP (3,n), I (3,n)), cP = (0, 0, z) unless the geometry has points."""
        g, I, out = self.geom, self.I(), []
        for k in np.nonzero(g.kept)[0]:
            a, b = g.off[k], g.off[k + 1]
            if g.cP is not None:
                cP = np.ascontiguousarray(g.cP[a:b].T)
            else:
                cP = np.zeros((3, b - a), np.float32)
                cP[2] = g.z[a:b]
            out.append((g.u1[a:b], g.v1[a:b], cP, np.ascontiguousarray(I[a:b].T)))
        return oracle.quantize_ranges_u16mm(out) if quantize else out


def _exact_ranges(m):
    z = m.astype(np.float32) / np.float32(1024.0)
    assert np.array_equal(z.astype(np.float64) * 1024.0, m.astype(np.float64))
    assert np.array_equal(np.sqrt(z * z), z)     # the oracle's norm of (0, 0, z) is z itself (as oracle.quantize_ranges_u16mm asserts)
    return z


def build(H, W, n_views, count, view_rule='random', min_cover=1e-6, seed=0, narrow=False, small_views=(), small_n=0, light=False):
    """A store in which pixel p (row-major) is seen by ``count[p]`` views, chosen by ``view_rule``: 'random' (a seeded subset),
    'first' (views 0 .. c-1) or 'edges' (a seeded subset of the views on the 64-bit mask-word boundaries 0, 63, 64, 127, ...,
    n_views-1).  ``small_views``: views outside the rule that hold ``small_n`` seeded observations each (the views a cover rule
    drops).  ``narrow``: ranges within 0.7 .. 2.73 (fewer than 2^24 float32 bit patterns: the default store picks 24-bit codes)."""
    rng = np.random.default_rng(seed)
    count = np.asarray(count, np.int64).reshape(-1)
    npx = H * W
    assert count.shape == (npx,)
    if view_rule == 'edges':
        pool = sorted({0, n_views - 1} | {w for w in range(63, n_views, 64)} | {w for w in range(64, n_views, 64)})
    else:
        pool = [k for k in range(n_views) if k not in set(small_views)]
    pool = np.asarray(pool)
    assert count.min() >= 0 and count.max() <= len(pool), (count.max(), len(pool))
    if view_rule == 'first':
        order = np.broadcast_to(np.arange(len(pool)), (npx, len(pool)))
    else:
        order = np.argsort(np.argsort(rng.random((npx, len(pool))), axis=1), axis=1)    # a random rank per (pixel, view)
    seen = np.zeros((npx, n_views), bool)
    seen[:, pool] = order < count[:, None]
    for k in small_views:
        seen[rng.choice(npx, small_n, replace=False), k] = True
    view, px = np.nonzero(seen.T)
    hi = M_NARROW if narrow else M_HI
    m = rng.integers(M_LO, hi + 1, len(view))
    m[:2] = (M_LO, hi)                      # both ends are present: which form the store takes does not hang on the draw
    cP = None
    if light:   # camera points with x, y != 0; the range as the match kernel forms it (tests/test_gpu_parity.py::_oracle_z)
        xy = (rng.uniform(-0.5, 0.5, (len(view), 2))).astype(np.float32)
        zc = _exact_ranges(m)
        cP = np.stack([xy[:, 0], xy[:, 1], zc], axis=1)
        z = np.sqrt((cP[:, 0] * cP[:, 0] + cP[:, 1] * cP[:, 1]) + cP[:, 2] * cP[:, 2], dtype=np.float32)
    else:
        z = _exact_ranges(m)
    g = Geometry(H, W, n_views, min_cover, view, px, z, cP)
    if not small_views:
        assert np.array_equal(np.bincount(px, minlength=npx), count)
    return g


def bits(n):
    return int(n).bit_length()


def n_rounds(g):
    return max(bits(g.H * g.W - 1), bits(g.n_views))


def round_colours(g, j, seed=0):
    """Round j of check (a): G = bit j of the pixel's row-major index, B = bit j of (view index + 1), both as 0 / 255; R a seeded byte."""
    rng = np.random.default_rng(1000 * seed + j + 17)
    rgb = np.empty((len(g.view), 3), np.uint8)
    rgb[:, 0] = rng.integers(0, 256, len(g.view))
    rgb[:, 1] = 255 * ((g.px >> j) & 1)
    rgb[:, 2] = 255 * (((g.view + 1) >> j) & 1)
    return rgb


def float_colours(g, seed=0):
    """The single round of a float-colour store: G = pixel index, B = view index + 1 as float32 integers (every sum < 2^24)."""
    rng = np.random.default_rng(1000 * seed + 5)
    f = np.empty((len(g.view), 3), np.float32)
    f[:, 0] = (rng.integers(0, 256, len(g.view)).astype(np.float64) / 255.0).astype(np.float32)
    f[:, 1] = g.px
    f[:, 2] = g.view + 1
    cm = g.count_map().reshape(-1).astype(np.int64)
    assert (cm * np.arange(g.H * g.W)).max() < 2 ** 24
    sB = np.zeros(g.H * g.W)
    np.add.at(sB, g.px[g.obs_kept], (g.view + 1)[g.obs_kept])
    assert sB.max() < 2 ** 24
    return f


def random_colours(g, seed=0):
    return np.random.default_rng(1000 * seed + 3).integers(0, 256, (len(g.view), 3)).astype(np.uint8)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """``D``: the CPU oracle's distance from tests/model64.py on this case, as tests/test_crafted_host.py measures it and
    holds it within [D/4, D] -- 'R': max |J_R - J64| of check (a) over all rounds; 'J', 'par', 'cost': of the T = 3 J-parameter
    trajectory (max per-pixel |dJ|, max |d parameters|, max relative d cost); 'cJ', 'cpar', 'ccost': of the closed-form one
    (None: the case has no closed-form trajectory).  The engine's bar is ``GPU_FACTOR`` times these."""
    id: str
    n_views: int
    count: object               # (npx, rng) -> int array [npx]
    H: int = 16
    W: int = 16
    rule: str = 'random'
    min_cover: float = 1e-6
    seed: int = 1
    small_views: tuple = ()
    small_n: int = 0
    closed: bool = True         # has a closed-form trajectory in check (c)
    D: dict = field(default_factory=dict, hash=False, compare=False)

    def geometry(self, narrow=False, light=False):
        key = (self.id, bool(narrow), bool(light))
        if key not in _GEOMS:
            npx = self.H * self.W
            cnt = self.count(npx, np.random.default_rng(self.seed + 77))
            _GEOMS[key] = build(self.H, self.W, self.n_views, cnt, self.rule, self.min_cover, self.seed, narrow=narrow,
                                small_views=self.small_views, small_n=self.small_n, light=light)
        return _GEOMS[key]


_GEOMS: dict = {}
SPARSE_ROUNDS = (0, 5, 12)   # of the 13 rounds of 'maxviews', where all of them would take too long
GPU_FACTOR = 8    # the engine adds in another order and uses 1-ulp hardware exp2, reciprocal and square root


def _equal(c):
    return lambda npx, rng: np.full(npx, c)


def _classes(*pairs):
    """(count, pixels) classes, scattered over the image by a seeded permutation."""
    def f(npx, rng):
        c = np.concatenate([np.full(n, v) for v, n in pairs])
        assert len(c) == npx
        return c[rng.permutation(npx)]
    return f


def _stair(npx, rng):
    c = np.arange(npx) % 301
    c[0] = 300
    return c


def _stair9(npx, rng):
    c = np.arange(npx) % 9
    c[0] = 8
    return c


def _cycle_down(n_views):
    return lambda npx, rng: n_views - (np.arange(npx) % (n_views + 1))


def _d(R, J, par, cost, cJ=None, cpar=None, ccost=None):
    return dict(R=R, J=J, par=par, cost=cost, cJ=cJ, cpar=cpar, ccost=ccost)


CASES = [
    # every pixel the same count: the short last chunk r = 1, 2, 3, 0, 1, 0; no masked chunk
    Case('eq1', 8, _equal(1), closed=False, D=_d(5.6e-07, 6.4e-07, 5.5e-08, 1.4e-07)),
    Case('eq2', 8, _equal(2), closed=False, D=_d(5.3e-07, 6.7e-07, 4.4e-08, 2.0e-07)),
    Case('eq3', 8, _equal(3), D=_d(5.0e-07, 6.7e-07, 2.8e-08, 1.8e-07, 4.0e-07, 1.5e-07, 3.9e-08)),
    Case('eq4', 8, _equal(4), rule='first', D=_d(4.9e-07, 6.7e-07, 4.7e-08, 1.8e-07, 3.9e-07, 1.2e-07, 4.6e-08)),
    Case('eq5', 8, _equal(5), D=_d(4.3e-07, 6.7e-07, 2.8e-08, 1.4e-07, 3.9e-07, 1.3e-07, 3.4e-08)),
    Case('eq8', 8, _equal(8), D=_d(4.8e-07, 6.8e-07, 3.5e-08, 1.8e-07, 3.3e-07, 1.0e-07, 3.2e-08)),
    # 64 distinct counts in every wave, zero-count pixels, quantised bins
    Case('stair', 300, _stair, D=_d(1.4e-06, 6.6e-07, 3.3e-08, 1.9e-07, 1.1e-06, 4.1e-07, 3.7e-08)),
    # levels = 64 and full = 1 in one strip
    Case('heavy', 64, _classes((64, 1), (1, 255)), closed=False, D=_d(6.0e-07, 7.1e-07, 4.2e-08, 1.3e-07)),
    # a class of exactly 128 pixels with one pixel more in the class above / below
    Case('straddle', 8, _classes((6, 1), (5, 128), (4, 127)), D=_d(4.3e-07, 6.6e-07, 4.1e-08, 1.9e-07, 3.8e-07, 1.2e-07, 3.1e-08)),
    Case('straddle_mirror', 8, _classes((5, 128), (4, 127), (3, 1)), D=_d(4.8e-07, 6.6e-07, 2.8e-08, 1.2e-07, 3.5e-07, 9.3e-08, 3.7e-08)),
    # pixels seen only by views on the 64-bit mask-word boundaries
    Case('edges', 200, lambda npx, rng: 1 + np.arange(npx) % 8, rule='edges', closed=False, D=_d(5.6e-07, 6.7e-07, 4.0e-08, 1.2e-07)),
    # bin_of switches from identity to quantised bins at 255 views
    Case('bins254', 254, _cycle_down(254), D=_d(1.6e-06, 6.7e-07, 3.5e-08, 1.1e-07, 1.4e-06, 7.6e-07, 3.6e-08)),
    Case('bins255', 255, _cycle_down(255), rule='first', D=_d(1.5e-06, 6.6e-07, 3.0e-08, 1.3e-07, 9.2e-07, 2.6e-07, 3.4e-08)),
    Case('bins256', 256, _cycle_down(256), D=_d(1.8e-06, 6.8e-07, 4.5e-08, 1.3e-07, 1.2e-06, 6.4e-07, 3.6e-08)),
    # kMaxViews
    Case('maxviews', 4096, _classes(*[(c, 32) for c in (0, 1, 15, 16, 17, 255, 4095, 4096)]), closed=False, D=_d(6.6e-06, 7.1e-07, 3.3e-08, 2.8e-08)),
    # four views of 20 observations each are not kept (20/256 < 0.3), interleaved with the eight kept ones
    Case('dropped', 12, lambda npx, rng: rng.integers(3, 9, npx), min_cover=0.3, small_views=(1, 4, 7, 10), small_n=20,
         D=_d(4.2e-07, 6.8e-07, 4.9e-08, 8.5e-08, 3.0e-07, 8.5e-08, 3.3e-08)),
    # tiles with slots outside the image; five tiles = 20 strips
    Case('ragged40x24', 8, _stair9, H=24, W=40, D=_d(5.0e-07, 6.8e-07, 3.1e-08, 8.5e-08, 4.3e-07, 1.2e-07, 3.2e-08)),
    Case('ragged80x16', 8, _stair9, H=16, W=80, D=_d(6.2e-07, 7.0e-07, 3.5e-08, 1.2e-07, 4.4e-07, 8.6e-08, 2.9e-08)),
]
CASE = {c.id: c for c in CASES}


_PARTNERS: dict = {}


def partner_geometry(case):
    """Another store of the case's size, for a launch over two images: 'heavy' next to a 16x16 case, the stair run backwards
    (other views, other ranges) next to a ragged one."""
    if (case.H, case.W) == (16, 16):
        return CASE['heavy'].geometry()
    if case.id not in _PARTNERS:
        _PARTNERS[case.id] = build(case.H, case.W, 8, 8 - _stair9(case.H * case.W, None), seed=case.seed + 5)
    return _PARTNERS[case.id]


# ---- backends ------------------------------------------------------------------------------------------------------------------
@dataclass
class Result:
    J: np.ndarray                       # (H,W,3) float32
    trace: np.ndarray | None = None     # (T,10) float64
    n_obs: int | None = None
    view_counts: np.ndarray | None = None
    view_keep: np.ndarray | None = None
    res_count: np.ndarray | None = None  # (H,W): observations per pixel over the kept views, as the backend holds them
    store_format: int | None = None


def oracle_backend(quantize=False):
    """The CPU oracle on the list set's samples (kept views only: the cover rule is the builder's)."""
    def run(ls, params0, J0, T=0, lr=0.05, closed=False):
        g = ls.geom
        samples = ls.samples(quantize)
        if T == 0:
            return Result(J=oracle.update_J(g.H, g.W, samples, params0))
        J, _, trace = oracle.fit(g.H, g.W, samples, None if closed else J0, params0=params0, num_iter=T, lr=lr, use_closed_form=closed)
        cm = np.zeros(g.H * g.W, np.int64)
        for u, v, _, _ in samples:
            np.add.at(cm, v.astype(np.int64) * g.W + u.astype(np.int64), 1)
        return Result(J=J, trace=trace, n_obs=int(sum(len(s[0]) for s in samples)), view_counts=g.counts, view_keep=g.kept,
                      res_count=cm.reshape(g.H, g.W))
    return run


_TARGETS: dict = {}


def target_view(H, W, device='cuda'):
    """A ``synth.make_scene(W, H, 1)`` target with every depth valid, as a DeviceView."""
    import torch

    from sucre_amd import engine, synth
    if (H, W) not in _TARGETS:
        scene = synth.make_scene(W, H, 1, seed=5)
        v = scene.views[scene.target]
        d = v.depth_f32()
        d = torch.where(d > 0, d, torch.ones_like(d))
        _TARGETS[(H, W)] = engine.DeviceView(depth=d.to(device).contiguous(), rgb=v.rgb_u8.to(device).contiguous(), K=scene.K,
                                             R=v.R, t=v.t, name=v.name)
    return _TARGETS[(H, W)]


def _planes(g, arr):
    """(N,3) per-observation values as the flat float32 array in which view k's (3, n_k) block is contiguous."""
    n = g.counts[g.view]
    flat = np.empty(3 * len(g.view), np.float32)
    base, loc = 3 * g.off[g.view], g.local()
    for pl in range(3):
        flat[base + pl * n + loc] = arr[:, pl]
    return flat


def device_lists(ls, device='cuda', ext=None):
    """``import_matches`` lists of ALL views (not-kept ones included).  The geometry is uploaded once and sliced per view; only
    the colours are uploaded per round.  ``ext``: None, 'points' (light model) or 'colour' (float-colour store)."""
    import torch
    g = ls.geom
    if device not in g._dev:
        g._dev[device] = dict(u1=torch.from_numpy(g.u1).to(device), v1=torch.from_numpy(g.v1).to(device), z=torch.from_numpy(g.z).to(device),
                              cP=None if g.cP is None else torch.from_numpy(_planes(g, g.cP)).to(device))
    d = g._dev[device]
    rgb = None if ls.rgb is None else torch.from_numpy(np.ascontiguousarray(ls.rgb)).to(device)
    planes = d['cP'] if ext == 'points' else torch.from_numpy(_planes(g, ls.fcol)).to(device) if ext == 'colour' else None
    lists = []
    for k in range(g.n_views):
        a, b = int(g.off[k]), int(g.off[k + 1])
        item = (d['u1'][a:b], d['v1'][a:b], d['z'][a:b], None if rgb is None else rgb[a:b])
        if planes is not None:
            item = item + (planes[3 * a:3 * b].view(3, b - a),)
        lists.append(item)
    return lists


class EngineBackend:
    """The HIP engine through ``engine.Restoration``.  ``r``: the workspace (fresh per case in the tests); ``driver``: 'fit',
    'group' (``engine.HipWaterGroup`` of one) or 'batch' (``engine.fit_batch`` next to ``partner = (restoration, list set)``,
    at position ``slot`` of the launch)."""

    def __init__(self, r, driver='fit', partner=None, slot=0):
        self.r, self.driver, self.partner, self.slot = r, driver, partner, slot

    def _load(self, r, ls, params0, J0):
        import torch
        g = ls.geom
        tgt = target_view(g.H, g.W)
        ext = 'points' if r.light else 'colour' if r.float_colour else None
        r.import_matches(tgt, device_lists(ls, 'cuda', ext), min_cover=g.min_cover)
        r.fit_init(tgt, params0, J0=torch.from_numpy(np.ascontiguousarray(J0, np.float32)).cuda())

    def __call__(self, ls, params0, J0, T=0, lr=0.05, closed=False):
        import torch

        from sucre_amd import dist as sdist
        from sucre_amd import engine
        r = self.r
        self._load(r, ls, params0, J0)
        fmt = int(r.store_format().cpu().numpy()[0])
        if T == 0:
            r.update_J()
            torch.cuda.synchronize()
            return Result(J=r.J().cpu().numpy(), store_format=fmt)
        if self.driver == 'fit':
            trace = r.fit(T, lr=lr, use_closed_form=closed)
        elif self.driver == 'batch':
            r2, ls2 = self.partner
            self._load(r2, ls2, params0, np.zeros((ls2.geom.H, ls2.geom.W, 3), np.float32))
            rs = [r, r2] if self.slot == 0 else [r2, r]
            trace = engine.fit_batch(rs, T, lr=lr, use_closed_form=closed)[self.slot]
        else:
            trace = torch.zeros((T, 10), dtype=torch.float64, device='cuda')
            sdist.fit_shared_water(engine.HipWaterGroup([r], lr=lr, use_closed_form=closed, trace=trace, params0=params0), T)
        torch.cuda.synchronize()
        return Result(J=r.J().cpu().numpy(), trace=trace.cpu().numpy()[:, :10], n_obs=r.n_obs(), view_counts=r.view_counts().cpu().numpy(),
                      view_keep=r.view_keep().cpu().numpy().astype(bool), res_count=r.residuals()[0].cpu().numpy(), store_format=fmt)


# ---- the checks ----------------------------------------------------------------------------------------------------------------
def ulps(got, want):
    """|got - want| in float32 units in the last place of ``want`` (float64 arithmetic; want = 0 asks for exactly 0)."""
    want32 = np.asarray(want, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


_REF: dict = {}   # float64 references, computed once per (geometry, round / mode, ranges as stored)


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def check_closed_form(g, backend, bar_R, label, quantize=False, rounds=None, store_format=None):
    """Check (a): exact closed form.  Returns the largest |J_R - J64| met."""
    assert np.float32(255.0) * np.float32(1.0 / 255.0) == np.float32(1.0)    # a byte of 255 is the colour 1.0f either way
    H, W = g.H, g.W
    cm = g.count_map()
    seen = cm > 0
    zero = np.zeros((H, W, 3), np.float32)
    worst = 0.0
    for j in (range(n_rounds(g)) if rounds is None else rounds):
        ls = ListSet(g, rgb=round_colours(g, j))
        res = backend(ls, PARAMS_A, zero, T=0)
        J = res.J
        where = (label, 'round', j)
        if store_format is not None:
            assert res.store_format == store_format, (where, 'store format', res.store_format)
        nan = np.isnan(J)
        assert np.array_equal(nan.all(axis=-1), ~seen) and np.array_equal(nan.any(axis=-1), ~seen), (where, 'NaN pattern')
        bit = ((np.arange(H * W) >> j) & 1).reshape(H, W).astype(np.float32)
        bad = seen & (J[..., 1] != bit)
        if bad.any():
            p = _first(bad)
            raise AssertionError((where, 'G', 'pixel', p, 'count', int(cm[p]), 'got', float(J[p][1]), 'want', float(bit[p]), int(bad.sum()), 'pixels'))
        ok = g.obs_kept
        nB = np.zeros(H * W)
        np.add.at(nB, g.px[ok], (((g.view + 1) >> j) & 1)[ok].astype(np.float64))
        with np.errstate(invalid='ignore', divide='ignore'):
            wantB = nB.reshape(H, W) / cm
            bad = seen & ~(ulps(J[..., 2], wantB) <= 4)
        if bad.any():
            p = _first(bad)
            raise AssertionError((where, 'B', 'pixel', p, 'count', int(cm[p]), 'got', float(J[p][2]), 'want', float(wantB[p]), int(bad.sum()), 'pixels'))
        ref = _cached((id(g), 'a', j, quantize), lambda: model64.closed_form_J(H, W, ls.samples(quantize), PARAMS_A)[..., 0])
        d = np.abs(J[..., 0].astype(np.float64) - ref)
        dR = float(d[seen].max())
        worst = max(worst, dR)
        if not dR <= bar_R:
            p = _first(seen & (d == dR))
            raise AssertionError((where, 'R', 'pixel', p, 'count', int(cm[p]), 'distance', dR, 'bar', bar_R))
    return worst


def check_closed_form_float(g, backend, bar_R, label):
    """Check (a) on float32 colours: one round, the colours are the integers themselves."""
    H, W = g.H, g.W
    cm = g.count_map()
    seen = cm > 0
    ls = ListSet(g, fcol=float_colours(g))
    J = backend(ls, PARAMS_A, np.zeros((H, W, 3), np.float32), T=0).J
    nan = np.isnan(J)
    assert np.array_equal(nan.all(axis=-1), ~seen) and np.array_equal(nan.any(axis=-1), ~seen), (label, 'NaN pattern')
    ok = g.obs_kept
    sB = np.zeros(H * W)
    np.add.at(sB, g.px[ok], (g.view + 1)[ok].astype(np.float64))
    with np.errstate(invalid='ignore', divide='ignore'):
        wantB = sB.reshape(H, W) / cm
        wantG = np.arange(H * W, dtype=np.float64).reshape(H, W)
        for name, c, want in (('G', 1, wantG), ('B', 2, wantB)):
            bad = seen & ~(ulps(J[..., c], want) <= 4)
            if bad.any():
                p = _first(bad)
                raise AssertionError((label, name, 'pixel', p, 'count', int(cm[p]), 'got', float(J[p][c]), 'want', float(want[p]), int(bad.sum()), 'pixels'))
    ref = _cached((id(g), 'af'), lambda: model64.closed_form_J(H, W, ls.samples(), PARAMS_A)[..., 0])
    dR = float(np.abs(J[..., 0].astype(np.float64) - ref)[seen].max())
    assert dR <= bar_R, (label, 'R', dR, bar_R)
    return dR


def check_cost(g, backend, label):
    """Check (b): exact cost.  All parameters 0, J = 0, R = 255 and G = B = 0, lr = 0, one iteration: every residual is 1, 0, 0."""
    H, W = g.H, g.W
    rgb = np.zeros((len(g.view), 3), np.uint8)
    rgb[:, 0] = 255
    res = backend(ListSet(g, rgb=rgb), np.zeros(9, np.float32), np.zeros((H, W, 3), np.float32), T=1, lr=0.0)
    assert res.trace.shape == (1, 10)
    assert res.trace[0, 0] == g.n_obs, (label, 'cost', res.trace[0, 0], 'observations', g.n_obs)
    assert not res.trace[0, 1:].any(), (label, 'parameters moved at lr = 0', res.trace[0, 1:])
    assert not np.ascontiguousarray(res.J).view(np.uint32).any(), (label, 'J moved at lr = 0')
    assert res.n_obs == g.n_obs, (label, 'n_obs', res.n_obs, g.n_obs)
    assert np.array_equal(np.asarray(res.view_counts), g.counts), (label, 'view_counts')
    assert np.array_equal(np.asarray(res.view_keep).astype(bool), g.kept), (label, 'view_keep')
    bad = res.res_count != g.count_map()
    assert not bad.any(), (label, 'count map', 'pixel', _first(bad), int(res.res_count[_first(bad)]), int(g.count_map()[_first(bad)]))


def trajectory(g, backend, label, closed=False, quantize=False):
    """Check (c), measured: T = 3 from a seeded random J0, parameters 0.1, random colours -- against tests/model64.py.  Returns
    (max |J - J64| over the pixels with observations, max |d parameters|, max relative d cost); pixels without observations
    keep J0 bit for bit (J-parameter mode) or are NaN (closed form)."""
    H, W = g.H, g.W
    seen = g.count_map() > 0
    # J0 in [3, 4): J0 e^(-beta z) >= 3 e^(-0.8) > 1 >= I, so every residual is negative and every gradient a sum of terms of ONE
    # sign.  With J0 in [0, 1) a pixel's gradient cancels to |g| ~ eps now and then (1 in 10^4 pixel-channels), where Adam's
    # step lr g / (|g| + eps) is decided by float32 rounding: the float32 oracle itself then lies 1e-4 from float64 on that
    # pixel (measured on 'dropped'), and no bar below that can be held by anyone.
    J0 = (3.0 + np.random.default_rng(11).random((H, W, 3))).astype(np.float32)
    p0 = np.full(9, 0.1, np.float32)
    ls = ListSet(g, rgb=random_colours(g))
    res = backend(ls, p0, J0, T=3, lr=0.05, closed=closed)
    J64, _, t64 = _cached((id(g), 'c', closed, quantize), lambda: model64.adam_fit(H, W, ls.samples(quantize), J0, p0, 3, use_closed_form=closed))
    J = res.J
    if closed:
        nan = np.isnan(J)
        assert np.array_equal(nan.all(axis=-1), ~seen) and np.array_equal(nan.any(axis=-1), ~seen), (label, 'NaN pattern')
    else:
        assert not np.isnan(J).any(), label
        assert np.array_equal(J[~seen].view(np.uint32), J0[~seen].view(np.uint32)), (label, 'a pixel without observations moved')
    dJ = float(np.abs(J.astype(np.float64) - J64)[seen].max())
    dpar = float(np.abs(res.trace[:, 1:] - t64[:, 1:]).max())
    dcost = float(np.abs(res.trace[:, 0] / t64[:, 0] - 1).max())
    return dJ, dpar, dcost


def check_trajectory(g, backend, D, label, closed=False, quantize=False, factor=1):
    """Check (c) at ``factor`` times the case's D."""
    got = trajectory(g, backend, label, closed, quantize)
    keys = ('cJ', 'cpar', 'ccost') if closed else ('J', 'par', 'cost')
    for name, x, k in zip(('J', 'parameters', 'cost'), got, keys):
        assert x <= factor * D[k], (label, 'closed form' if closed else 'J-parameter', name, x, 'bar', factor * D[k])
    return got


HOST_VARIANTS = (('wide', False, False), ('narrow', True, False), ('u16mm', False, True))   # (name, narrow ranges, ranges as uint16 mm)


def measure(case, make_backend, variants=HOST_VARIANTS):
    """Checks (a) and (c) on every variant of the case's ranges with ``make_backend(quantize)``: the identities are asserted, the
    distances from tests/model64.py are returned as {key of Case.D: largest over the variants}."""
    m = dict(R=0.0, J=0.0, par=0.0, cost=0.0)
    if case.closed:
        m.update(cJ=0.0, cpar=0.0, ccost=0.0)
    for i, (name, narrow, quantize) in enumerate(variants):
        g, be, label = case.geometry(narrow), make_backend(quantize), (case.id, name)
        rounds = SPARSE_ROUNDS if i > 0 and g.n_views > 1000 else None     # (kMaxViews: every round once is enough on the CPU)
        m['R'] = max(m['R'], check_closed_form(g, be, np.inf, label, quantize=quantize, rounds=rounds))
        for closed, keys in ((False, ('J', 'par', 'cost')), (True, ('cJ', 'cpar', 'ccost'))):
            if closed and not case.closed:
                continue
            for k, x in zip(keys, trajectory(g, be, label, closed, quantize)):
                m[k] = max(m[k], x)
    return m


# ---- mutations: what the checks must catch -------------------------------------------------------------------------------------
def _rebuild(g, keep=None, px=None, z=None):
    keep = np.ones(len(g.view), bool) if keep is None else keep
    return Geometry(g.H, g.W, g.n_views, g.min_cover, g.view[keep], (g.px if px is None else px)[keep], (g.z if z is None else z)[keep])


def _pick_busy(g, rng):
    """An observation of a kept view."""
    return int(rng.choice(np.nonzero(g.obs_kept)[0]))


def mutate(g, kind, seed=0):
    """(geometry, colour map): the list set a backend gets instead of the true one.  ``colour map`` turns the true round's
    (N,3) colours into the mutated store's."""
    rng = np.random.default_rng(seed + 101)
    N = len(g.view)
    same = lambda c: c
    if kind == 'drop':               # one observation lost
        keep = np.ones(N, bool)
        keep[_pick_busy(g, rng)] = False
        return _rebuild(g, keep=keep), (lambda c: c[keep])
    if kind == 'move':               # one observation lands on the neighbouring pixel (one the view does not see yet)
        taken = set((g.view * g.H * g.W + g.px).tolist())
        for i in rng.permutation(np.nonzero(g.obs_kept)[0]):
            q = g.px[i] + 1 if g.px[i] + 1 < g.H * g.W else g.px[i] - 1
            if int(g.view[i] * g.H * g.W + q) not in taken:
                px = g.px.copy()
                px[i] = q
                order = np.lexsort((px, g.view))     # views stay in pixel order
                return Geometry(g.H, g.W, g.n_views, g.min_cover, g.view[order], px[order], g.z[order]), (lambda c: c[order])
        raise AssertionError('no observation can move')
    if kind == 'swap_colours':       # two observations of different pixels carry each other's colours
        i = _pick_busy(g, rng)
        j = int(rng.choice(np.nonzero(g.obs_kept & (g.px != g.px[i]))[0]))

        def swap(c):
            c = c.copy()
            c[[i, j]] = c[[j, i]]
            return c
        return g, swap
    if kind == 'swap_ranges':        # two observations of ONE pixel carry each other's ranges (the two furthest apart)
        cm = g.count_map().reshape(-1)
        p = int(rng.choice(np.nonzero(cm >= 2)[0]))
        idx = np.nonzero(g.obs_kept & (g.px == p))[0]
        i, j = idx[np.argmin(g.z[idx])], idx[np.argmax(g.z[idx])]
        assert g.z[i] != g.z[j]
        z = g.z.copy()
        z[[i, j]] = z[[j, i]]
        return _rebuild(g, z=z), same
    raise ValueError(kind)


MUTATIONS = ('drop', 'move', 'swap_colours', 'swap_ranges')


def mutated(backend, g, kind):
    """``backend`` fed the mutated store whenever it is handed a list set of ``g``."""
    g2, cmap = mutate(g, kind)

    def run(ls, *a, **kw):
        assert ls.geom is g
        return backend(ListSet(g2, rgb=None if ls.rgb is None else cmap(ls.rgb), fcol=None if ls.fcol is None else cmap(ls.fcol)), *a, **kw)
    return run
