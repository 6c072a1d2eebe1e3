"""SUCRe restoration: model, optimiser loop, per-image pipeline and command line.

Drop-in for the reference's ``sucre.py`` (sucre.py:35-307): ``SUCRe``, ``adam``, ``restore_image``, ``parse_args``
and the argparse CLI keep their names, arguments, defaults, printed stages and output files
(``<stem>_rgb.png``, ``<stem>_reconstruction.png``, ``<name>.pt`` with keys ``B, beta, gamma, J``).  The 200
full-batch Adam iterations of ``adam`` (sucre.py:138-148) run as 200 back-to-back launches of one fused HIP
kernel over observations that never leave HBM, with no host synchronisation until the trace is read.

    python -m sucre_amd.sucre --image-dir IMAGES --depth-dir DEPTHS --model-dir COLMAP --output-dir OUT \\
        --image-name NAME [...]        # same flags as the reference, see --help

Under ``torchrun`` (WORLD_SIZE > 1) the images to restore are sharded over the ranks, one GPU each.
"""
from __future__ import annotations

import argparse
import collections
import dataclasses
import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch
from PIL import Image as PILImage
from torch import Tensor

from . import _pixelio, dist as sdist
from . import loader, se3, sfm


class SUCRe(torch.nn.Module):
    """Image-formation model ``I = l * (J exp(-beta z) + B (1 - exp(-gamma z)))`` of one image (sucre.py:35-82).

    Parameters ``B, beta, gamma`` are (3,1), initialised to 0.1; ``J`` is an (H,W,3) parameter initialised to the
    image itself with NaN where the depth map is invalid, or -- with ``use_closed_form`` -- a plain attribute
    recomputed from the observations."""

    stretch = None   # None: plot_J stretches every image by its own percentiles (the reference); (lo, hi): a fixed stretch

    def __init__(self, image: sfm.Image, light_model: bool = False, use_closed_form: bool = False,
                 _J_by_engine: bool = False):
        """``_J_by_engine`` (engine-internal): leave ``J`` uninitialised on the device -- the fit's first kernel
        (``sucre_fit_init``) writes the very same start values, ``float32(float64(k)/255)`` with NaN where the depth is
        invalid, and ``adam`` copies the fitted J back; saves the pipeline five torch launches and a host wait per image."""
        super().__init__()
        self.image = image
        self.light_model = light_model
        self.use_closed_form = use_closed_form
        self.B = torch.nn.Parameter(torch.full((3, 1), 0.1))
        self.beta = torch.nn.Parameter(torch.full((3, 1), 0.1))
        self.gamma = torch.nn.Parameter(torch.full((3, 1), 0.1))
        if light_model:  # light pose (twist, light-from-camera) and the 2x2 factor of the beam-shape matrix
            self.cam2light = torch.nn.Parameter(torch.zeros(6))
            self.sigma = torch.nn.Parameter(torch.eye(2))
        if not use_closed_form:
            cached = getattr(image, '_device_view', None)
            if _J_by_engine and cached is not None and cached[0].type == 'cuda':
                J = torch.empty(cached[1].rgb.shape, dtype=torch.float32, device=cached[1].rgb.device)
                self._J_unset = True
            elif cached is not None and cached[0].type == 'cuda':
                # the pixels are already resident for the engine: same values as get_rgb() / get_depth_map()
                # (float32(float64(k)/255), loader.py:157-163) without decoding the files a second time
                view = cached[1]
                J = view.rgb.clone() if view.rgb.dtype == torch.float32 else (view.rgb.to(torch.float64) / 255).to(torch.float32)
                J[view.depth <= 0] = torch.nan
            else:
                J = image.get_rgb()
                J[image.get_depth_map() <= 0] = torch.nan
            self.J = torch.nn.Parameter(J)

    # -- model evaluation (output stage / compatibility; the fit itself runs in the HIP engine) -------------------
    def compute_l_z(self, cP: Tensor) -> tuple[float | Tensor, Tensor]:
        """Illumination factor l and total light path z of camera-frame points (3, n) (sucre.py:52-64)."""
        z = cP.norm(dim=0)
        if not self.light_model:
            return 1.0, z
        R, t = se3.exp(self.cam2light)
        lP = R @ cP + t                                   # points in the light's frame
        lp = lP[:2] / lP[2]                               # (2, n) direction from the light axis
        Minv = (self.sigma.T @ self.sigma).inverse()
        q = (lp * (Minv @ lp)).sum(dim=0)                 # lp^T Sigma^-1 lp per point
        return torch.exp(-q / 2), z + lP.norm(dim=0)

    @torch.no_grad()
    def update_J(self, matches_data: loader.MatchesData, force_update: bool = False):
        """Closed-form J from the current water parameters (sucre.py:66-77), computed by the engine."""
        if not (self.use_closed_form or force_update):
            return
        resto = _restoration_of(matches_data, self)
        resto.params().copy_(self.water_vector().to(resto.device))
        resto.update_J()
        self.J = resto.J().to(self.B.device)

    @torch.no_grad()
    def invert(self) -> 'SUCRe':
        """Single-view ``update_J``: J from the module's OWN image -- its depth map and colours, no matches -- at the module's
        current parameters (``engine.invert_images``; sucre.py:66-77 with the image as its only observation).  Sets the
        attribute of a closed-form model, copies into the parameter of a J-parameter one.  Reads the parameters to the host
        (one small device-to-host copy)."""
        from . import engine
        dev = self.B.device
        if dev.type != 'cuda':
            raise RuntimeError('invert runs on the GPU engine: move the model to a cuda device (SUCRe(...).to("cuda"))')
        J = engine.invert_images([self.image.device_view(dev)], self.water_vector().cpu(), light=self.light_model)[0]
        if self.use_closed_form:
            self.J = J
        else:
            self.J.copy_(J)
            self._J_unset = False
        return self

    @torch.no_grad()
    def residuals(self, matches_data: loader.MatchesData):
        """Per-pixel and per-view residuals of this model on ``matches_data`` (``engine.Restoration.residuals``): the
        module's water (and light) parameters go to the engine first, as in ``update_J``; J is the engine's own.  Returns
        the device tensors ``(count, ssr, view_stats)``; the Adam state and the step count are left alone."""
        resto = _restoration_of(matches_data, self)
        resto.params().copy_(self.water_vector().to(resto.device))
        return resto.residuals()

    def forward(self, u: Tensor, v: Tensor, cP: Tensor) -> Tensor:
        l, z = self.compute_l_z(cP)
        direct = self.J[v, u].T * torch.exp(-self.beta * z)
        veil = self.B * (1 - torch.exp(-self.gamma * z))
        return l * (direct + veil)

    def water_vector(self) -> Tensor:
        """B, beta, gamma (+ cam2light, sigma with the light model) flattened to the floats the engine stores."""
        parts = [self.B, self.beta, self.gamma] + ([self.cam2light, self.sigma] if self.light_model else [])
        return torch.cat([p.detach().flatten() for p in parts]).float()

    # -- output stage (sucre.py:84-121) -----------------------------------------------------------------------------
    @torch.no_grad()
    def plot_J(self) -> PILImage.Image:
        """Restored image: per-channel 1-99 percentile stretch of the valid pixels, invalid pixels black.  With
        ``self.stretch = (lo, hi)`` set (--common-stretch, --stretch-from) the percentiles, the minimum and the maximum of the
        image are replaced by the given numbers: ``uint8(((min(max(J, lo), hi) - lo) / (hi - lo)) * 255)`` in float32, the same
        for every image that shares the stretch."""
        if self.stretch is not None:
            lo, hi = self.stretch
            if self.J.is_cuda:
                from . import engine
                return PILImage.fromarray(engine.plot_stretch(self.J.detach().contiguous(), lo, hi).cpu().numpy())
            return PILImage.fromarray(stretch_picture(self.J.detach().cpu().numpy(), lo, hi))
        if self.J.is_cuda and _NUMPY_2:
            return PILImage.fromarray(self._plot_J_device().cpu().numpy())
        J = self.J.detach().cpu().numpy().copy()
        ok = ~np.isnan(J).any(axis=2)
        vals = J[ok]
        lo, hi = np.percentile(vals, 1, axis=0), np.percentile(vals, 99, axis=0)
        vals = np.clip(vals, lo, hi)
        vals = vals - vals.min(axis=0)
        vals = vals / vals.max(axis=0)
        J[~ok] = 0.0
        J[ok] = vals
        return PILImage.fromarray(np.uint8(J * 255))

    def _plot_J_device(self) -> Tensor:
        """The same stretch with J left on the GPU (uint8 (H,W,3) out).  The two percentiles of every channel are
        numpy's linear interpolation between two order statistics of the valid pixels: the engine finds those four
        values per channel by radix select on the device (``sucre_select_ranks``), the ranks and the interpolation
        are numpy's own float32 arithmetic (``percentile_plan`` / ``percentile_lerp``), so the percentiles are the
        very numbers ``np.percentile`` returns for the whole array.  After the clip the minimum is the lower
        percentile itself and the maximum of the shifted values the float32 difference of the two, so what remains is
        one elementwise pass of IEEE-exact operations (``sucre_plot_stretch``): the same bits as the host path."""
        return _plot_J_on_device(self.J.detach().contiguous())

    @torch.no_grad()
    def plot_reconstruction(self) -> PILImage.Image:
        """The image as the fitted model re-synthesises it from J and the depth map."""
        dev = self.B.device
        u, v, cP = self.image.unproject_depth_map(self._depth_on(dev), to_world=False)
        out = torch.zeros((self.image.camera.height, self.image.camera.width, 3), device=dev)
        out[v, u] = self(u=u, v=v, cP=cP).clip(0, 1).T
        if out.is_cuda:   # the float32 product and the truncating cast are the same IEEE operations on either side
            return PILImage.fromarray((out * 255).to(torch.uint8).cpu().numpy())
        return PILImage.fromarray(np.uint8(out.cpu().numpy() * 255))

    @torch.no_grad()
    def plot_l(self) -> PILImage.Image:
        """Illumination factor over the image, jet colour map (sucre.py:96-104)."""
        import matplotlib.pyplot as plt
        dev = self.cam2light.device
        u, v, cP = self.image.unproject_depth_map(self._depth_on(dev), to_world=False)
        l, _ = self.compute_l_z(cP)
        lmap = torch.zeros((self.image.camera.height, self.image.camera.width), device=dev)
        lmap[v, u] = l
        return PILImage.fromarray(np.uint8(plt.colormaps['jet'](lmap.cpu().numpy())[:, :, :3] * 255))

    def _depth_on(self, dev) -> Tensor:
        """The target's depth map on ``dev``: the copy already resident for the engine when there is one (same
        values as ``get_depth_map``), else decoded from the file like the reference does."""
        if dev.type == 'cuda' and hasattr(self.image, 'device_view'):
            return self.image.device_view(dev).depth
        return self.image.get_depth_map().to(dev)

    def save_plots(self, save_dir: Path, iteration: int | None = None):
        stem = Path(self.image.name).stem
        tag = '' if iteration is None else f'_{iteration:04d}'
        _save_png(self.plot_J(), Path(save_dir) / f'{stem}_rgb{tag}.png')
        _save_png(self.plot_reconstruction(), Path(save_dir) / f'{stem}_reconstruction{tag}.png')
        if self.light_model:
            _save_png(self.plot_l(), Path(save_dir) / f'{stem}_vignetting{tag}.png')


def _plot_J_on_device(J: Tensor) -> Tensor:
    """``SUCRe._plot_J_device`` of any (H,W,3) float32 contiguous device image (a restored image, a mosaic of them)."""
    from . import engine
    n = engine.count_valid(J)
    if n == 0:
        return torch.zeros(J.shape, dtype=torch.uint8, device=J.device)   # (numpy raises on an empty percentile)
    plan = [percentile_plan(n, q) for q in (1, 99)]
    stats = engine.select_ranks(J, [plan[0][0], plan[0][1], plan[1][0], plan[1][1]]).cpu().numpy()   # (3, 4)
    lo = np.array([percentile_lerp(stats[c, 0], stats[c, 1], plan[0][2]) for c in range(3)], np.float32)
    hi = np.array([percentile_lerp(stats[c, 2], stats[c, 3], plan[1][2]) for c in range(3)], np.float32)
    return engine.plot_stretch(J, lo, hi)


def _save_png(img: PILImage.Image, path: Path) -> None:
    """Writes ``img`` as a PNG holding exactly its pixels.  PNG is lossless, so only the encoding effort is a choice:
    8-bit RGB images go through ``_pixelio.encode_rgb`` (Sub-filtered rows, one zlib stream at SUCRE_PNG_COMPRESS_LEVEL,
    default 1: 2.5-4x faster than PIL's encoder at the same level), in a worker process when the CLI has started some;
    anything else, or SUCRE_PNG_WRITER=pil, is saved by PIL (level 6 is PIL's default and what the reference writes)."""
    from . import _pixelio
    level = _pixelio.default_level()
    if img.mode != 'RGB' or os.environ.get('SUCRE_PNG_WRITER', 'zlib') == 'pil':
        img.save(path, compress_level=level)
    else:
        pool = _pixelio.POOL
        if pool is not None:
            try:
                pool.write(path, np.asarray(img), level)
                return
            except _pixelio.WorkerLost as e:
                print(f'warning: {e}; writing {path} in-process')
        _pixelio.write_rgb(str(path), np.asarray(img), level)


# percentile_plan / percentile_lerp restate numpy >= 2, where the quantile, the virtual index and the interpolation of a
# float32 array stay float32.  numpy 1.x runs np.percentile in float64 (and promotes the clipped image): there plot_J takes
# the host path, which calls np.percentile itself, so the picture equals the reference's on the same install either way.
_NUMPY_2 = int(np.__version__.split('.')[0]) >= 2


def percentile_plan(n: int, q: float) -> tuple[int, int, np.floating]:
    """(rank below, rank above, weight) of ``np.percentile(a, q)`` (method 'linear') for a float32 array of ``n``
    values, in numpy's own arithmetic: the quantile ``q / 100`` and the virtual index ``(n - 1) q'`` are formed in
    the array's dtype, float32 (numpy/lib/_function_base_impl.py: percentile, _QuantileMethods['linear'],
    _get_indexes, _get_gamma)."""
    quant = np.asanyarray(np.true_divide(q, np.float32(100)))
    virtual = np.asanyarray((n - 1) * quant)
    below = np.floor(virtual)
    above = below + 1
    if virtual >= n - 1:
        below = above = np.float32(n - 1)
    if virtual < 0:
        below = above = np.float32(0)
    gamma = np.asanyarray(virtual - below, dtype=virtual.dtype)
    return int(below), int(above), gamma[()]


def percentile_lerp(a, b, t):
    """numpy's ``_lerp``: ``a + (b - a) t``, formed from the upper end when ``t >= 0.5``."""
    a, b = np.float32(a), np.float32(b)
    diff = np.subtract(b, a)
    out = np.add(a, diff * t)
    if t >= 0.5:
        out = np.subtract(b, diff * (1 - t))
    return out


def percentile_plan64(n: int, q: float) -> tuple[int, int, float]:
    """(rank below, rank above, weight) of ``np.percentile(a.astype(np.float64), q)`` (method 'linear') for ``n`` values, in
    float64: ``virtual = (n - 1) (q / 100)``, ``below = floor(virtual)``, ``above = min(below + 1, n - 1)``, ``t = virtual -
    below``.  The plan of a POOL of images (``engine.pooled_percentiles``): a pool passes 2^24 pixels with nine 1080p images,
    where the float32 index arithmetic of ``percentile_plan`` -- numpy's own for a float32 array, kept for the per-image path
    that mirrors the reference -- would round the ranks."""
    n = int(n)
    if n < 1:
        raise ValueError(f'percentile_plan64: n must be >= 1, not {n}')
    q = float(q)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f'percentile_plan64: q must lie in [0, 100], not {q}')
    virtual = float(n - 1) * (q / 100.0)
    below = int(np.floor(virtual))
    if below >= n - 1:
        return n - 1, n - 1, 0.0
    return below, below + 1, virtual - below


def stretch_picture(J: np.ndarray, lo, hi) -> np.ndarray:
    """(H,W,3) uint8: the fixed stretch of a host image, ``uint8(((min(max(J, lo), hi) - lo) / (hi - lo)) * 255)`` in float32,
    invalid pixels (a NaN in any channel) black -- ``plot_J`` with the per-image percentiles, minimum and maximum replaced by
    ``lo``, ``lo`` and ``hi - lo``; the arithmetic of ``sucre_plot_stretch``."""
    J = np.asarray(J, np.float32)
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    ok = ~np.isnan(J).any(axis=2)
    out = np.zeros(J.shape, np.uint8)
    vals = np.minimum(np.maximum(J[ok], lo), hi)
    out[ok] = (((vals - lo) / (hi - lo)) * np.float32(255)).astype(np.uint8)
    return out


def check_stretch(obj, where: str = 'stretch') -> tuple[np.ndarray, np.ndarray]:
    """``(lo, hi)``, two (3,) float32 arrays, of a mapping such as a loaded ``stretch.pt`` (tensors or arrays of any float dtype;
    other keys are ignored) or of a ``(lo, hi)`` pair.  A stretch is usable only if all six numbers are finite and ``hi > lo``
    in every channel: ``ValueError`` naming the key or the channel that is missing, mis-shaped, non-finite or non-increasing."""
    if hasattr(obj, 'keys'):
        for key in ('lo', 'hi'):
            if key not in obj:
                raise ValueError(f"{where} holds no '{key}'")
        pair = {'lo': obj['lo'], 'hi': obj['hi']}
    else:
        try:
            lo, hi = obj
        except (TypeError, ValueError):
            raise ValueError(f"{where} holds no stretch (a mapping with the keys lo, hi or a (lo, hi) pair is expected)") from None
        pair = {'lo': lo, 'hi': hi}
    out = {}
    for key, v in pair.items():
        if torch.is_tensor(v):
            v = v.detach().cpu().numpy()
        v = np.asarray(v)
        if v.shape != (3,) or v.dtype.kind != 'f':
            raise ValueError(f"'{key}' in {where} is {v.dtype} {v.shape}, expected three floats, shape (3,)")
        out[key] = v.astype(np.float32)
    for c, name in enumerate('RGB'):
        l, h = out['lo'][c], out['hi'][c]
        if not np.isfinite(l):
            raise ValueError(f"'lo' in {where} is not finite in channel {name} ({l})")
        if not np.isfinite(h):
            raise ValueError(f"'hi' in {where} is not finite in channel {name} ({h})")
        if not h > l:
            raise ValueError(f"{where}: hi must exceed lo in every channel, but channel {name} has lo {l} and hi {h}")
    return out['lo'], out['hi']


def read_stretch_file(path: Path) -> tuple[np.ndarray, np.ndarray]:
    """``check_stretch`` of a ``.pt`` file, for the command line: ``SystemExit`` naming the file and the key or channel."""
    try:
        data = torch.load(path, map_location='cpu')
    except Exception as e:
        raise SystemExit(f'--stretch-from: cannot read {path}: {e}')
    try:
        return check_stretch(data, where=str(path))
    except ValueError as e:
        raise SystemExit(f'--stretch-from: {e}')


def common_stretch(Js: list, q=(1, 99), group=None) -> tuple[np.ndarray, np.ndarray, int]:
    """``(lo, hi, n)``: the per-channel ``q[0]``-th and ``q[1]``-th percentile, (3,) float32 each, of the POOL of the valid
    pixels of the device images ``Js`` of all ranks of ``group`` (``engine.pooled_percentiles``), and the pooled number of valid
    pixels.  ``ValueError`` when the pool is empty or the two do not make a stretch (``check_stretch``)."""
    from . import engine
    P, n = engine.pooled_percentiles(Js, q=(float(q[0]), float(q[1])), group=group)
    lo, hi = check_stretch((P[:, 0].copy(), P[:, 1].copy()), where=f'the common stretch over {n} valid pixels')
    return lo, hi, n


def _restoration_of(matches_data: loader.MatchesData, sucre: 'SUCRe | None' = None):
    """The engine workspace behind ``matches_data``: the one ``Image.match_images`` filled, or -- for a container built
    with ``append`` like the reference's ``load_matches`` does (loader.py:103-118) -- one the samples are imported
    into on first use.  There is no CPU path for the fit."""
    resto = getattr(matches_data, 'restoration', None)
    if resto is None and sucre is not None and getattr(matches_data, 'data', None):
        dev = sucre.B.device
        if dev.type != 'cuda':
            raise RuntimeError('the fit runs on the GPU engine: move the model to a cuda device (SUCRe(...).to("cuda"))')
        resto = matches_data.to_engine(sucre.image.camera.height, sucre.image.camera.width, dev, light=sucre.light_model)
    if resto is None:
        raise RuntimeError('this MatchesData holds no observations the engine can use (build it with Image.match_images + '
                           'MatchesFile.load_matches, or append samples to it); there is no CPU fallback for the fit')
    return resto


def _pull_results(sucre: SUCRe, resto) -> None:
    p = resto.params().to(sucre.B.device)
    with torch.no_grad():
        sucre.B.copy_(p[0:3].view(3, 1))
        sucre.beta.copy_(p[3:6].view(3, 1))
        sucre.gamma.copy_(p[6:9].view(3, 1))
        if sucre.light_model:
            sucre.cam2light.copy_(p[9:15])
            sucre.sigma.copy_(p[15:19].view(2, 2))
        J = resto.J().to(sucre.B.device)
        if sucre.use_closed_form:
            sucre.J = J
        else:
            sucre.J.copy_(J)
            sucre._J_unset = False


def _format_trace(trace: np.ndarray, first_iteration: int) -> str:
    """The per-iteration lines of sucre.py:149-152."""
    with np.printoptions(precision=4):
        return '\n'.join(f'iter: {first_iteration + i:04d}, cost: {row[0]:.4e}, B: {row[1:4].astype(np.float32)}, '
                         f'beta: {row[4:7].astype(np.float32)}, gamma: {row[7:10].astype(np.float32)}'
                         for i, row in enumerate(trace))


def _log_trace(trace: np.ndarray, first_iteration: int) -> None:
    print(_format_trace(trace, first_iteration))


def snapshot_stops(num_iter: int, save_interval: int | None) -> list[tuple[int, bool]]:
    """Where ``adam`` cuts its ``num_iter`` iterations into engine calls: ``(stop, snapshot)`` pairs in ascending order, a call
    running the iterations from the previous stop (0 at first) up to ``stop``, exclusive, and ``snapshot`` telling whether the
    plots are saved behind it.  The reference saves them after iteration i when ``i % save_interval == 0`` (sucre.py:153), so
    every such i < num_iter ends a call (stop = i + 1); the last pair always ends at ``num_iter``.  ``save_interval`` None: one
    call, no snapshot."""
    if save_interval is None:
        return [(num_iter, False)]
    stops = sorted({k + 1 for k in range(0, num_iter, save_interval)} | {num_iter})
    return [(stop, stop >= 1 and (stop - 1) % save_interval == 0) for stop in stops]


@dataclasses.dataclass(frozen=True)
class _Extras:
    """What a restoration can be asked for beyond the reference's arguments: --save-quality; --trim-outliers, --trim-rounds;
    --view-gains, --gain-rounds, --gain-limit; the ``(lo, hi)`` of --stretch-from; --save-uncertainty.  Built from the command line (``_run_request``),
    from the keywords of ``restore_images`` and from those of ``adam``; everything between them hands the record on."""
    save_quality: bool = False
    trim_outliers: float = None
    trim_rounds: int = 1
    view_gains: bool = False
    gain_rounds: int = 1
    gain_limit: float = 2.0
    stretch: tuple = None
    save_uncertainty: bool = False

    def checked(self, save_interval: int = None) -> '_Extras':
        """The record with its stretch as ``check_stretch`` returns it.  ``ValueError`` for a value out of range, for gains next
        to a trim and for either next to ``save_interval`` snapshots."""
        stretch = None if self.stretch is None else check_stretch(self.stretch)
        if self.trim_outliers is not None:
            if not (np.isfinite(float(self.trim_outliers)) and float(self.trim_outliers) > 0):
                raise ValueError(f'trim_outliers must be a finite multiple > 0, not {self.trim_outliers!r}')
            if int(self.trim_rounds) < 1:
                raise ValueError(f'trim_rounds must be >= 1, not {self.trim_rounds!r}')
        if self.view_gains:
            if int(self.gain_rounds) < 1:
                raise ValueError(f'gain_rounds must be >= 1, not {self.gain_rounds!r}')
            if not (np.isfinite(float(self.gain_limit)) and float(self.gain_limit) >= 1):
                raise ValueError(f'gain_limit must be finite and >= 1, not {self.gain_limit!r}')
            if self.trim_outliers is not None:
                raise ValueError('view_gains does not combine with trim_outliers')
        for name, on in (('trim_outliers', self.trim_outliers is not None), ('view_gains', self.view_gains)):
            if on and save_interval is not None:
                raise ValueError(f'{name} does not combine with save_interval snapshots')
        return dataclasses.replace(self, stretch=stretch)


_NO_EXTRAS = _Extras()


class _Job:
    """One image between ``_restore_submit`` (everything enqueued, nothing waited for) and ``_restore_finish``.  ``extras``: what
    was asked for; ``trace``: the last fit's; ``quality``, ``trim``, ``gains``: the records of --save-quality and of every round;
    ``uncertainty``: that of --save-uncertainty, ``pooled_uncertainty``: the ``engine.water_uncertainty`` of a shared fit's pooled sums."""
    extras = _NO_EXTRAS
    params0 = None   # the start of every fit, on the host; None: read from the module (``adam``)
    trace = quality = trim = gains = uncertainty = pooled_uncertainty = None

    def __init__(self, **kw):
        self.__dict__.update(kw)


def adam(sucre: SUCRe, matches_data: loader.MatchesData, lr: float = 0.05, num_iter: int = 200, batch_size: int = 1,
         save_dir: Path = None, save_interval: int = None, device: str = 'cpu', verbose: bool = True,
         trim_outliers: float = None, trim_rounds: int = 1, view_gains: bool = False, gain_rounds: int = 1,
         gain_limit: float = 2.0, save_uncertainty: bool = False, _job: _Job = None) -> SUCRe:
    """``num_iter`` steps of ``torch.optim.Adam(lr)`` on the least-squares cost (sucre.py:124-157).

    ``batch_size`` is accepted for compatibility: the engine always uses the full batch in one pass, which is
    what the reference's accumulated mini-batch gradients add up to.

    ``trim_outliers`` (not a reference argument): after the fit, ``trim_rounds`` rounds of trim -> fit anew from the same
    initial values with the same ``num_iter`` (``_enqueue_trim``); the model ends with the last fit, and ``sucre._trim`` holds
    every round's record.

    ``view_gains`` (not a reference argument): after the fit, ``gain_rounds`` rounds of estimate the per-view gains -> divide
    them out of the store -> fit anew from the same initial values with the same ``num_iter`` (``_enqueue_gains``);
    ``sucre._gains`` holds every round's record.  Not together with ``trim_outliers``.

    ``save_uncertainty`` (not a reference argument): behind the last fit, the float64 pass of ``engine.Restoration.uncertainty``;
    ``sucre._uncertainty`` holds its ``(count, jterms, sums)`` on the device (``engine.water_uncertainty``,
    ``engine.j_standard_error``).  Not with the light model.

    ``_job`` (internal, ``_restore_one``): its ``extras`` stand in for the six keywords above and may ask for the quality pass
    behind the last fit; it receives the records."""
    extras = _job.extras if _job is not None else _Extras(trim_outliers=trim_outliers, trim_rounds=trim_rounds, view_gains=view_gains,
                                                          gain_rounds=gain_rounds, gain_limit=gain_limit, save_uncertainty=save_uncertainty)
    if extras.save_uncertainty and sucre.light_model:
        raise NotImplementedError(_NO_LIGHT_UNCERTAINTY)
    extras = extras.checked(save_interval if save_dir is not None else None)
    job = _Job(sucre=sucre, matches_data=matches_data, extras=extras)   # (no params0: every fit starts from what the module holds)
    print(f'Solve least squares with Adam optimizer ({num_iter} iterations).')
    job.resto = resto = _begin(job)
    done = 0
    for stop, snapshot in snapshot_stops(num_iter, save_interval if save_dir is not None else None):
        if stop > done:
            # at a snapshot stop closed-form J stays J(theta_k) of the last iteration k: the pair
            # (J(theta_k), theta_{k+1}) is what the reference plots (sucre.py:141,153-154)
            trace = resto.fit(stop - done, lr=lr, use_closed_form=sucre.use_closed_form, keep_J=snapshot)
            if verbose:
                _log_trace(trace.cpu().numpy(), done)
            done = stop
        if snapshot:
            _pull_results(sucre, resto)
            sucre.save_plots(save_dir=save_dir, iteration=done - 1)
            if sucre.use_closed_form and done == num_iter:
                resto.update_J()   # the final update_J of sucre.py:156, held back for the snapshot

    def fit_again(jobs, after):
        print(f'Solve least squares with Adam optimizer ({num_iter} iterations) after {after}.')
        trace = resto.fit(num_iter, lr=lr, use_closed_form=sucre.use_closed_form)
        if verbose:
            _log_trace(trace.cpu().numpy(), 0)
    # (no snapshot stops in the rounds: nothing has been pulled into the model yet, so each starts from the same values again)
    _enqueue_refits([job], fit_again)
    _enqueue_quality(job)   # --save-quality: the pass right behind the fit, read with the results
    _enqueue_uncertainty(job)
    if job.uncertainty is not None:
        sucre._uncertainty = job.uncertainty
    if job.trim is not None:
        sucre._trim = job.trim
    if job.gains is not None:
        sucre._gains = job.gains
    if _job is not None:
        _job.quality, _job.trim, _job.gains, _job.uncertainty = job.quality, job.trim, job.gains, job.uncertainty
    _pull_results(sucre, resto)
    return sucre


def _begin(job: _Job):
    """``_adam_begin`` of a job: from its start values on the host when it has them, from the module otherwise."""
    if job.params0 is None:
        return _adam_begin(job.sucre, job.matches_data)
    return _adam_begin(job.sucre, job.matches_data, params0=job.params0)


def _adam_begin(sucre: SUCRe, matches_data: loader.MatchesData, params0: np.ndarray | None = None):
    """``params0``: the model's water (and light) parameters when the caller already has them on the host; reading
    them from the module costs a device-to-host copy, i.e. a wait for everything enqueued on the stream."""
    resto = _restoration_of(matches_data, sucre)
    if sucre.light_model and not resto.light:
        raise RuntimeError('these matches were computed without light_model=True: the camera points the light model '
                           'needs were not kept (call Image.match_images(..., light_model=True))')
    target = sucre.image.device_view(resto.device)
    if resto.float_colour:
        target = target.as_float_colour()
    J0 = None if (sucre.use_closed_form or getattr(sucre, '_J_unset', False)) else sucre.J.detach()
    if params0 is None:
        params0 = sucre.water_vector().detach().cpu().numpy()
    resto.fit_init(target, params0=params0, J0=J0)
    return resto


# ---- --save-quality: where J can be trusted, and which view hurts the fit -----------------------------------------------
QUALITY_RMS_FULL_SCALE = 0.25   # RMS residual (intensities are in [0, 1]) that maps to white in <stem>_residual.png


def coverage_image(count: np.ndarray, n_kept: int) -> np.ndarray:
    """8-bit grey: ``255 * count // n_kept`` -- the share of the kept views that observe the pixel."""
    count = np.asarray(count, np.int64)
    return np.uint8(255 * count // max(1, int(n_kept)))


def residual_image(count: np.ndarray, ssr: np.ndarray) -> np.ndarray:
    """8-bit grey: ``uint8(255 * min(1, rms / QUALITY_RMS_FULL_SCALE))`` with ``rms = sqrt(sum_c ssr_c / (3 count))``, 0 where
    the pixel has no observation."""
    count = np.asarray(count, np.float64)
    total = np.asarray(ssr, np.float64).sum(axis=-1)
    rms = np.sqrt(np.divide(total, 3.0 * count, out=np.zeros_like(total), where=count > 0))
    return np.uint8(255.0 * np.minimum(1.0, rms / QUALITY_RMS_FULL_SCALE))


def _enqueue_residuals(resto) -> tuple:
    """The residual pass on the current stream, no host wait: (count, ssr, view_stats, view_keep) on the device."""
    return resto.residuals() + (resto.view_keep().clone(),)


def _enqueue_quality(job) -> None:
    if job.extras.save_quality:
        job.quality = _enqueue_residuals(job.resto)


def _view_names(job, n_views: int) -> list:
    """The names of the views a job's records have their rows for; their indices where the matches carry no image list."""
    image_list = getattr(job.matches_data, 'image_list', None)
    return [im.name for im in image_list] if image_list else [str(k) for k in range(n_views)]


def _write_quality(job) -> None:
    """``<stem>_quality.pt``, ``<stem>_coverage.png``, ``<stem>_residual.png`` and one printed line."""
    count, ssr, stats, keep = job.quality   # host tensors (_restore_finish)
    stem = Path(job.image.name).stem
    views = _view_names(job, stats.shape[0])
    view_kept = keep != 0
    view_n = stats[:, 0].round().to(torch.int64)
    view_ssr = stats[:, 1:].clone()
    torch.save({'count': count, 'ssr': ssr, 'views': views, 'view_kept': view_kept, 'view_n': view_n, 'view_ssr': view_ssr},
               job.output_dir / f'{stem}_quality.pt')
    _save_png(PILImage.fromarray(coverage_image(count.numpy(), int(view_kept.sum()))), job.output_dir / f'{stem}_coverage.png')
    _save_png(PILImage.fromarray(residual_image(count.numpy(), ssr.numpy())), job.output_dir / f'{stem}_residual.png')
    n = int(view_n.sum())
    rms = np.sqrt(view_ssr.sum(dim=0).numpy() / max(1, n))
    per_view = np.sqrt(view_ssr.sum(dim=1).numpy() / np.maximum(1, 3 * view_n.numpy()))
    per_view[~(view_kept.numpy() & (view_n.numpy() > 0))] = -1.0
    line = f'{job.image.name}: residual RMS R {rms[0]:.4f} G {rms[1]:.4f} B {rms[2]:.4f} over {n} observations'
    if (per_view >= 0).any():
        worst = int(per_view.argmax())
        line += f'; worst kept view {views[worst]} (RMS {per_view[worst]:.4f})'
    print(line)


# ---- --save-uncertainty: how well the observations determine B, beta, gamma and J -----------------------------------------------
_NO_LIGHT_UNCERTAINTY = ('the uncertainty of a light-model fit is not built: the lamp\'s ten parameters would have to join B, beta, '
                         'gamma, and errors conditional on a fixed lamp would understate')
_CHANNELS = 'RGB'


def _enqueue_uncertainty(job) -> None:
    """The float64 pass on the current stream, no host wait: (count, jterms, sums) on the device."""
    if job.extras.save_uncertainty:
        job.uncertainty = job.resto.uncertainty()


def pooled_uncertainty(sums_list: list, group=None) -> torch.Tensor:
    """The 24 float64 words of several images' ``engine.Restoration.uncertainty`` added up, on the host: H, SSR, N and P (and the
    pixels without an A) of a fit that shares its water add over the images -- in the order of the list within this rank, then
    through ``dist.all_reduce_sum`` across the ranks of ``group``.  RCCL reduces device tensors only (``dist.fit_shared_water``
    moves its observation count for the same reason): under an 'nccl' group the 24 words go to this rank's device -- that of the
    sums, the current one for host sums --, are reduced there and come back.  ``engine.water_uncertainty`` of the result is the
    shared parameters' covariance."""
    import torch.distributed as tdist

    from . import _lib
    total = torch.zeros(_lib.UNCERTAINTY_WORDS, dtype=torch.float64)
    for sums in sums_list:
        total = total + sums.detach().to('cpu', torch.float64).reshape(-1)
    if tdist.is_initialized() and tdist.get_backend(group) == 'nccl':
        dev = next((s.device for s in sums_list if s.is_cuda), None)
        comm = total.to(dev if dev is not None else torch.device('cuda', torch.cuda.current_device()))
        sdist.all_reduce_sum(comm, group)
        return comm.cpu()
    sdist.all_reduce_sum(total, group)
    return total


def uncertainty_image(J_se: np.ndarray) -> np.ndarray:
    """8-bit grey: ``uint8(255 * min(1, sqrt(mean_c sigma_J^2) / QUALITY_RMS_FULL_SCALE))``, 0 where nothing is observed (or the
    channel's water is not determined: sigma_J is NaN there)."""
    var = np.asarray(J_se, np.float64) ** 2
    rms = np.sqrt(np.nan_to_num(var.mean(axis=-1), nan=0.0, posinf=np.inf))
    return np.uint8(255.0 * np.minimum(1.0, rms / QUALITY_RMS_FULL_SCALE))


def _uncertainty_record(result: dict) -> dict:
    """What ``engine.water_uncertainty`` returned (with the ``sums`` it was made from) as the tensors of a .pt file."""
    t = lambda x, dt=torch.float64: torch.as_tensor(np.asarray(x), dtype=dt)   # noqa: E731
    se = t(result['se'])
    return {'B_se': se[:, 0:1].clone(), 'beta_se': se[:, 1:2].clone(), 'gamma_se': se[:, 2:3].clone(), 'cov': t(result['cov']),
            'corr': t(result['corr']), 'cond': t(result['cond']), 's2': t(result['s2']), 'dof': int(result['dof']),
            'n_obs': int(result['n_obs']), 'n_pixels': int(result['n_pixels']), 'normal': t(result['normal']),
            'sums': t(result['sums']), 'well_posed': t(result['well_posed'], torch.bool)}


def _uncertainty_line(result: dict, J_se: np.ndarray = None) -> str:
    from .engine import WATER_NAMES
    se, ok = np.asarray(result['se']), np.asarray(result['well_posed'], bool)
    parts = [f'{name} ± ' + '/'.join(f'{se[c, i]:.4g}' if ok[c] else 'n/a' for c in range(3)) for i, name in enumerate(WATER_NAMES)]
    line = 'standard errors ' + ', '.join(parts)
    if ok.any():
        corr = np.where(ok[:, None, None], np.asarray(result['corr']), 0.0)
        pairs = [(abs(corr[c, i, j]), c, i, j) for c in range(3) for i in range(3) for j in range(i + 1, 3)]
        _, c, i, j = max(pairs)
        line += f'; strongest correlation {WATER_NAMES[i]}~{WATER_NAMES[j]} {corr[c, i, j]:.3f} ({_CHANNELS[c]})'
    if J_se is not None:
        med = [np.nanmedian(J_se[..., c]) if np.isfinite(J_se[..., c]).any() else np.nan for c in range(3)]
        line += '; median sigma_J ' + ' '.join(f'{_CHANNELS[c]} {med[c]:.4g}' for c in range(3))
    for c in np.nonzero(~ok)[0]:
        line += f'; channel {_CHANNELS[c]}: the water parameters are not determined by these observations (dof {int(result["dof"])})'
    return line


def _uncertainty_on_host(job) -> dict:
    """The record of --save-uncertainty with sigma_J made where the terms are (``engine.j_standard_error``), then on the host.  With
    a shared fit the covariance is the pooled one (``job.pooled_uncertainty``); ``sums`` stay the image's own."""
    from . import engine
    count, jterms, sums = job.uncertainty
    own = sums.cpu()
    result = dict(job.pooled_uncertainty) if job.pooled_uncertainty is not None else engine.water_uncertainty(own)
    J_se = engine.j_standard_error(jterms, count, result).cpu()
    result['sums'] = own.numpy()
    return {**_uncertainty_record(result), 'J_se': J_se, 'count': count.cpu(), 'result': result}


def _write_uncertainty(job) -> None:
    """``<stem>_uncertainty.pt``, ``<stem>_uncertainty.png`` and one printed line."""
    record = dict(job.uncertainty)   # host tensors (_restore_finish)
    result = record.pop('result')
    stem = Path(job.image.name).stem
    torch.save(record, job.output_dir / f'{stem}_uncertainty.pt')
    J_se = record['J_se'].numpy()
    _save_png(PILImage.fromarray(uncertainty_image(J_se)), job.output_dir / f'{stem}_uncertainty.png')
    print(f'{job.image.name}: ' + _uncertainty_line(result, J_se))


# ---- --trim-outliers: sigma-clip single observations on the device, fit again ------------------------------------------
def _enqueue_trim(resto, k_sigma: float) -> dict:
    """One round on the current stream, no host wait (``Restoration.trim_outliers`` behind the residual pass it takes its scale
    from); the fit must be started over.  The round's record, on the device."""
    n_obs, kept = resto.n_obs_device().clone(), resto.view_keep().clone()
    dropped, view_dropped, thresholds = resto.trim_outliers(k_sigma, resto.residuals())
    return {'dropped': dropped, 'view_dropped': view_dropped, 'thresholds': thresholds, 'n_obs': n_obs, 'view_kept': kept,
            'k': float(k_sigma)}


def trimmed_image(dropped_rounds, n_kept: int) -> np.ndarray:
    """``<stem>_trimmed.png``: ``coverage_image`` of the observations dropped from every pixel, summed over the rounds, against
    the number of views kept before the first round."""
    total = np.asarray(dropped_rounds, np.int64)
    return coverage_image(total.reshape((-1,) + total.shape[-2:]).sum(axis=0), n_kept)


def _write_trim(job) -> None:
    """``<stem>_trim.pt``, ``<stem>_trimmed.png`` and one printed line per round."""
    rounds = job.trim   # host tensors (_restore_finish)
    stem = Path(job.image.name).stem
    views = _view_names(job, int(rounds[0]['view_dropped'].shape[0]))
    dropped = torch.stack([r['dropped'] for r in rounds])
    torch.save({'dropped': dropped, 'views': views, 'view_dropped': torch.stack([r['view_dropped'] for r in rounds]),
                'thresholds': torch.stack([r['thresholds'] for r in rounds]), 'k': rounds[0]['k'],
                'n_obs': torch.cat([r['n_obs'] for r in rounds]), 'view_kept': torch.stack([r['view_kept'] != 0 for r in rounds])},
               job.output_dir / f'{stem}_trim.pt')
    _save_png(PILImage.fromarray(trimmed_image(dropped.numpy(), int((rounds[0]['view_kept'] != 0).sum()))),
              job.output_dir / f'{stem}_trimmed.png')
    for i, r in enumerate(rounds):
        t = np.sqrt(r['thresholds'].numpy().astype(np.float64))
        print(f'{job.image.name}: trim round {i + 1} dropped {int(r["view_dropped"].sum())} of {int(r["n_obs"])} observations '
              f'(threshold R {t[0]:.4f} G {t[1]:.4f} B {t[2]:.4f})')


# ---- --view-gains: one multiplicative gain per view and channel, estimated on the device and divided out; fit again ------
def _enqueue_gains(resto, limit: float) -> dict:
    """One round on the current stream, no host wait (``Restoration.view_gains``, then ``apply_view_gains`` with what it
    estimated); the fit must be started over.  The round's record, on the device."""
    kept = resto.view_keep().clone()
    gains, inv, sums = resto.view_gains(limit)
    view_clipped = resto.apply_view_gains(inv)
    return {'gains': gains, 'inv': inv, 'sums': sums, 'view_clipped': view_clipped, 'view_kept': kept, 'limit': float(limit)}


def _write_gains(job) -> None:
    """``<stem>_gains.pt`` and one printed line per round."""
    rounds = job.gains   # host tensors (_restore_finish)
    stem = Path(job.image.name).stem
    n_views = int(rounds[0]['gains'].shape[0])
    views = _view_names(job, n_views)
    gain = torch.ones((n_views, 3), dtype=torch.float64)
    for r in rounds:
        gain = gain * r['gains']
    torch.save({'views': views, 'gains': torch.stack([r['gains'] for r in rounds]), 'sums': torch.stack([r['sums'] for r in rounds]),
                'view_clipped': torch.stack([r['view_clipped'] for r in rounds]),
                'view_kept': torch.stack([r['view_kept'] != 0 for r in rounds]), 'gain': gain, 'limit': rounds[0]['limit']},
               job.output_dir / f'{stem}_gains.pt')
    for i, r in enumerate(rounds):
        g = r['gains'].numpy()
        worst = int(np.abs(np.log(g)).max(axis=1).argmax())
        print(f'{job.image.name}: gain round {i + 1}: largest correction in view {views[worst]} '
              f'(gain R {g[worst, 0]:.4f} G {g[worst, 1]:.4f} B {g[worst, 2]:.4f}; {int(r["view_clipped"].sum())} values clipped)')


# ---- the rounds behind a fit: change the store, start over, fit again ----------------------------------------------------------
# per kind, in the order they run: the field of _Extras that switches it on, the field with its rounds, what a round enqueues
# (with the workspace and the field that holds its argument), the attribute of _Job that collects the records, its word in a line
_REFITS = (('trim_outliers', 'trim_rounds', _enqueue_trim, 'trim_outliers', 'trim', 'trim'),
           ('view_gains', 'gain_rounds', _enqueue_gains, 'gain_limit', 'gains', 'gain'))


def _enqueue_refits(jobs: list, fit) -> None:
    """The rounds of --trim-outliers, then those of --view-gains, for images whose first fit is enqueued.  A round: for every image
    that still has one to run, what the kind enqueues and ``fit_init`` with the initial values of the first fit; then
    ``fit(images, 'trim round 1')`` -- the caller's way of fitting them again, alone or in a batch launch, and of saying so."""
    for switch, rounds, enqueue, argument, records, word in _REFITS:
        on = [j for j in jobs if getattr(j.extras, switch) not in (None, False)]
        for job in on:
            setattr(job, records, [])
        for i in range(max((int(getattr(j.extras, rounds)) for j in on), default=0)):
            again = [j for j in on if i < int(getattr(j.extras, rounds))]
            for job in again:
                getattr(job, records).append(enqueue(job.resto, getattr(job.extras, argument)))
                _begin(job)
            fit(again, f'{word} round {i + 1}')


def _restore_submit(image: sfm.Image, colmap_model: sfm.COLMAPModel, output_dir: Path, light_model: bool,
                    use_closed_form: bool, min_cover: float, image_list: list[sfm.Image], lr: float, num_iter: int,
                    params_path: Path, force_compute_matches: bool, num_workers: int, device: str,
                    defer_checks: bool = False, extras: _Extras = _NO_EXTRAS) -> _Job:
    """Stages of sucre.py:160-210 up to and including the enqueued fit; the trace and J stay on the device.
    ``defer_checks``: the integrity verdicts and the observation count stay on the device until ``_restore_finish``
    reads them with the results -- waiting for them here would make the host wait for the matching, which shares the
    GPU with the previous image's fit, before it can enqueue this image's fit (measured: 7-37 ms per image)."""
    print(f'Restore {image.name}.')
    output_dir = Path(output_dir)
    matches_path = (output_dir / image.name).with_suffix('.h5')
    matches_file = loader.MatchesFile(matches_path, colmap_model=colmap_model, overwrite=force_compute_matches)
    if image_list is None:
        image_list = list(colmap_model.images.values())

    # The model is built before the matching is enqueued (the reference builds it after, sucre.py:199; the two do not
    # depend on each other): moving its parameters to the device is a host-to-device copy, which the host waits for,
    # and behind the matching on the same stream that wait would last until the matching is done.
    if str(device).startswith('cuda'):
        image.device_view(device)   # J starts from the resident pixels (SUCRe.__init__)
    sucre = SUCRe(image=image, light_model=light_model, use_closed_form=use_closed_form,
                  _J_by_engine=defer_checks and params_path is None)
    if params_path is not None:
        sucre.load_state_dict(torch.load(params_path), strict=False)
    params0 = sucre.water_vector().detach().cpu().numpy()   # still on the host: no wait
    sucre.stretch = extras.stretch   # (lo, hi): every _rgb*.png of this model, snapshots included (plot_J)
    sucre = sucre.to(device)

    reuse = not force_compute_matches and matches_file.on_disk()
    if reuse:   # a kept matches file (ours or the reference's): consumed as is, like sucre.py:185
        try:
            matches_file.load_file(image, device=device, light=light_model)
        except NotImplementedError as e:   # e.g. --light-model on kept matches of resized images
            print(f'{matches_file.path.name} is not reused ({e}).')
            reuse = False
    if not reuse:
        print(f'Compute {image.name} matches.')
        image.match_images(image_list=image_list, matches_file=matches_file, min_cover=min_cover,
                           num_workers=num_workers, device=device, light_model=light_model)
        print('Prepare matches for optimization.')
        matches_file.prepare_matches(num_workers=num_workers)
    print('Check matches integrity.')
    matches_file.check_integrity(defer=defer_checks)
    print('Load matches.')
    matches_data = matches_file.load_matches(pin_memory=False)
    if not defer_checks:
        _report_observations(image, len(matches_data))

    return _Job(image=image, sucre=sucre, matches_file=matches_file, matches_data=matches_data,
                matches_path=matches_path, output_dir=output_dir, lr=lr, num_iter=num_iter, deferred_checks=defer_checks,
                params0=params0, extras=extras)


def _report_observations(image: sfm.Image, n_obs: int) -> None:
    print(f'Total of {n_obs} observations.')
    if n_obs == 0:
        raise RuntimeError(f'{image.name}: no observation survived matching; nothing to fit')


def _restore_enqueue_fits(jobs: list) -> None:
    """The whole fit of sucre.py:138-156 of every image of a chunk enqueued in one go (no intermediate plots): no host
    synchronisation.  Images of one size without the extension planes (light model, float32 colours) advance in ONE launch per
    iteration (``engine.fit_batch``: what a small image pays for most is its own launches -- 640x480 x 5 views: 16.7 us per image
    and iteration alone, 7.3 in a launch of 32), with the bits of a fit by itself.  Whatever does not fit a batch is fitted by
    itself; a chunk of one says so once, a larger one before every refit too."""
    from . import engine
    groups: dict = {}
    singles = []
    for job in jobs:
        job.resto = resto = _begin(job)
        if resto.light or resto.float_colour:
            singles.append(job)
        else:
            groups.setdefault((resto.H, resto.W, resto.obs_format, job.num_iter, job.lr, job.sucre.use_closed_form), []).append(job)

    def fit_alone(members, after=None):
        for job in members:
            if after is None or len(jobs) > 1:
                print(f'Solve least squares with Adam optimizer ({job.num_iter} iterations).')
            job.trace = job.resto.fit(job.num_iter, lr=job.lr, use_closed_form=job.sucre.use_closed_form)

    def fit_together(members, after=None):   # (the refits too: a batch launch gives every image its own bits)
        if len(members) == 1:
            return fit_alone(members, after)
        first = members[0]   # (one group: one num_iter, lr and use_closed_form)
        print(f'Solve least squares with Adam optimizer ({first.num_iter} iterations), {len(members)} images per launch.')
        traces = engine.fit_batch([j.resto for j in members], first.num_iter, lr=first.lr, use_closed_form=first.sucre.use_closed_form)
        for j, t in zip(members, traces):
            j.trace = t

    batches = [members for members in groups.values() if len(members) > 1]
    singles += [members[0] for members in groups.values() if len(members) == 1]
    for members, fit in [(members, fit_together) for members in batches] + [(singles, fit_alone)]:
        fit(members)
        _enqueue_refits(members, fit)
        for job in members:
            _enqueue_quality(job)
            _enqueue_uncertainty(job)


def fit_batch_size(images: list, light_model: bool = False, in_flight: int = 2, n_views: int | None = None, device='cuda') -> int:
    """Images per fit launch in a survey (engine knob ``SUCRE_FIT_BATCH``; not a reference flag).  ``auto``: 8 for images of
    less than a megapixel (BASELINE config 1's 640x480: 144 -> 215 Mpix/s; 32 per launch: 219), 1 otherwise -- at 1080p a
    launch of two images is no faster than two launches in flight -- and 1 with the light model.
    Every image of a chunk holds its own workspace, ``fit_batch x in_flight`` of them at once: with ``n_views`` (the largest
    number of views a target can be matched against) the automatic batch is halved until those workspaces fit into 80 % of
    the device memory that is free now -- a 1280x720 survey with hundreds of neighbours keeps fewer images per launch instead
    of running out of memory."""
    env = os.environ.get('SUCRE_FIT_BATCH', 'auto').strip().lower()
    if env != 'auto':
        return max(1, int(env))
    if light_model or not images:
        return 1
    W, H = max(int(im.camera.width) for im in images), max(int(im.camera.height) for im in images)
    batch = 8 if W * H < 1_000_000 else 1
    if batch > 1 and n_views:
        from . import _lib, engine
        cap = min(engine.view_capacity(min(int(n_views), engine.MAX_VIEWS)), engine.MAX_VIEWS)
        need = int(_lib.load().sucre_workspace_bytes(H, W, cap))
        try:
            free = int(torch.cuda.mem_get_info(device)[0]) + int(torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device))
        except Exception:   # no device to ask: keep the plain rule
            return batch
        while batch > 1 and need * batch * max(1, int(in_flight)) > 0.8 * free:
            batch //= 2
    return batch


def _rounds_on_host(rounds: list | None) -> list | None:
    """The records of a job's trim or gain rounds with their tensors copied to the host; None when it ran none."""
    return None if rounds is None else [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()} for r in rounds]


def _restore_finish(job: _Job, keep_matches: bool, writers: ThreadPoolExecutor | None = None):
    """Results back from the device (the only wait of the image), then the output files (sucre.py:211-219).  With a
    ``writers`` pool the files are written in the background -- percentile stretch, PNG encoding and the .pt take
    ~1 s of host time per 1080p image, 30x the GPU time -- and the future is returned instead of the model."""
    sucre = job.sucre
    if job.deferred_checks:   # raises what check_integrity / the empty-list test would have raised before the fit
        _report_observations(job.image, job.matches_file.finish_integrity())
    if job.trace is not None:
        job.trace = job.trace.cpu().numpy()
        if writers is None:
            _log_trace(job.trace, 0)
        _pull_results(sucre, _restoration_of(job.matches_data))
    if job.quality is not None:
        job.quality = tuple(t.cpu() for t in job.quality)
    job.trim, job.gains = _rounds_on_host(job.trim), _rounds_on_host(job.gains)
    if job.uncertainty is not None:
        job.uncertainty = _uncertainty_on_host(job)
    if keep_matches and job.matches_file.restoration._views_dev is not None:   # freshly matched (not loaded from this
        if job.trim is not None:                                               # very file); needs the live workspace
            print(f'Keep {job.matches_file.save(survivors=True)} (the observations that survived the trim).')
        elif job.gains is not None:
            print(f'Keep {job.matches_file.save(colour_scales=[r["inv"] for r in job.gains])} (colours with the view gains divided out).')
        else:
            print(f'Keep {job.matches_file.save()}.')
    if writers is None:
        _write_outputs(job, keep_matches)
        return sucre
    if sucre.B.is_cuda:
        torch.cuda.current_stream(sucre.B.device).synchronize()   # the writer thread works on another stream
    return writers.submit(_write_outputs, job, keep_matches, True)


def _write_outputs(job: _Job, keep_matches: bool, log: bool = False) -> None:
    sucre = job.sucre
    if log and job.trace is not None:   # formatted off the main thread, printed as one block
        print(f'{job.image.name}:\n' + _format_trace(job.trace, 0))
    sucre.save_plots(save_dir=job.output_dir)
    if job.quality is not None:
        _write_quality(job)
    if job.trim is not None:
        _write_trim(job)
    if job.gains is not None:
        _write_gains(job)
    if job.uncertainty is not None:
        _write_uncertainty(job)
    torch.save({**sucre.cpu().state_dict(), 'J': sucre.J.detach().cpu()},
               (job.output_dir / job.image.name).with_suffix('.pt'))
    if not keep_matches and job.matches_path.exists():
        print(f'Erase {job.matches_path}.')
        job.matches_path.unlink()


def restore_image(image: sfm.Image, colmap_model: sfm.COLMAPModel, output_dir: Path, light_model: bool = False,
                  use_closed_form: bool = False, min_cover: float = 0.000001, image_list: list[sfm.Image] = None,
                  lr: float = 0.05, num_iter: int = 200, batch_size: int = 1, save_interval: int = None,
                  params_path: Path = None, force_compute_matches: bool = False, keep_matches: bool = False,
                  num_workers: int = 0, device: str = 'cpu'):
    """Per-image pipeline (sucre.py:160-219): match -> prepare -> check -> load -> fit -> save.  The signature is the
    reference's, default ``device='cpu'`` included -- which this engine refuses (``sfm.require_gpu``): pass a GPU."""
    return _restore_one(image, colmap_model, output_dir, light_model, use_closed_form, min_cover, image_list, lr, num_iter,
                        batch_size, save_interval, params_path, force_compute_matches, keep_matches, num_workers, device)


def _restore_one(image, colmap_model, output_dir, light_model, use_closed_form, min_cover, image_list, lr, num_iter, batch_size,
                 save_interval, params_path, force_compute_matches, keep_matches, num_workers, device, extras: _Extras = _NO_EXTRAS):
    """``restore_image`` plus what its pinned signature has no room for (``_Extras``)."""
    sfm.require_gpu(device, 'restore_image')
    extras = extras.checked(save_interval)
    job = _restore_submit(image, colmap_model, output_dir, light_model, use_closed_form, min_cover, image_list, lr,
                          num_iter, params_path, force_compute_matches, num_workers, device, extras=extras)
    adam(sucre=job.sucre, matches_data=job.matches_data, lr=lr, num_iter=num_iter, batch_size=batch_size,
         save_dir=job.output_dir, save_interval=save_interval, device=device, _job=job)
    return _restore_finish(job, keep_matches)


def restore_images(images: list[sfm.Image], colmap_model: sfm.COLMAPModel, output_dir: Path, in_flight: int = 2,
                   keep_matches: bool = False, device: str = 'cuda', fit_batch: int | None = None, **kw) -> None:
    """A survey: the same per-image pipeline with ``in_flight`` images on the GPU at once (engine.in_flight_slot)
    and the output files written by background threads (SUCRE_WRITER_THREADS).  While image i iterates,
    image i+1 is matched and submitted and the plots of images < i are encoded, so neither the tails of the fit
    launches nor the PNG encoding leave the GPU idle.  Per-image results are the same bits as ``restore_image``
    (each image has its own workspace and stream; nothing is shared).  ``fit_batch`` consecutive images share a slot and
    their fits one launch per iteration (``fit_batch_size``; same bits again).  ``trim_outliers=None, trim_rounds=1`` (in
    ``kw``): the rounds of --trim-outliers, enqueued with the image behind its first fit, no host wait added; ``view_gains=False,
    gain_rounds=1, gain_limit=2.0``: those of --view-gains, likewise; ``stretch=(lo, hi)``: every ``_rgb.png`` by this fixed
    stretch (``check_stretch``) instead of the image's own percentiles (--stretch-from)."""
    extras = _Extras(**{f.name: kw.pop(f.name) for f in dataclasses.fields(_Extras) if f.name in kw}).checked()
    pending: list[tuple[int, list]] = []
    written = []
    if fit_batch is None:
        candidates = kw.get('image_list')
        n_views = len(candidates) if candidates is not None else len(colmap_model.images)
        fit_batch = fit_batch_size(images, bool(kw.get('light_model', False)), in_flight=in_flight, n_views=n_views, device=device)
    _restore_pipeline(images, colmap_model, output_dir, in_flight, keep_matches, device, pending, written, kw, extras, max(1, int(fit_batch)))


def _restore_pipeline(images, colmap_model, output_dir, in_flight, keep_matches, device, pending, written, kw, extras: _Extras,
                      fit_batch: int = 1) -> None:
    from . import engine
    # writer threads: the CPUs this process may use minus two (this thread and the HIP runtime's), at most 32
    with ThreadPoolExecutor(max_workers=max(1, int(os.environ.get('SUCRE_WRITER_THREADS', min(32, loader.effective_cpus() - 2)))),
                            thread_name_prefix='sucre-write') as writers:
        def finish(slot, jobs):
            with engine.in_flight_slot(slot, device, wait_for_caller=False):
                for job in jobs:
                    written.append(_restore_finish(job, keep_matches, writers))
            while len(written) > 64:                  # bound the host memory held by queued outputs (~50 MB each)
                written.pop(0).result()

        chunks = [images[i:i + fit_batch] for i in range(0, len(images), fit_batch)]
        for c, chunk in enumerate(chunks):
            slot = c % in_flight
            while pending and (len(pending) >= in_flight or pending[0][0] == slot):
                finish(*pending.pop(0))
            with engine.in_flight_slot(slot, device, wait_for_caller=False):   # inputs: Image.device_view, complete
                jobs = []
                for k, image in enumerate(chunk):
                    with engine.slot_lane(k):   # every image of the chunk in its own workspace
                        jobs.append(_restore_submit(image, colmap_model, output_dir, device=device, defer_checks=True, extras=extras, **kw))
                _restore_enqueue_fits(jobs)
            pending.append((slot, jobs))
        for slot, jobs in pending:
            finish(slot, jobs)
        for f in written:
            f.result()   # re-raises anything a writer thread hit


# ---- --apply-water: a fitted water model applied to any image (single-view inversion) ------------------------------------
APPLY_IMAGES_PER_LAUNCH = 32


def water_shapes(light_model: bool) -> dict:
    """Key -> shape of what a water file must hold (sucre.py:41-46)."""
    shapes = {'B': (3, 1), 'beta': (3, 1), 'gamma': (3, 1)}
    if light_model:
        shapes.update(cam2light=(6,), sigma=(2, 2))
    return shapes


def check_water(water, light_model: bool = False, where: str = 'water') -> dict:
    """The float32 CPU tensors ``B, beta, gamma`` (3,1) -- and ``cam2light`` (6), ``sigma`` (2,2) with the light model -- of a
    mapping such as a loaded ``shared_water.pt`` or per-image ``<name>.pt``; other keys are ignored.  ``ValueError`` naming the
    first key that is missing or mis-shaped."""
    if not hasattr(water, 'keys'):
        raise ValueError(f'{where} holds no parameters (a mapping with the keys {", ".join(water_shapes(light_model))} is expected)')
    out = {}
    for key, shape in water_shapes(light_model).items():
        if key not in water:
            raise ValueError(f"{where} holds no '{key}'" + (' (--light-model needs the light parameters too)' if key in ('cam2light', 'sigma') else ''))
        t = water[key]
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"'{key}' in {where} is {got}, expected a tensor of shape {shape}")
        out[key] = t.detach().to('cpu', torch.float32)
    return out


def read_water_file(path: Path, light_model: bool = False) -> dict:
    """``check_water`` of a ``.pt`` file, for the command line: ``SystemExit`` naming the file and the key."""
    try:
        data = torch.load(path, map_location='cpu')
    except Exception as e:
        raise SystemExit(f'--apply-water: cannot read {path}: {e}')
    try:
        return check_water(data, light_model, where=str(path))
    except ValueError as e:
        raise SystemExit(f'--apply-water: {e}')


def _free_device_memory(device) -> int:
    return int(torch.cuda.mem_get_info(device)[0])


def _check_stretch_memory(images: list, device) -> None:
    """--apply-water --common-stretch keeps the J of every image of this rank on the device until the pool is complete: their
    H W 12 bytes must fit into 0.8 of what is free now.  Checked before any image is decoded."""
    need = sum(int(im.camera.height) * int(im.camera.width) * 12 for im in images)
    free = _free_device_memory(device)
    if need > 0.8 * free:
        raise SystemExit(f'--common-stretch: the restored images of this rank ({len(images)} image(s), {need} bytes) stay on {device} '
                         f'until the pool is complete, and {free} bytes are free; run more ranks (torchrun --nproc-per-node N), or '
                         f'measure the stretch on fewer images and give its stretch.pt to the others with --stretch-from')


def _write_common_stretch(output_dir: Path, lo, hi, n_valid: int, request: list, rank: int) -> None:
    """Rank 0: ``stretch.pt`` and the line that reports the common stretch."""
    if rank != 0:
        return
    torch.save({'lo': torch.from_numpy(np.asarray(lo, np.float32).copy()), 'hi': torch.from_numpy(np.asarray(hi, np.float32).copy()),
                'q': torch.tensor([1.0, 99.0]), 'n_valid': int(n_valid), 'images': list(request)}, Path(output_dir) / 'stretch.pt')
    print(f'common stretch over {len(request)} images, {int(n_valid)} valid pixels: '
          + ', '.join(f'{name} lo {lo[c]:.6g} hi {hi[c]:.6g}' for c, name in enumerate('RGB')))


def _write_applied(image: sfm.Image, J: Tensor, water: dict, light_model: bool, output_dir: Path, device, stretch=None) -> None:
    """``<stem>_rgb.png``, ``<name>.pt`` and, with the light model, ``<stem>_vignetting.png`` of one inverted image.  No
    ``_reconstruction.png``: the reconstruction of a single-view inversion is the input image."""
    sucre = SUCRe(image=image, light_model=light_model, use_closed_form=True)
    sucre.load_state_dict(water, strict=True)
    sucre.J = J
    sucre.stretch = stretch
    stem = Path(image.name).stem
    _save_png(sucre.plot_J(), output_dir / f'{stem}_rgb.png')
    if light_model:
        _save_png(sucre.to(device).plot_l(), output_dir / f'{stem}_vignetting.png')
    torch.save({**sucre.cpu().state_dict(), 'J': J.detach().cpu()}, (output_dir / image.name).with_suffix('.pt'))


def apply_water(images: list, colmap_model: sfm.COLMAPModel, output_dir: Path, water, light_model: bool = False,
                device: str = 'cuda', in_flight: int = 2, stretch=None, request: list | None = None, rank: int = 0) -> None:
    """Restores ``images`` (``sfm.Image`` objects or names of ``colmap_model``) with GIVEN water parameters instead of fitting
    them: per image ``J = (I - l B (1 - e^(-gamma z))) a / a^2``, ``a = l e^(-beta z)``, from the image's own depth map
    (``engine.invert_images``: ``update_J`` with the image as its only observation).  ``water``: a mapping with ``B, beta,
    gamma`` (3,1) -- and ``cam2light`` (6), ``sigma`` (2,2) with ``light_model`` -- e.g. a loaded ``shared_water.pt`` or
    ``<name>.pt``, or the path of one.  Only the target images are decoded (the next launch's while this one's run); nothing is
    matched and no workspace is allocated.  Up to 32 images go into one launch on one of ``in_flight`` slots, and the
    output files -- ``<stem>_rgb.png``, ``<name>.pt`` (the parameters and J), ``<stem>_vignetting.png`` with the light model --
    are written by background threads.  ``stretch``: ``None`` -- every ``_rgb.png`` by its own percentiles, as the reference
    does; ``(lo, hi)`` -- by this fixed stretch (``check_stretch``; --stretch-from); ``'common'`` -- by the 1st and 99th percentile
    of the pool of the valid pixels of ALL images (of all ranks, when a process group is up: ``common_stretch``): the J of this
    rank's images then stay on the device and the files are written once the pool is complete; rank 0 (``rank``) also writes
    ``stretch.pt`` (``lo, hi, q, n_valid, images``: ``request``, the names of all ranks' images) for --stretch-from."""
    from . import engine
    sfm.require_gpu(device, 'apply_water')
    common = isinstance(stretch, str)
    if common and stretch != 'common':
        raise ValueError(f"apply_water: stretch is None, 'common' or a (lo, hi) pair, not {stretch!r}")
    if stretch is not None and not common:
        stretch = check_stretch(stretch)
    if isinstance(water, (str, Path)):
        water = torch.load(water, map_location='cpu')
    water = check_water(water, light_model)
    params = torch.cat([water[k].flatten() for k in water_shapes(light_model)]).numpy()
    images = [colmap_model[im] if isinstance(im, str) else im for im in images]
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    in_flight = max(1, int(in_flight))
    if common:
        _check_stretch_memory(images, device)
    held: list = []   # 'common': (image, J) of this rank until the pool is complete
    chunks = [images[i:i + APPLY_IMAGES_PER_LAUNCH] for i in range(0, len(images), APPLY_IMAGES_PER_LAUNCH)]
    if chunks:
        loader.prefetch_device_views(chunks[0], device, background=True)
    pending: list = []
    written = []
    with ThreadPoolExecutor(max_workers=max(1, int(os.environ.get('SUCRE_WRITER_THREADS', min(32, loader.effective_cpus() - 2)))),
                            thread_name_prefix='sucre-write') as writers:
        def finish(slot, chunk, Js):
            with engine.in_flight_slot(slot, device, wait_for_caller=False):
                torch.cuda.current_stream().synchronize()   # the writer threads work on another stream
            if common:
                held.extend(zip(chunk, Js))
                return
            for image, J in zip(chunk, Js):
                written.append(writers.submit(_write_applied, image, J, water, light_model, output_dir, device, stretch))
            while len(written) > 64:   # bound the memory held by queued outputs
                written.pop(0).result()

        for c, chunk in enumerate(chunks):
            slot = c % in_flight
            while pending and (len(pending) >= in_flight or pending[0][0] == slot):
                finish(*pending.pop(0))
            if c + 1 < len(chunks):
                loader.prefetch_device_views(chunks[c + 1], device, background=True)
            for image in chunk:
                print(f'Restore {image.name} (given water parameters).')
            views = [image.device_view(device) for image in chunk]   # waits only for an image that is still being decoded
            with engine.in_flight_slot(slot, device, wait_for_caller=False):   # inputs: Image.device_view, complete
                Js = engine.invert_images(views, params, light=light_model)
            pending.append((slot, chunk, Js))
        for item in pending:
            finish(*item)
        if common:   # every rank takes part, also one without an image
            with torch.cuda.device(device):
                lo, hi, n_valid = common_stretch([J for _, J in held])
            _write_common_stretch(output_dir, lo, hi, n_valid, request if request is not None else [im.name for im in images], rank)
            for image, J in held:
                written.append(writers.submit(_write_applied, image, J, water, light_model, output_dir, device, (lo, hi)))
                while len(written) > 64:
                    written.pop(0).result()
            held.clear()
        for f in written:
            f.result()   # re-raises anything a writer thread hit


# ---- --check-consistency: do the restored images agree where they see the same seabed? ------------------------------------

def consistency_summary(stats, H: int, W: int, min_cover: float) -> dict:
    """What the per-view rows of ``engine.view_consistency`` say, in float64 numpy.  Per view: ``kept`` -- the cover rule of
    sfm.py:136 on the matches, ``stats[:, 0] / (W H) > min_cover``; ``n`` -- valid pairs; ``rms_restored`` and ``rms_raw`` (n_views, 3)
    -- ``sqrt(sum d^2 / n)`` of the restored and of the raw colours; ``gain`` -- ``sum a b / sum b^2``, the brightness ratio target :
    view per channel (1 where ``sum b^2`` is not positive); ``rms_restored_gain`` -- ``sqrt(max(0, sum a^2 - (sum a b)^2 / sum b^2) / n)``,
    what a gain per pair could not remove: the part no common stretch can fix.  A view without a valid pair has zeros (gain 1).
    ``pooled_restored``, ``pooled_raw``, ``pooled_restored_gain`` (3,): ``sqrt(sum sum d^2 / sum n)`` over the kept views, and
    ``pooled_n``, their pairs."""
    stats = np.asarray(stats, np.float64).reshape(-1, 26)
    n = stats[:, 1]
    kept = stats[:, 0] / (int(W) * int(H)) > min_cover
    nn = np.where(n > 0, n, 1.0)[:, None]
    sd, saa, sbb, sab = (stats[:, 2 + 3 * i:5 + 3 * i] for i in range(4))
    positive = sbb > 0
    safe = np.where(positive, sbb, 1.0)
    left = np.where(positive, np.maximum(0.0, saa - sab * sab / safe), saa)   # sum (a - g b)^2 at the best g
    pooled_n = float(n[kept].sum())

    def pooled(s):
        return np.sqrt(s[kept].sum(axis=0) / pooled_n) if pooled_n > 0 else np.zeros(3)

    return {'kept': kept, 'n_matches': stats[:, 0].copy(), 'n': n.copy(),
            'rms_restored': np.sqrt(sd / nn), 'rms_raw': np.sqrt(stats[:, 14:17] / nn),
            'gain': np.where(positive, sab / safe, 1.0), 'rms_restored_gain': np.sqrt(left / nn),
            'pooled_restored': pooled(sd), 'pooled_raw': pooled(stats[:, 14:17]), 'pooled_restored_gain': pooled(left),
            'pooled_n': pooled_n}


def merge_consistency(records: list, request: list, min_cover: float) -> dict:
    """The survey's ``consistency.pt`` from the targets' records -- ``{'target', 'views', 'stats', 'H', 'W'}``, in any order and
    however they were split over ranks: the targets are taken in ``request`` order, so the result does not depend on the world
    size.  One row per directed kept pair (a, b) with a valid pixel pair: ``n``, ``rms_restored``, ``rms_raw``, ``gain``,
    ``rms_restored_gain``; the pooled figures are ``sqrt(sum sum d^2 / sum n)`` over all rows."""
    order = {name: i for i, name in enumerate(request)}
    records = sorted(records, key=lambda r: order[r['target']])
    a, b, n = [], [], []
    cols = {k: [] for k in ('rms_restored', 'rms_raw', 'gain', 'rms_restored_gain')}
    sums = np.zeros((3, 3))   # sum d^2 of the restored, the raw and the gain-compensated colours
    for r in records:
        stats = np.asarray(r['stats'], np.float64).reshape(-1, 26)
        s = consistency_summary(stats, r['H'], r['W'], min_cover)
        for k in np.nonzero(s['kept'] & (s['n'] > 0))[0]:
            a.append(r['target']); b.append(r['views'][k]); n.append(int(round(s['n'][k])))
            for key in cols:
                cols[key].append(s[key][k])
            sums[0] += stats[k, 2:5]
            sums[1] += stats[k, 14:17]
            sums[2] += s['rms_restored_gain'][k] ** 2 * s['n'][k]
    total = float(sum(n))
    pooled = np.sqrt(sums / total) if total > 0 else np.zeros((3, 3))
    out = {'a': a, 'b': b, 'n': torch.tensor(n, dtype=torch.int64), 'images': list(request), 'targets': [r['target'] for r in records],
           'min_cover': float(min_cover), 'pooled_n': int(total), 'pooled_restored': torch.from_numpy(pooled[0].copy()),
           'pooled_raw': torch.from_numpy(pooled[1].copy()), 'pooled_restored_gain': torch.from_numpy(pooled[2].copy())}
    for key, rows in cols.items():
        out[key] = torch.from_numpy(np.asarray(rows, np.float64).reshape(-1, 3))
    return out


def _consistency_file(results_dir: Path, image) -> Path:
    return (Path(results_dir) / image.name).with_suffix('.pt')   # sucre.py:213-215


def _read_restored(path: Path, image, lazy: bool = False, flag: str = '--check-consistency') -> Tensor:
    """``J`` of a result file, checked against the image's camera.  ``lazy``: only the shape is wanted -- the file is mapped, not
    read, where torch can (a zip archive, what torch.save writes).  ``flag``: the mode that asks, named in the refusals."""
    try:
        try:
            data = torch.load(path, map_location='cpu', mmap=True) if lazy else torch.load(path, map_location='cpu')
        except (RuntimeError, ValueError, TypeError):
            if not lazy:
                raise
            data = torch.load(path, map_location='cpu')
        J = data['J']
    except Exception as e:
        raise SystemExit(f'{flag}: cannot read J from {path}: {e}')
    want = (int(image.camera.height), int(image.camera.width), 3)
    if not torch.is_tensor(J) or tuple(J.shape) != want:
        raise SystemExit(f'{flag}: J of {path} has shape {tuple(J.shape) if torch.is_tensor(J) else type(J).__name__}, '
                         f'but the camera of {image.name} is {want[1]}x{want[0]}: (H, W, 3) = {want} expected')
    return J


def consistency_cache_budget(device) -> int:
    """Bytes of restored images (12 per pixel) --check-consistency keeps on the device across targets:
    SUCRE_CONSISTENCY_CACHE_GB, by default a quarter of the device's memory (the pixel cache of sfm.py takes up to half)."""
    gb = os.environ.get('SUCRE_CONSISTENCY_CACHE_GB')
    if gb is not None:
        return int(float(gb) * 2 ** 30)
    return int(torch.cuda.mem_get_info(device)[1]) // 4


class _RestoredCache:
    """The restored images on the device, least recently used dropped first once ``budget`` bytes are exceeded; the images
    named in ``pinned`` (the current target and its neighbours) are never dropped."""

    def __init__(self, results_dir: Path, device, budget: int, flag: str = '--check-consistency'):
        self.results_dir, self.device, self.budget, self.flag = Path(results_dir), device, int(budget), flag
        self.entries: 'collections.OrderedDict[str, Tensor]' = collections.OrderedDict()
        self.total = 0

    @staticmethod
    def nbytes(image) -> int:
        return int(image.camera.height) * int(image.camera.width) * 12

    def get(self, image, pinned: set) -> Tensor:
        J = self.entries.get(image.name)
        if J is not None:
            self.entries.move_to_end(image.name)
            return J
        need = self.nbytes(image)
        for name in [k for k in self.entries if k not in pinned]:
            if self.total + need <= self.budget:
                break
            self.total -= self.entries.pop(name).numel() * 4
        named = {} if self.flag == '--check-consistency' else {'flag': self.flag}
        J = _read_restored(_consistency_file(self.results_dir, image), image, **named).to(torch.float32).contiguous().to(self.device)
        self.entries[image.name] = J
        self.total += need
        return J


def _write_consistency(image, views: list, count, ssd, stats, min_cover: float, output_dir: Path) -> dict:
    """``<stem>_consistency.pt``, ``<stem>_consistency.png`` and the printed line of one target; returns its record."""
    H, W = int(image.camera.height), int(image.camera.width)
    s = consistency_summary(stats.numpy(), H, W, min_cover)
    stem = Path(image.name).stem
    torch.save({'views': list(views), 'stats': stats, 'kept': torch.from_numpy(s['kept'].copy()), 'count': count, 'ssd': ssd,
                'min_cover': float(min_cover), 'pooled_n': int(s['pooled_n']),
                **{k: torch.from_numpy(np.ascontiguousarray(s[k])) for k in ('n_matches', 'n', 'rms_restored', 'rms_raw', 'gain',
                                                                             'rms_restored_gain', 'pooled_restored', 'pooled_raw',
                                                                             'pooled_restored_gain')}},
               output_dir / f'{stem}_consistency.pt')
    _save_png(PILImage.fromarray(residual_image(count.numpy(), ssd.numpy())), output_dir / f'{stem}_consistency.png')
    r, raw = s['pooled_restored'], s['pooled_raw']
    line = (f'{image.name}: consistency with {int(s["kept"].sum())} views over {int(s["pooled_n"])} pixel pairs: restored RMS '
            f'R {r[0]:.4f} G {r[1]:.4f} B {r[2]:.4f} (raw R {raw[0]:.4f} G {raw[1]:.4f} B {raw[2]:.4f})')
    per_view = np.sqrt((s['rms_restored'] ** 2).mean(axis=1))   # sqrt(sum_c sum d^2 / (3 n))
    per_view[~(s['kept'] & (s['n'] > 0))] = -1.0
    if (per_view >= 0).any():
        worst = int(per_view.argmax())
        line += f'; least consistent with {views[worst]} (RMS {per_view[worst]:.4f})'
    print(line)
    return {'target': image.name, 'views': list(views), 'stats': stats.numpy().copy(), 'H': H, 'W': W}


def check_consistency(images: list, colmap_model: sfm.COLMAPModel, results_dir: Path, output_dir: Path, image_list: list | None = None,
                      min_cover: float = 0.000001, device: str = 'cuda', request: list | None = None, rank: int = 0,
                      num_workers: int = 0) -> dict | None:
    """Cross-view colour consistency of a finished restoration: for every image of ``images`` (``sfm.Image`` objects or names of
    ``colmap_model``) its restored ``J`` -- ``results_dir / <name>.pt``, key ``J``, what this project and the reference write --
    is compared with the ``J`` of every other image of ``image_list`` (the model's images unless given) that has such a file,
    on the pixels the two-way match of their depth maps pairs (``engine.view_consistency``).  Nothing is fitted.  The
    neighbours keep ``image_list`` order, go through ``overlapping_views`` unless SUCRE_CULL_VIEWS=0 and are capped at
    ``engine.MAX_VIEWS``; images of ``image_list`` without a file are skipped and counted.  Every target's file is checked
    before any image is decoded: a missing one, or a ``J`` (of a target or of a neighbour) that is not (H, W, 3) of its camera,
    stops the run naming it.  The restored images stay on the device across targets, least recently used dropped first, within
    ``consistency_cache_budget``; a target whose own neighbours exceed it is refused.  Per target: ``<stem>_consistency.pt``
    (``views, stats, kept, count, ssd, min_cover`` and the arrays of ``consistency_summary``), ``<stem>_consistency.png``
    (``residual_image`` of the squared differences) and one line.  Every rank takes part in the gather of the records (when a
    process group is up); rank 0 writes ``consistency.pt`` (``merge_consistency``), prints the survey's line and returns the
    merged dictionary, the others return None."""
    from . import engine
    sfm.require_gpu(device, 'check_consistency')
    images = [colmap_model[im] if isinstance(im, str) else im for im in images]
    image_list = list(colmap_model.images.values()) if image_list is None else list(image_list)
    results_dir, output_dir = Path(results_dir), Path(output_dir)
    for image in images:   # before anything is decoded
        path = _consistency_file(results_dir, image)
        if not path.is_file():
            raise SystemExit(f'--check-consistency: {path} is missing: {image.name} has no restored image in {results_dir}')
    have = [im for im in image_list if _consistency_file(results_dir, im).is_file()]
    n_without = len(image_list) - len(have)
    for image in {im.name: im for im in images + have}.values():
        _read_restored(_consistency_file(results_dir, image), image, lazy=True)
    if n_without:
        print(f'--check-consistency: {n_without} of {len(image_list)} images have no restored image in {results_dir} and are skipped.')
    output_dir.mkdir(parents=True, exist_ok=True)
    cull = os.environ.get('SUCRE_CULL_VIEWS', '1') != '0'
    if images:
        loader.prefetch_for_targets(images, have, device, num_workers=num_workers, min_cover=0.0 if cull else -1.0)
    cache = _RestoredCache(results_dir, device, consistency_cache_budget(device))
    records = []
    for image in images:
        others = [im for im in have if im.name != image.name]
        if cull and len(others) > 1:
            others = [others[i] for i in image.overlapping_views(others, device)]
        others = others[:engine.MAX_VIEWS]
        if not others:
            raise SystemExit(f'--check-consistency: {image.name} has no neighbour with a restored image in {results_dir}')
        need = sum(cache.nbytes(im) for im in others + [image])
        if need > cache.budget:
            raise SystemExit(f'--check-consistency: the restored images of {image.name} and its {len(others)} neighbours take {need} '
                             f'bytes, more than the {cache.budget} bytes kept on {device} (SUCRE_CONSISTENCY_CACHE_GB); list images '
                             f'to leave out in --filter-images-path')
        pinned = {im.name for im in others} | {image.name}
        with torch.cuda.device(device):
            J = cache.get(image, pinned)
            Js = [cache.get(im, pinned) for im in others]
            target = image.device_view(device)
            views = [im.device_view(device) for im in others]
            count, ssd, stats = engine.view_consistency(target, J, views, Js)
            count, ssd, stats = count.cpu(), ssd.cpu(), stats.cpu()
        records.append(_write_consistency(image, [im.name for im in others], count, ssd, stats, min_cover, output_dir))
    gathered = [r for part in sdist.all_gather_objects(records) for r in part]
    if rank != 0:
        return None
    request = list(request) if request is not None else [im.name for im in images]
    merged = merge_consistency(gathered, request, min_cover)
    torch.save(merged, output_dir / 'consistency.pt')
    r, raw = merged['pooled_restored'].numpy(), merged['pooled_raw'].numpy()
    print(f'consistency over {len(merged["a"])} pairs of {len(merged["targets"])} images: restored RMS R {r[0]:.4f} G {r[1]:.4f} '
          f'B {r[2]:.4f}, raw R {raw[0]:.4f} G {raw[1]:.4f} B {raw[2]:.4f}')
    return merged


# ---- --mosaic: one georeferenced picture of the seabed from the restored images ---------------------------------------------

MOSAIC_IMAGES_PER_CALL = 32   # images per phase call: one launch each (csrc/mosaic.h)


def _rotation_of(image) -> np.ndarray:
    R = image.pose.R if hasattr(image, 'pose') else image.R
    return np.asarray(R.detach().cpu().numpy() if torch.is_tensor(R) else R, np.float64).reshape(3, 3)


def mosaic_axes(images: list) -> Tensor:
    """The default frame of a mosaic, (3,3) float32 with rows e1, e2, e3, from the world-from-camera rotations of ``images``
    (``sfm.Image`` objects, or anything with ``R``): e3 is the normalised mean of the cameras' optical axes ``R[:, 2]`` -- the
    mosaic looks the way the cameras look --, e1 the first image's ``R[:, 0]`` with its e3 component removed, normalised
    (``R[:, 1]`` instead, when less than 1e-6 of it remains), e2 = e3 x e1.  Computed in float64, rounded once."""
    Rs = [_rotation_of(im) for im in images]
    if not Rs:
        raise ValueError('mosaic_axes: no image')
    mean = np.sum([R[:, 2] for R in Rs], axis=0) / len(Rs)
    length = np.linalg.norm(mean)
    if not length > 1e-6:
        raise ValueError('mosaic_axes: the cameras\' optical axes cancel out; give the axes')
    e3 = mean / length
    for column in (0, 1):
        e1 = Rs[0][:, column] - np.dot(Rs[0][:, column], e3) * e3
        if np.linalg.norm(e1) >= 1e-6:
            break
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(e3, e1)
    return torch.from_numpy(np.stack([e1, e2, e3]).astype(np.float32))


def mosaic_default_gsd(depths: list, fxs: list) -> np.float32:
    """``float32(2 median_i(median(valid depths of image i) / fx_i))`` in float64: twice the footprint of a typical pixel, so
    that a typical cell is hit by a few pixels of every image that sees it.  ``depths``: the decoded depth maps (tensors or
    arrays, <= 0: invalid); images without a valid depth are left out."""
    per_image = []
    for d, fx in zip(depths, fxs):
        d = np.asarray(d.detach().cpu().numpy() if torch.is_tensor(d) else d, np.float64)
        d = d[d > 0]
        if d.size:
            per_image.append(np.median(d) / float(fx))
    if not per_image:
        raise ValueError('mosaic_default_gsd: no image has a valid depth')
    return np.float32(2.0 * np.median(np.asarray(per_image, np.float64)))


def mosaic_source_picture(source: np.ndarray) -> np.ndarray:
    """(Hm,Wm,3) uint8: every ordinal hashed to a colour of its own (channels in 64..255), empty cells black."""
    source = np.asarray(source)
    h = ((source.astype(np.int64) + 1) * 2654435761) & 0xffffffff
    h ^= h >> 15
    out = np.stack([64 + ((h >> s) & 0xff) * 191 // 255 for s in (0, 8, 16)], axis=-1).astype(np.uint8)
    out[source < 0] = 0
    return out


def mosaic_fill_mask(level: np.ndarray) -> np.ndarray:
    """(Hm,Wm) uint8 of a mosaic's ``fill_level``: 255 measured, 128 filled, 0 empty."""
    return np.where(level == 0, 255, np.where(level > 0, 128, 0)).astype(np.uint8)


def mosaic_surface_picture(surface: np.ndarray) -> np.ndarray:
    """(Hm,Wm) uint8 of a mosaic's ``surface``: a filled cell (no NaN) gets ``1 + rint(254 (smax - s) / (smax - smin))`` in float64
    over the filled cells -- the highest ground, the smallest coordinate along the view axis, is white --, 255 when the surface is
    flat; an empty cell 0."""
    s = np.asarray(surface, dtype=np.float64)
    filled = ~np.isnan(s)
    out = np.zeros(s.shape, np.uint8)
    if filled.any():
        smin, smax = s[filled].min(), s[filled].max()
        out[filled] = 255 if smax == smin else (1 + np.rint(254.0 * (smax - s[filled]) / (smax - smin))).astype(np.uint8)
    return out


def mosaic_culled_picture(culled: np.ndarray) -> np.ndarray:
    """(Hm,Wm) uint8 of a mosaic's ``culled``: ``255 culled // max(1, culled.max())``."""
    c = np.asarray(culled).astype(np.int64)
    return (255 * c // max(1, int(c.max(initial=0)))).astype(np.uint8)


def _mosaic_picture(J: Tensor, stretch) -> np.ndarray:
    """(Hm,Wm,3) uint8 of a mosaic's ``J`` on the device: the fixed ``stretch`` when given, ``plot_J``'s own percentiles over the
    filled cells otherwise."""
    from . import engine
    if stretch is not None:
        return engine.plot_stretch(J, *stretch).cpu().numpy()
    if _NUMPY_2:
        return _plot_J_on_device(J).cpu().numpy()
    J = J.cpu().numpy().copy()   # numpy 1.x: np.percentile itself, as plot_J does there
    ok = ~np.isnan(J).any(axis=2)
    vals = J[ok]
    lo, hi = np.percentile(vals, 1, axis=0), np.percentile(vals, 99, axis=0)
    vals = np.clip(vals, lo, hi)
    vals = vals - vals.min(axis=0)
    vals = vals / vals.max(axis=0)
    J[~ok] = 0.0
    J[ok] = vals
    return np.uint8(J * 255)


_MOSAIC_FLAG = {'grid': '--mosaic', 'blend': '--mosaic-blend', 'fill': '--mosaic-fill', 'feather': '--mosaic-feather',
                'bands': '--mosaic-bands', 'surface': '--mosaic-surface', 'support': '--mosaic-support', 'gains': '--mosaic-gains',
                'gain_limit': '--mosaic-gain-limit', 'gain_solve': '--mosaic-gain-solve', 'reject': '--mosaic-reject'}


def _mosaic_refused(e: ValueError, fields=tuple(_MOSAIC_FLAG)) -> BaseException:
    """The SystemExit that names the flag of the ``field`` of an engine's mosaic refusal; ``e`` itself when it has none of ``fields``."""
    field = getattr(e, 'field', None)
    return SystemExit(f'{_MOSAIC_FLAG[field]}: {e}') if field in fields else e


_MOSAIC_PNG = {   # how a row of engine.MOSAIC_OUTPUTS becomes its PNG: (the output on the device, the stretch) -> uint8 array
    'stretch': _mosaic_picture,
    'bytes': lambda t, stretch: t.cpu().numpy(),
    'source': lambda t, stretch: mosaic_source_picture(t.cpu().numpy()),
    'mask': lambda t, stretch: mosaic_fill_mask(t.cpu().numpy()),
    'height': lambda t, stretch: mosaic_surface_picture(t.cpu().numpy()),
    'count': lambda t, stretch: mosaic_culled_picture(t.cpu().numpy()),
}


def mosaic(images: list, colmap_model: sfm.COLMAPModel, results_dir: Path, output_dir: Path, gsd: float | None = None, axes=None,
           stretch=None, device: str = 'cuda', blend: float | None = None, fill: float | None = None, feather: int | None = None,
           bands: int | None = None, surface: float | None = None, support: int | None = None, gains: int | None = None,
           gain_limit: float | None = None, reject: float | None = None, gain_solve: str | None = None) -> dict:
    """One picture of the seabed from a finished restoration: every pixel of ``images`` (``sfm.Image`` objects or names of
    ``colmap_model``; at most ``engine.MAX_VIEWS``, ordinal = position) with a valid depth and a restored colour --
    ``results_dir / <name>.pt``, key ``J`` -- is dropped onto the plane grid ``axes`` (``mosaic_axes`` unless given) of ``gsd``
    metres per cell (``mosaic_default_gsd`` unless given; printed), and the pixel seen through the least water wins its cell
    (``engine.Mosaic``; csrc/mosaic.h).  Holes stay empty unless ``fill`` is given.  Every file is checked before any image is decoded.
    Every option below is a field of one ``engine.MosaicOptions``, built and checked here once; the images are cut into batches here (at most
    ``MOSAIC_IMAGES_PER_CALL``, and what fits the cache together) and ``engine.Mosaic.run`` takes every phase over every batch.  The
    restored images stay on the device across the four phases within ``consistency_cache_budget`` and are read again per phase
    otherwise: the same bits either way.  The PNGs are those of the rows of ``engine.MOSAIC_OUTPUTS``.  Writes ``mosaic.png``
    (``plot_J``'s stretch over the filled cells, or the fixed ``stretch``), ``mosaic_raw.png``, ``mosaic_source.png`` (``mosaic_source_picture``) and ``mosaic.pt`` (``J, raw, source, pixel,
    range, axes, gsd, lo, images, n_filled, per_image``), prints one line and returns the dictionary of ``mosaic.pt``.

    ``blend``: a blend depth H in metres (``engine.MOSAIC_BLEND_RANGE``).  One more pass over the batches then sums, per cell, ALL
    its pixels in fixed point, each with the weight ``max(1 - (z - zmin) / H, 0)^2`` of its range z over the cell's smallest one,
    and a pass over the cells divides (csrc/mosaic.h, "The blend": the same bits in any order).  The four files above stay the
    best-view ones, byte for byte -- their seams are the diagnostic --; ``mosaic_blend.png`` (``J_blend`` through the function that
    makes ``mosaic.png``) and ``mosaic_blend_raw.png`` come next to them, ``mosaic.pt`` gains ``J_blend, raw_blend, weight, samples,
    blend`` and one more line is printed.

    ``fill``: a reach R in metres (``engine.MOSAIC_FILL_RANGE``).  After the other phases a bounded push-pull over a pyramid of
    the grid (``engine.Mosaic.fill``; csrc/fill.h) closes every hole up to R across and does not extrapolate far beyond the
    footprint.  Every file and key above stays as it is, byte for byte; ``mosaic_filled.png`` (``J_filled`` through the function
    that makes ``mosaic.png``: its own percentiles, or ``stretch``), ``mosaic_raw_filled.png`` and ``mosaic_filled_mask.png`` (255
    measured, 128 filled, 0 empty) come next to them -- with a blend also ``mosaic_blend_filled.png`` and
    ``mosaic_blend_raw_filled.png`` --, ``mosaic.pt`` gains ``J_filled, raw_filled, fill_level`` (``J_blend_filled,
    raw_blend_filled``), ``fill`` and ``fill_levels``, and one more line is printed.

    ``feather``: with ``blend``, a feather width F in source pixels (``engine.MOSAIC_FEATHER_RANGE``).  Every sample's weight then
    takes one more factor, ``min(sqrt(dist2) / F, 1)`` of its distance to the nearest pixel of its image that does not take part or
    lies outside it -- an exact integer map made on the device per batch (csrc/mosaic.h, "The feather") --, so the blend fades
    out towards the edge of every footprint, NaN patch and depth hole and does not step there.  The blended files and keys are then
    the feathered ones (a fill fills from them); the best-view ones stay as they are, byte for byte; ``mosaic.pt`` gains
    ``feather`` and one more line is printed after the blend's (its share "within F px of an edge" is counted over the pixels that
    take part, ``engine.Mosaic.feather_counts``, whether or not their weight rounds to nothing).

    ``bands``: with ``blend``, the number K of detail bands (``engine.MOSAIC_BANDS_RANGE``) of a multi-band blend next to the blend.
    Every image is split in source space into K detail bands and a residual (csrc/bands.h), one more pass over the batches
    blends every band with the blend's own fixed-point sums -- the residual with ``(H, F)``, every finer band with half the depth
    and half the feather of the one before (``engine.mosaic_band_plan``) --, and a pass over the cells adds them: the colour of the
    blend with the detail of the best view.  Every file and key above stays as it is, byte for byte; ``mosaic_multiband.png``
    (``J_multiband`` through the function that makes ``mosaic.png``) comes next to them -- with a fill also
    ``mosaic_multiband_filled.png`` --, ``mosaic.pt`` gains ``J_multiband`` (``J_multiband_filled``), ``bands`` and ``band_plan``,
    the list of ``(H_j, F_j)``, and one more line is printed after the blend's and the feather's.  Not built: a multi-band raw
    mosaic.

    ``surface``: a tolerance T in metres (``engine.MOSAIC_SURFACE_RANGE``) of a surface test ahead of every phase above
    (csrc/surface.h).  One more pass over the batches finds, per cell, the highest sample along the mosaic's view axis ``e3`` -- the
    smallest ``e3 . wP`` --, and a sample that lies more than T below its cell's top takes part in nothing: the lower of two
    surfaces no longer wins a cell because a camera is close to it, and the blend no longer mixes two layers.  The grid and the set
    of filled cells are those of a run without the flag, and a T that culls nothing leaves every file and key above as it is, byte
    for byte.  ``mosaic_surface.png`` (``mosaic_surface_picture``: the height, highest ground white) and ``mosaic_culled.png``
    (``mosaic_culled_picture``) come next to the other files, ``mosaic.pt`` gains ``surface``, ``culled`` and ``surface_tol``, and one
    more line is printed after the mosaic's.  The surface is a plain minimum: one spurious high sample owns its cell; ``support``
    is the remedy.

    ``support``: with ``surface``, the number M of views (``engine.MOSAIC_SUPPORT_RANGE``) the top of a cell must rest on
    (csrc/support.h): the highest level that at least M different images reach -- a view listed twice has two ordinals and counts
    twice; a cell seen by fewer than M images rests on the lowest of its per-image tops --, found in M passes over the batches, and
    a sample that stands more than T ABOVE it takes part in nothing either: a fish in one view's depth map no longer owns its cells.
    The filled cells stay those of a run without the flag, and ``support=1`` is the surface test bit for bit.
    ``mosaic_culled_above.png`` (``mosaic_culled_picture`` of ``culled_above``) comes next to the other files, ``mosaic.pt`` gains
    ``support``, ``surface_source``, ``culled_above``, ``surface_top`` and ``surface_support``, ``surface`` is the supported top, and
    one more line is printed after the surface's.  The limit: an error that M or more images share passes, and a real feature that
    one image alone sees more than T above what M images agree on is removed.  Not built: the single-pass k-smallest form.

    ``gains``: the rounds R (``engine.MOSAIC_GAIN_ROUNDS_RANGE``) of a per-image gain compensation between the splat and every later
    phase (csrc/gains_mosaic.h): one gain per image and channel, found from the cells that two or more images share, so that images
    restored with a water model each agree on the colour of the same seabed; ``gain_limit``: with ``gains``, the limit L
    (``engine.MOSAIC_GAIN_LIMIT_RANGE``, ``engine.MOSAIC_GAIN_LIMIT`` unless given) -- every gain lies within [1 / L, L].  Every file
    and key that is not a ``J`` stays as it is, byte for byte; every ``J`` is that of a run without the flag on the images times
    their gains; ``mosaic.pt`` gains ``gains``, ``gain_sums``, ``gain_rms``, ``gain_overlap``, ``gain_rounds`` and ``gain_limit``, and
    one more line is printed after the mosaic's and the surface's.  The rounds remove what overlapping images disagree on; a slow
    drift along a chain of N images needs on the order of N^2 rounds and is not what the rounds are for.

    ``gain_solve``: with ``gains``, 'direct' (``engine.MOSAIC_GAIN_SOLVES``) -- the rounds' objective solved exactly, once, in place of
    the first round's solve (csrc/gains_direct.h): per shared cell the colour sums of up to eight images, from them one sum per pair of
    overlapping images, and one n x n solve per channel on the host with a weak prior towards gain 1.  It removes the drift along a
    chain -- a lawn-mower transect under a drifting strobe -- that no affordable number of rounds removes; the remaining R - 1 rounds
    and the measuring pass run unchanged from its table, so ``gain_rms[1]`` shows what it achieved.  A shared cell that more than
    eight images reach is left out of the solve.  ``mosaic.pt`` gains ``gain_solve``, ``gain_direct``, ``gain_pair_index``,
    ``gain_pair_words``, ``gain_diag``, ``gain_excluded_cells``, ``gain_shared_cells``, ``gain_kept``, ``gain_components`` and
    ``gain_prior``, and one more line is printed
    after the gains'.  'rounds' or None: the rounds alone, every file as without the argument.

    ``reject``: a tolerance T in units of ``J`` (``engine.MOSAIC_REJECT_RANGE``) of a colour consensus across views ahead of the
    splat (csrc/reject.h).  The depth maps are rendered from the reconstruction, so a fish, a fin, a caustic band or a particle cloud
    carries the seabed's height and its own colour: no height test sees it.  Per cell the images that reach it -- the eight earliest
    when there are more -- are ordered by their mean brightness there, the median one is the cell's reference, and a sample of another
    image that differs from the reference's mean colour by more than T in any channel takes part in nothing from the splat on, the
    gain compensation included.  A cell that fewer than three images reach rejects nothing, and the reference's own samples never go:
    the grid and the filled cells stay those of a run without the argument, and a T that rejects nothing leaves every other file and
    key byte for byte.  T must exceed the offsets between images that ``gains`` is to remove afterwards: there is no second
    rejection.  ``mosaic_rejected.png`` (``mosaic_culled_picture`` of the counts) comes next to the other files, ``mosaic.pt`` gains
    ``rejected``, ``reject_ref``, ``reject_source``, ``reject_views``, ``reject_overflow``, ``reject_per_image`` and ``reject_tol``,
    and one more line is printed after the surface's and the support's."""
    from . import engine
    sfm.require_gpu(device, 'mosaic')
    images = [colmap_model[im] if isinstance(im, str) else im for im in images]
    if not images:
        raise SystemExit('--mosaic: no image in the request')
    if len(images) > engine.MAX_VIEWS:
        raise SystemExit(f'--mosaic: {len(images)} images in the request, at most {engine.MAX_VIEWS} go into one mosaic')
    if stretch is not None:
        stretch = check_stretch(stretch)
    try:
        options = engine.MosaicOptions(blend=blend, feather=feather, fill=fill, bands=bands, surface=surface, support=support, gains=gains,
                                       gain_limit=gain_limit, gain_solve=gain_solve, reject=reject).checked('mosaic')
    except ValueError as e:
        if e.needs is not None:   # an option without the one it goes with: in the command line's words
            raise SystemExit(f'{_MOSAIC_FLAG[e.field]}: only with {_MOSAIC_FLAG[e.needs]} {engine.MOSAIC_VALUES[e.needs][5]}')
        raise _mosaic_refused(e)
    blend, feather, fill, bands, surface, support = (options.blend, options.feather, options.fill, options.bands, options.surface,
                                                     options.support)
    gains, gain_limit, gain_solve, reject = options.gains, options.gain_limit, options.gain_solve, options.reject
    results_dir, output_dir = Path(results_dir), Path(output_dir)
    for image in images:   # before anything is decoded
        path = _consistency_file(results_dir, image)
        if not path.is_file():
            raise SystemExit(f'--mosaic: {path} is missing: {image.name} has no restored image in {results_dir}')
    for image in images:
        _read_restored(_consistency_file(results_dir, image), image, lazy=True, flag='--mosaic')
    output_dir.mkdir(parents=True, exist_ok=True)
    axes = mosaic_axes(images) if axes is None else torch.as_tensor(axes, dtype=torch.float32).reshape(3, 3)
    cache = _RestoredCache(results_dir, device, consistency_cache_budget(device), flag='--mosaic')
    batches = []   # (ordinal of the first image, images): consecutive images, at most 32, whose restored images fit the cache together
    for i, image in enumerate(images):
        if batches and len(batches[-1][1]) < MOSAIC_IMAGES_PER_CALL \
                and sum(cache.nbytes(im) for im in batches[-1][1]) + cache.nbytes(image) <= cache.budget:
            batches[-1][1].append(image)
        else:
            batches.append((i, [image]))
    loader.prefetch_device_views(batches[0][1], device, background=True)

    def resident(batch):
        pinned = {im.name for im in batch}
        return [im.device_view(device) for im in batch], [cache.get(im, pinned) for im in batch]

    with torch.cuda.device(device):
        if gsd is None:
            depths = [im.device_view(device).depth for im in images]
            gsd = mosaic_default_gsd(depths, [float(im.camera.K[0, 0]) for im in images])
            del depths
            print(f'--mosaic: ground sample distance {float(gsd):.6g} m (twice the median pixel footprint; --mosaic-gsd sets it).')
        try:
            m = engine.Mosaic(axes, gsd, device).run([(first, lambda batch=batch: resident(batch)) for first, batch in batches], options)
        except ValueError as e:
            # Three refusals of the run belong to a flag: begin's of the grid (--mosaic), normalize's of a cell's sample count
            # (--mosaic-blend) and the gain passes' of a cell's sample count or an image's size (--mosaic-gains).  The options were checked above, so begin and fill have nothing left to refuse in them; every other
            # ValueError (of a view, of a restored image) passes as it is.  A fourth: the direct solve's of a state that does not
            # fit the device (--mosaic-gain-solve).  A fifth: the consensus' of a state that does not fit, or of an image's sample
            # count in one cell (--mosaic-reject).
            raise _mosaic_refused(e, ('grid', 'blend', 'gains', 'gain_solve', 'reject'))
        out = m.result()
        pictures = [(png, _MOSAIC_PNG[how](out[key], stretch))
                    for key, (_, _, _, _, png, how) in engine.MOSAIC_OUTPUTS.items()
                    if png is not None and key in out]
        out = {k: v.cpu() if torch.is_tensor(v) else v for k, v in out.items()}
        surface_counts = None if surface is None else [int(x) for x in m.surface_counts.cpu()]
        support_counts = None if support is None else [int(x) for x in m.support_counts.cpu()]
    Hm, Wm = m.Hm, m.Wm
    source = out['source']
    filled = source >= 0
    n_filled, n_cells = int(filled.sum()), Hm * Wm
    per_image = torch.bincount(source[filled].to(torch.int64), minlength=len(images))
    for png, picture in pictures:
        _save_png(PILImage.fromarray(picture), output_dir / png)
    data = {**out, 'axes': m.axes.clone(), 'gsd': float(m.gsd), 'lo': torch.tensor([float(m.lo[0]), float(m.lo[1])], dtype=torch.float32),
            'images': [im.name for im in images], 'n_filled': n_filled, 'per_image': per_image}
    if blend is not None:
        data['blend'] = float(blend)
    if fill is not None:
        data['fill'], data['fill_levels'] = float(fill), int(m.fill_levels)
    if bands is not None:
        data['band_plan'] = [(float(h), f) for h, f in m.band_plan]
    torch.save(data, output_dir / 'mosaic.pt')
    top = int(per_image.argmax())
    print(f'mosaic of {len(images)} images: {Wm} x {Hm} cells of {float(m.gsd):.6g} m, {n_filled} filled '
          f'({100.0 * n_filled / n_cells:.1f} %), {n_cells - n_filled} empty; largest share {images[top].name} '
          f'({100.0 * int(per_image[top]) / max(1, n_filled):.1f} %)')
    if surface is not None:
        tops = out['surface'][filled]
        s0, s1 = (float(tops.min()), float(tops.max())) if n_filled else (0.0, 0.0)
        gone, part = surface_counts
        print(f'mosaic surface of {float(surface):.6g} m: top between {s0:.6g} and {s1:.6g} m along the view axis; {gone} of {part} samples '
              f'({100.0 * gone / max(1, part):.1f} %) lie more than {float(surface):.6g} m below their cell\'s top, in '
              f'{int((out["culled"] > 0).sum())} cells')
    if support is not None:
        _, above, part = support_counts
        print(f'mosaic support of {support} views: {int(((out["support"] < support) & filled).sum())} of {n_filled} filled cells rest on '
              f'fewer than {support}; {above} of {part} samples ({100.0 * above / max(1, part):.1f} %) stand more than '
              f'{float(surface):.6g} m above their cell\'s supported top, in {int((out["culled_above"] > 0).sum())} cells')
    if reject is not None:
        per = out['reject_per_image']
        tested, gone = int(per[:, 0].sum()), int(per[:, 1].sum())
        worst = int(per[:, 1].argmax()) if len(per) else 0
        print(f'mosaic reject of {float(reject):.6g}: {int(((out["reject_source"] >= 0) & filled).sum())} of {n_filled} filled cells have a '
              f'consensus of {engine._lib.MOSAIC_REJECT_MIN_VIEWS} or more images ({int(out["reject_overflow"].sum())} hold more than '
              f'{engine._lib.MOSAIC_REJECT_CELL_IMAGES}: the {engine._lib.MOSAIC_REJECT_CELL_IMAGES} earliest vote); {gone} of {tested} samples '
              f'({100.0 * gone / max(1, tested):.1f} %) differ from it by more than {float(reject):.6g}, in '
              f'{int((out["rejected"] > 0).sum())} cells; most rejected {images[worst].name} ({int(per[worst, 1]) if len(per) else 0} samples)')
    if gains is not None:
        g, rms, overlap = out['gains'].double(), out['gain_rms'], out['gain_overlap']
        far = (g.log().abs().max(dim=1).values * (overlap > 0)).argmax() if len(images) else 0
        lo, hi = np.float32(1.0 / gain_limit), np.float32(gain_limit)
        clipped = 0 if gain_limit == 1.0 else int((((out['gains'] == float(lo)) | (out['gains'] == float(hi))) & (overlap > 0)[:, None]).sum())
        print(f'mosaic gains of {gains} rounds (limit {gain_limit:.6g}): {int((overlap > 0).sum())} of {len(images)} images share a cell with '
              f'another; RMS disagreement in shared cells '
              + ' '.join(f'{ch} {float(rms[0, c]):.6g} -> {float(rms[-1, c]):.6g}' for c, ch in enumerate('RGB'))
              + f'; largest correction {images[int(far)].name} (gain R {float(g[far, 0]):.6g} G {float(g[far, 1]):.6g} B {float(g[far, 2]):.6g}); '
              f'{clipped} values clipped')
    if gain_solve is not None:
        diag, index = out['gain_diag'], out['gain_pair_index']
        print(f'mosaic gain solve direct: {int((index[:, 0] < index[:, 1]).sum())} overlapping pairs among {int((diag[:, 0] > 0).sum())} images '
              f'in {out["gain_components"]} connected groups; {out["gain_excluded_cells"]} of {out["gain_shared_cells"]} shared cells hold more than '
              f'{engine._lib.MOSAIC_GAIN_CELL_IMAGES} images and are left out')
        if out['gain_kept']:
            print(f'mosaic gain solve direct: channel {" ".join("RGB"[c] for c in out["gain_kept"])} kept its gains (its system has no finite '
                  f'positive solution)')
    if blend is not None:
        samples = out['samples'].to(torch.int64)
        total, most, several = int(samples.sum()), int(samples.max()), int((samples > 1).sum())
        print(f'mosaic blend of depth {float(blend):.6g} m: {total} samples, {total / max(1, n_filled):.2f} per filled cell on average, '
              f'{most} at most; {100.0 * several / max(1, n_filled):.1f} % of the filled cells blend more than one sample')
    if feather is not None:
        near, part = (int(x) for x in m.feather_counts.cpu())
        print(f'mosaic feather of {feather} px: {100.0 * near / max(1, part):.1f} % of the samples within {feather} px of an edge; '
              f'smallest weight sum in a filled cell {float(out["weight"][out["samples"] > 0].min()) if n_filled else 0.0:.6g}')
    if bands is not None:
        diff = (out['J_multiband'].double() - out['J_blend'].double())[filled]
        rms = diff.pow(2).mean(dim=0).sqrt().tolist() if n_filled else [0.0] * 3
        print(f'mosaic multi-band blend of {bands} bands: depths {" ".join(f"{float(h):.6g}" for h, _ in m.band_plan)} m, feathers '
              f'{" ".join("-" if f is None else str(f) for _, f in m.band_plan)} px; RMS difference from the blend '
              f'R {rms[0]:.6g} G {rms[1]:.6g} B {rms[2]:.6g}')
    if fill is not None:
        level = out['fill_level']
        print(f'mosaic fill of {float(fill):.6g} m ({int(m.fill_levels)} levels): {int((level > 0).sum())} cells filled, '
              f'{int((level < 0).sum())} left empty; deepest level {max(0, int(level.max()))}')
    return data


# ---- what the modes that do not fit refuse ------------------------------------------------------------------------------------
_GIVEN_WITH = {'--trim-outliers': ('--trim-rounds',), '--view-gains': ('--gain-rounds', '--gain-limit')}   # flags that count as it


def _given(args, flag: str) -> bool:
    """Whether ``flag`` stands on the command line, told from the namespace: a flag of the reference is there with its default,
    one of this engine's own only when it was given (``_Parser``); a flag that only goes with another counts as that one."""
    if flag == '--image-scale':
        return args.image_scale != 1
    value = getattr(args, flag[2:].replace('-', '_'), None)
    return (value is not None and value is not False) or any(_given(args, other) for other in _GIVEN_WITH.get(flag, ()))


_NOTHING_SHARED, _NO_TRIM, _NO_GAINS = 'nothing is fitted, so nothing is shared', 'there is no fit to trim', 'there is no fit to estimate gains from'
_NO_RESIDUALS, _NO_SNAPSHOT = 'there is no fit, hence no residuals', 'there are no iterations to snapshot'
_NO_UNCERTAINTY = 'there is no fit, hence no normal equations to take standard errors from'
_NO_PARAMETERS, _NO_PICTURE = 'no parameters are read: the restored images are', 'no picture of J is written'
_MODE_REFUSES = {   # mode -> (flag, why), in the order they are looked at
    '--mosaic': [('--shared-water', _NOTHING_SHARED),
                 ('--apply-water', 'restore first, into the directory to mosaic, then mosaic it'),
                 ('--check-consistency', 'check the directory in a run of its own'),
                 ('--trim-outliers', _NO_TRIM), ('--view-gains', _NO_GAINS), ('--save-quality', _NO_RESIDUALS),
                 ('--save-interval', _NO_SNAPSHOT), ('--params-path', _NO_PARAMETERS), ('--keep-matches', 'nothing is matched'),
                 ('--common-stretch', 'the mosaic is one picture: it is stretched by its own percentiles, or by --stretch-from'),
                 ('--image-scale', 'resized images have float32 colours, and the raw mosaic takes uint8'),
                 ('--save-uncertainty', _NO_UNCERTAINTY)],
    '--check-consistency': [('--shared-water', _NOTHING_SHARED),
                            ('--apply-water', 'restore first, into the directory to check, then check it'),
                            ('--trim-outliers', _NO_TRIM), ('--view-gains', _NO_GAINS), ('--save-quality', _NO_RESIDUALS),
                            ('--save-interval', _NO_SNAPSHOT), ('--params-path', _NO_PARAMETERS),
                            ('--keep-matches', 'no match list is kept: the pairs are compared where they are found'),
                            ('--common-stretch', _NO_PICTURE), ('--stretch-from', _NO_PICTURE),
                            ('--image-scale', 'resized images have float32 colours, and the raw comparison reads uint8'),
                            ('--mosaic', 'make the mosaic in a run of its own'), ('--save-uncertainty', _NO_UNCERTAINTY)],
    '--apply-water': [('--shared-water', _NOTHING_SHARED), ('--trim-outliers', _NO_TRIM), ('--view-gains', _NO_GAINS),
                      ('--save-quality', 'a single-view inversion has no residuals'), ('--save-interval', _NO_SNAPSHOT),
                      ('--params-path', 'the parameters come from the --apply-water file'), ('--keep-matches', 'nothing is matched'),
                      ('--mosaic', 'restore first, then make the mosaic of that directory'), ('--save-uncertainty', _NO_UNCERTAINTY)],
}


_ONLY_WITH = [   # (flag, the flag it needs, that one's value), in the order they are looked at
    ('--mosaic-gsd', '--mosaic', 'DIR'), ('--mosaic-blend', '--mosaic', 'DIR'), ('--mosaic-fill', '--mosaic', 'DIR'),
    ('--mosaic-feather', '--mosaic-blend', 'H'), ('--mosaic-bands', '--mosaic-blend', 'H'),
    ('--mosaic-gain-limit', '--mosaic-gains', 'R'), ('--mosaic-gains', '--mosaic', 'DIR'),
    ('--mosaic-support', '--mosaic-surface', 'T'), ('--mosaic-surface', '--mosaic', 'DIR'),
    ('--mosaic-gain-solve', '--mosaic-gains', 'R'), ('--mosaic-reject', '--mosaic', 'DIR'),
]


def _refuse_lone_flags(args) -> None:
    """The flags of ``_ONLY_WITH`` given without the flag they go with, refused before any file is opened."""
    for flag, needs, value in _ONLY_WITH:
        if getattr(args, flag[2:].replace('-', '_'), None) is not None and getattr(args, needs[2:].replace('-', '_'), None) is None:
            raise SystemExit(f'{flag}: only with {needs} {value}')


def _refuse_mode_flags(args, mode: str) -> None:
    """What ``mode`` (--mosaic, --check-consistency, --apply-water) does not combine with, refused before any file is opened."""
    for flag, why in _MODE_REFUSES[mode]:
        if _given(args, flag):
            raise SystemExit(f'{mode}: {flag} does not combine with it ({why}); drop one of the two flags')


def _refuse_mosaic_values(args, world: int = 1) -> None:
    """The values of --mosaic-gsd, --mosaic-blend, --mosaic-fill, --mosaic-feather, --mosaic-bands, --mosaic-surface,
    --mosaic-support, --mosaic-gains, --mosaic-gain-limit, --mosaic-gain-solve and --mosaic-reject and the world size a mosaic takes,
    refused before any file is opened."""
    gsd = getattr(args, 'mosaic_gsd', None)
    if gsd is not None and not (np.isfinite(gsd) and gsd > 0):
        raise SystemExit(f'--mosaic-gsd: G must be a finite size > 0 in metres, not {gsd}')
    from . import engine
    for field, (_, span, integral, unit, _, letter, words) in engine.MOSAIC_VALUES.items():
        value = getattr(args, 'mosaic_' + field, None)
        if value is None:
            continue
        if integral is None:   # a choice
            if value not in span:
                raise SystemExit(f'{_MOSAIC_FLAG[field]}: {letter} must be {" or ".join(span)}, not {value}')
            continue
        lo, hi = span
        if not (np.isfinite(value) and lo <= value <= hi and (not integral or value == int(value))):
            raise SystemExit(f'{_MOSAIC_FLAG[field]}: {letter} must be {words} within [{lo:g}, {hi:g}] {unit}, not '
                             + (f'{value:g}' if integral else f'{value}'))
    if world > 1:
        raise SystemExit(f'--mosaic: a world size of {world} is not supported yet: the four phases are separate entries of the library '
                         f'so that ranks can all-reduce bounds, keys and pixel words between them, but that all-reduce is not built; '
                         f'run one process')


def _refuse_stretch_flags(args) -> None:
    """What --common-stretch and --stretch-from do not combine with, refused before any file is opened."""
    if not getattr(args, 'common_stretch', False):
        return
    if getattr(args, 'stretch_from', None) is not None:
        raise SystemExit('--common-stretch: --stretch-from gives the stretch already; drop one of the two flags')
    if not getattr(args, 'shared_water', False) and getattr(args, 'apply_water', None) is None:
        raise SystemExit('--common-stretch: only with --shared-water or --apply-water -- images restored with their own water each '
                         'have no common scale; take the stretch.pt of such a run and give it to this one with --stretch-from')
    if args.save_interval is not None:
        raise SystemExit('--common-stretch: --save-interval snapshots are written before the pool is complete; drop one of the two '
                         'flags (--stretch-from combines with snapshots)')


def parse_args(args: argparse.Namespace):
    """Runs the CLI request (sucre.py:222-261); with WORLD_SIZE > 1 each rank restores its shard of the images."""
    rank, local_rank, world = sdist.env_rank_world()
    shared = bool(getattr(args, 'shared_water', False))
    apply = getattr(args, 'apply_water', None)
    check = getattr(args, 'check_consistency', None)
    mosaic_dir = getattr(args, 'mosaic', None)
    _refuse_lone_flags(args)
    if mosaic_dir is not None:
        _refuse_mode_flags(args, '--mosaic')
        _refuse_mosaic_values(args, world)
    if check is not None:
        _refuse_mode_flags(args, '--check-consistency')
    _refuse_stretch_flags(args)
    common = bool(getattr(args, 'common_stretch', False))
    stretch = None
    if getattr(args, 'stretch_from', None) is not None:   # read and checked before any image is opened
        stretch = read_stretch_file(args.stretch_from)
    if apply is not None:
        _refuse_mode_flags(args, '--apply-water')
        water = read_water_file(apply, args.light_model)
    _refuse_trim_flags(args)
    _refuse_gain_flags(args)
    if shared:
        _refuse_shared_flags(args)
    if getattr(args, 'save_uncertainty', False) and args.light_model:
        raise SystemExit(f'--save-uncertainty: --light-model does not combine with it ({_NO_LIGHT_UNCERTAINTY}); drop one of the two flags')
    # torch's CPU thread pool follows the machine's CPU count; inside a container with a CPU quota that many spinning
    # threads only get the process throttled (147 CPU-seconds for 64 images on a 256-CPU box with a 16-CPU quota)
    local_world = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', world)))
    cpus = max(1, loader.effective_cpus() // local_world)   # the ranks of one node share its CPUs (and its quota)
    torch.set_num_threads(max(1, min(torch.get_num_threads(), cpus)))
    device = args.device
    if world > 1 and str(device).startswith('cuda'):
        # one GPU per rank; ranks beyond the GPUs of the box wrap around (two ranks on a one-GPU test box: per-image mode
        # has no collective, so sharing a GPU only shares its time)
        index = local_rank % max(1, torch.cuda.device_count())
        device = f'cuda:{index}'
        torch.cuda.set_device(index)
    print('Loading COLMAP model.')
    colmap_model = sfm.COLMAPModel(model_dir=args.model_dir, image_dir=args.image_dir, depth_dir=args.depth_dir,
                                   image_scale=args.image_scale)
    if args.image_name is not None:
        images = [colmap_model[args.image_name]]
    elif args.image_list is not None:
        images = [colmap_model[name] for name in args.image_list.read_text().splitlines() if name.strip()]
    else:
        lo, hi = args.image_ids
        images = [colmap_model.images[i] for i in range(lo, hi) if i in colmap_model.images]
    if shared and len(images) < world:
        raise SystemExit(f'--shared-water: {len(images)} image(s) for {world} ranks; every rank needs at least one image')
    request = [im.name for im in images]
    images = sdist.shard_images(images, rank, world)

    skipped = set(args.filter_images_path.read_text().splitlines()) if args.filter_images_path else set()
    image_list = [im for im in colmap_model.images.values() if im.name not in skipped]
    if shared:
        _check_shared_memory(images, image_list, args.light_model, device)
    args.output_dir.mkdir(parents=True, exist_ok=True)
    in_flight = int(os.environ.get('SUCRE_IMAGES_IN_FLIGHT', '2'))   # engine knob, not a reference flag
    survey = not shared and len(images) > 1 and in_flight > 1 and args.save_interval is None and str(device).startswith('cuda')
    if apply is not None:
        survey = len(images) > 1 and str(device).startswith('cuda')   # (the worker processes: decoding and PNG encoding)
        print(f'--apply-water: single-view inversion at the parameters of {apply}; nothing is fitted or matched, so --num-iter, '
              f'--learning-rate, --batch-size, --use-closed-form, --min-cover, --filter-images-path and --force-compute-matches are ignored.')
    if check is not None:
        survey = False
        print(f'--check-consistency: the restored images of {check} are compared where they see the same seabed; nothing is fitted, '
              f'so --num-iter, --learning-rate, --batch-size, --use-closed-form, --light-model and --force-compute-matches are ignored.')
    if mosaic_dir is not None:
        survey = False
        print(f'--mosaic: the restored images of {mosaic_dir} are dropped onto one grid; nothing is fitted or matched, so --num-iter, '
              f'--learning-rate, --batch-size, --use-closed-form, --light-model, --min-cover, --filter-images-path and '
              f'--force-compute-matches are ignored.')
    if survey:
        # image files are decoded and the result pictures encoded by child processes (_pixelio.WorkerPool: CPU work in
        # the process that drives the GPU slows its launches down, and PIL's decoder does not scale over threads);
        # SUCRE_IO_PROCESSES=0 keeps both in this process's threads
        n_io = int(os.environ.get('SUCRE_IO_PROCESSES', max(1, cpus - 2)))
        if n_io > 0:
            _pixelio.start_pool(n_io)
    # The host's torch work is all tiny (3x3 inverses and products per view, nine-number parameter vectors): with its default of
    # one intra-op thread per core every such call wakes the whole OpenMP team -- 2 ms instead of 0.1 ms per camera on a 16-core
    # box with the decode and writer threads next to it (tools/cli_survey_bench.py: 20 -> 16.5 ms per 640x480 image, 49 -> 41 per
    # 1080p image).  SUCRE_HOST_TORCH_THREADS (1; 0 = leave torch alone); restored on the way out.
    host_threads = int(os.environ.get('SUCRE_HOST_TORCH_THREADS', '1'))
    threads_before = torch.get_num_threads()
    if host_threads > 0:
        torch.set_num_threads(host_threads)
    try:
        if mosaic_dir is not None:
            mosaic(images, colmap_model, mosaic_dir, args.output_dir, gsd=getattr(args, 'mosaic_gsd', None), stretch=stretch, device=device,
                   **{field: getattr(args, 'mosaic_' + field, None) for field in _MOSAIC_FLAG if field != 'grid'})
        elif check is not None:
            if world > 1:   # the targets' records are gathered on rank 0
                sdist.init_process_group()
            check_consistency(images, colmap_model, check, args.output_dir, image_list=image_list, min_cover=args.min_cover,
                              device=device, request=request, rank=rank, num_workers=args.num_workers)
        elif apply is not None:
            if common and world > 1:   # the pool spans the ranks: its histograms are all-reduced
                sdist.init_process_group()
            apply_water(images, colmap_model, args.output_dir, water, light_model=args.light_model, device=device, in_flight=in_flight,
                        stretch='common' if common else stretch, request=request, rank=rank)
        elif shared:
            restore_shared_water(images, colmap_model, args, image_list, device, request, rank, world,
                                 stretch='common' if common else stretch)
        else:
            _run_request(args, images, image_list, colmap_model, device, survey, in_flight, stretch=stretch)
    finally:
        _pixelio.stop_pool()
        if host_threads > 0:
            torch.set_num_threads(threads_before)


def _extras_of(args, stretch=None) -> _Extras:
    """The record of a command line; a flag of this engine's own is in the namespace only when it was given (``_Parser``)."""
    given = {f.name: getattr(args, f.name) for f in dataclasses.fields(_Extras) if hasattr(args, f.name)}
    return _Extras(**{**given, 'stretch': stretch})


def _run_request(args, images, image_list, colmap_model, device, survey: bool, in_flight: int, stretch=None) -> None:
    if str(device).startswith('cuda') and images:   # start decoding + uploading the scene now, in the background
        loader.prefetch_for_targets(images, image_list, device, num_workers=args.num_workers, min_cover=args.min_cover)
    extras = _extras_of(args, stretch)
    if survey:
        restore_images(images, colmap_model, args.output_dir, in_flight=in_flight, keep_matches=args.keep_matches,
                       device=device, light_model=args.light_model, use_closed_form=args.use_closed_form,
                       min_cover=args.min_cover, image_list=image_list, lr=args.learning_rate, num_iter=args.num_iter,
                       params_path=args.params_path, force_compute_matches=args.force_compute_matches,
                       num_workers=args.num_workers, **vars(extras))
        return
    for image in images:
        _restore_one(image, colmap_model, args.output_dir, args.light_model, args.use_closed_form, args.min_cover, image_list,
                     args.learning_rate, args.num_iter, args.batch_size, args.save_interval, args.params_path,
                     args.force_compute_matches, args.keep_matches, args.num_workers, device, extras)


def _refuse_trim_flags(args) -> None:
    """What --trim-outliers does not combine with (and what it takes), refused before anything is decoded or matched."""
    trim, rounds = getattr(args, 'trim_outliers', None), getattr(args, 'trim_rounds', None)
    if trim is None:
        if rounds is not None:
            raise SystemExit('--trim-rounds: only with --trim-outliers K')
        return
    if not (np.isfinite(trim) and trim > 0):
        raise SystemExit(f'--trim-outliers: K must be a finite multiple > 0, not {trim}')
    if rounds is not None and rounds < 1:
        raise SystemExit(f'--trim-rounds: N must be >= 1, not {rounds}')
    if getattr(args, 'shared_water', False):
        raise SystemExit('--trim-outliers: a shared fit (--shared-water) is not trimmed; drop one of the two flags')
    if args.save_interval is not None:
        raise SystemExit('--trim-outliers: --save-interval snapshots are not supported for a trimmed refit; drop one of the two flags')


def _refuse_gain_flags(args) -> None:
    """What --view-gains does not combine with (and what it takes), refused before anything is decoded or matched."""
    rounds, limit = getattr(args, 'gain_rounds', None), getattr(args, 'gain_limit', None)
    if not getattr(args, 'view_gains', False):
        if rounds is not None:
            raise SystemExit('--gain-rounds: only with --view-gains')
        if limit is not None:
            raise SystemExit('--gain-limit: only with --view-gains')
        return
    if rounds is not None and rounds < 1:
        raise SystemExit(f'--gain-rounds: N must be >= 1, not {rounds}')
    if limit is not None and not (np.isfinite(limit) and limit >= 1):
        raise SystemExit(f'--gain-limit: L must be finite and >= 1, not {limit}')
    if getattr(args, 'shared_water', False):
        raise SystemExit('--view-gains: a shared fit (--shared-water) is not compensated; drop one of the two flags')
    if args.save_interval is not None:
        raise SystemExit('--view-gains: --save-interval snapshots are not supported for a compensated refit; drop one of the two flags')
    if getattr(args, 'trim_outliers', None) is not None:
        raise SystemExit('--view-gains: --trim-outliers is not supported together with it yet; drop one of the two flags')


def _refuse_shared_flags(args) -> None:
    """What --shared-water does not combine with, refused before anything is decoded or matched."""
    if args.image_scale != 1:
        raise SystemExit(f'--shared-water: --image-scale {args.image_scale} gives float32 colours, which shared fits do not '
                         f'support; drop --image-scale or --shared-water')
    if args.save_interval is not None:
        raise SystemExit('--shared-water: --save-interval snapshots are not supported for a shared fit; drop one of the two flags')


def _check_shared_memory(images: list, image_list: list, light_model: bool, device) -> None:
    """All the images of a rank stay matched on the device at once: their workspaces (sucre_workspace_bytes, plus
    sucre_light_workspace_bytes with the light model, at the engine's capacity steps) must fit into what is free now."""
    from . import _lib, engine
    lib = _lib.load()
    cap = min(engine.view_capacity(min(len(image_list), engine.MAX_VIEWS)), engine.MAX_VIEWS)
    need = 0
    for im in images:
        H, W = int(im.camera.height), int(im.camera.width)
        need += int(lib.sucre_workspace_bytes(H, W, cap))
        if light_model:
            need += int(lib.sucre_light_workspace_bytes(H, W, cap))
    free = int(torch.cuda.mem_get_info(device)[0])
    if need > free:
        raise SystemExit(f'--shared-water: the {len(images)} image(s) of this rank need {need} bytes of workspaces on {device}, '
                         f'{free} are free; run more ranks (torchrun --nproc-per-node N) so that each holds fewer images')


def restore_shared_water(images: list, colmap_model: sfm.COLMAPModel, args, image_list: list, device, request: list,
                         rank: int = 0, world: int = 1, stretch=None) -> None:
    """--shared-water: every image of this rank is matched into its own workspace, then all are fitted jointly with one
    B, beta, gamma (and, with --light-model, one cam2light, sigma) for the whole request -- every image keeps its own J --
    through engine.HipWaterGroup under dist.fit_shared_water (one all-reduce of the sums per iteration across the ranks).
    Per image the outputs of a plain run; rank 0 also writes ``shared_water.pt`` (the shared parameters, ``trace``, ``images``).
    ``stretch``: ``(lo, hi)`` -- every ``_rgb.png`` by this fixed stretch (--stretch-from); ``'common'`` -- by the 1st and 99th
    percentile of the pool of the valid pixels of the J of all images of all ranks, pooled where they are once the group has
    finished (``common_stretch``); rank 0 then also writes ``stretch.pt`` (--common-stretch)."""
    from . import engine
    if world > 1:
        sdist.init_process_group()
    if str(device).startswith('cuda') and images:
        loader.prefetch_for_targets(images, image_list, device, num_workers=args.num_workers, min_cover=args.min_cover)
    extras = _extras_of(args, None if isinstance(stretch, str) else stretch)
    jobs = []
    for k, image in enumerate(images):
        with engine.slot_lane(k):   # every image in its own workspace
            jobs.append(_restore_submit(image, colmap_model, args.output_dir, args.light_model, args.use_closed_form,
                                        args.min_cover, image_list, args.learning_rate, args.num_iter, args.params_path,
                                        args.force_compute_matches, args.num_workers, device, extras=extras))
    for job in jobs:
        job.resto = _adam_begin(job.sucre, job.matches_data, params0=jobs[0].params0)
    restos = [job.resto for job in jobs]
    T = int(args.num_iter)
    trace = torch.zeros((T, 20 if args.light_model else 10), dtype=torch.float64, device=restos[0].device)
    print(f'Solve least squares with Adam optimizer ({T} iterations), shared water over {len(request)} images.')
    group = engine.HipWaterGroup(restos, lr=args.learning_rate, use_closed_form=args.use_closed_form, trace=trace,
                                 params0=jobs[0].params0)
    sdist.fit_shared_water(group, T)
    for job in jobs:   # --save-quality, --save-uncertainty: behind the group's finish, per image, before anything is read
        _enqueue_quality(job)
        _enqueue_uncertainty(job)
    pooled = None
    if extras.save_uncertainty:   # H, SSR, N and P add over the images of all ranks; every image's J_se uses the pooled covariance
        sums_list = [job.uncertainty[2] for job in jobs]
        pooled_sums = pooled_uncertainty(sums_list)
        pooled = {**engine.water_uncertainty(pooled_sums), 'sums': pooled_sums.numpy()}
        for job in jobs:
            job.pooled_uncertainty = pooled
    trace = trace.cpu().numpy()
    _log_trace(trace, 0)
    for job, resto in zip(jobs, restos):
        _pull_results(job.sucre, resto)
    shared = {k: v.detach().cpu().clone() for k, v in jobs[0].sucre.state_dict().items() if k != 'J'}
    if isinstance(stretch, str):   # 'common': the J of this rank are resident; every rank obtains the same six numbers
        lo, hi, n_valid = common_stretch([job.sucre.J.detach().contiguous() for job in jobs])
        _write_common_stretch(args.output_dir, lo, hi, n_valid, request, rank)
        for job in jobs:
            job.sucre.stretch = (lo, hi)
    for job in jobs:
        _restore_finish(job, args.keep_matches)
    if rank == 0:
        torch.save({**shared, 'trace': torch.from_numpy(trace), 'images': list(request)}, Path(args.output_dir) / 'shared_water.pt')
    if pooled is not None:   # (every rank takes part in the gather)
        per_image = [x for part in sdist.all_gather_objects([(job.image.name, job.uncertainty['sums']) for job in jobs]) for x in part]
        if rank == 0:
            by_name = dict(per_image)
            torch.save({**_uncertainty_record(pooled), 'images': list(request), 'image_sums': torch.stack([by_name[name] for name in request])},
                       Path(args.output_dir) / 'shared_water_uncertainty.pt')
            print('shared water: ' + _uncertainty_line(pooled))


class _Parser(argparse.ArgumentParser):
    """The reference's parser plus ``extras``: flags of this engine's own that stay out of the reference-pinned table of
    actions and defaults (tests/test_shared_water_cli.py lists it action by action).  They are parsed first, from the same
    command line, and whatever they set is added to the namespace; absent, they leave no trace in it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.extras = argparse.ArgumentParser(add_help=False, allow_abbrev=False, formatter_class=self.formatter_class,
                                              usage=argparse.SUPPRESS)

    def parse_known_args(self, args=None, namespace=None):
        own, rest = self.extras.parse_known_args(args)
        namespace, rest = super().parse_known_args(rest, namespace)
        for k, v in vars(own).items():
            setattr(namespace, k, v)
        return namespace, rest

    def format_help(self):
        own = self.extras.format_help()
        return super().format_help() + '\nfurther outputs:\n' + own[own.index('  --'):]


def build_parser() -> argparse.ArgumentParser:
    """Same flags, defaults and exclusivity group as the reference CLI (sucre.py:264-305)."""
    p = _Parser(description='SUCRe (MI355X engine).', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--image-dir', required=True, type=Path, help='directory holding the colour images')
    p.add_argument('--depth-dir', required=True, type=Path, help='directory holding the depth_<stem>.png maps')
    p.add_argument('--model-dir', required=True, type=Path, help='undistorted COLMAP model (cameras/images .bin or .txt)')
    p.add_argument('--output-dir', required=True, type=Path, help='where restored images and parameters go')
    which = p.add_mutually_exclusive_group(required=True)
    which.add_argument('--image-name', type=str, help='restore this single image')
    which.add_argument('--image-list', type=Path, help='text file, one image name per line')
    which.add_argument('--image-ids', type=int, nargs=2, metavar=('MIN_ID', 'MAX_ID'),
                       help='restore COLMAP image ids in [MIN_ID, MAX_ID)')
    p.add_argument('--light-model', action='store_true', help='model artificial lighting (light pose + beam shape)')
    p.add_argument('--use-closed-form', action='store_true',
                   help='solve J in closed form from the water parameters instead of optimising it')
    p.add_argument('--min-cover', type=float, default=0.000001,
                   help='drop a neighbour whose matches cover at most this fraction of the image')
    p.add_argument('--image-scale', type=float, default=1.0, help='rescale factor applied to all images (colour: OpenCV INTER_AREA when shrinking, INTER_CUBIC when '
                        'enlarging -- cv2 is used when installed, otherwise both are restated from its published algorithms, '
                        'unchecked against cv2 itself; depth: nearest neighbour)')
    p.add_argument('--filter-images-path', type=Path, help='text file of image names never used as neighbours')
    p.add_argument('--learning-rate', type=float, default=0.05, help='Adam learning rate')
    p.add_argument('--num-iter', type=int, default=200, help='Adam iterations')
    p.add_argument('--batch-size', type=int, default=5,
                   help='accepted for compatibility; the engine always runs the full batch in one pass')
    p.add_argument('--save-interval', type=int, help='also save the restored image every this many iterations')
    p.add_argument('--params-path', type=Path, help='.pt file to warm-start the model parameters from')
    p.add_argument('--force-compute-matches', action='store_true', help='discard a kept matches file first')
    p.add_argument('--keep-matches', action='store_true', help='export the match lists next to the outputs')
    p.add_argument('--num-workers', type=int, default=0, help='threads decoding images (0 = main thread)')
    p.add_argument('--device', type=str, default='cuda', help='GPU to run on')
    # (off unless given, and then absent from the namespace: the reference's flags and defaults stay exactly what they are)
    p.add_argument('--shared-water', action='store_true', default=argparse.SUPPRESS,
                   help='fit all images of the request jointly: one B, beta, gamma (and, with --light-model, one cam2light, '
                        'sigma) for all of them, a J per image; also writes shared_water.pt')
    p.extras.add_argument('--save-quality', action='store_true', default=argparse.SUPPRESS,
                          help='also write, per image, <stem>_quality.pt (observations and squared residuals of the fit per pixel and '
                        'per neighbour view), <stem>_coverage.png and <stem>_residual.png, and print the RMS residual and the '
                        'worst-fitting view')
    p.extras.add_argument('--save-uncertainty', action='store_true', default=argparse.SUPPRESS,
                          help='also write, per image, <stem>_uncertainty.pt (standard errors, covariance and correlation of B, beta, '
                               'gamma per channel from the Gauss-Newton normal equations of the fit, summed in float64 on the device, '
                               'and the standard error of J per pixel) and <stem>_uncertainty.png, and print the standard errors; '
                               'with --shared-water the sums are pooled over all images (shared_water_uncertainty.pt); tells a '
                               'survey whose water is determined from one whose residuals are merely small')
    p.extras.add_argument('--trim-outliers', type=float, metavar='K', default=argparse.SUPPRESS,
                          help='after the fit, drop every observation whose residual exceeds K times the RMS residual of its '
                               'channel (never a pixel\'s last ones) and fit again from the same start; also writes, per image, '
                               '<stem>_trim.pt and <stem>_trimmed.png and prints what each round dropped')
    p.extras.add_argument('--apply-water', type=Path, metavar='PATH', default=argparse.SUPPRESS,
                          help='do not fit: restore every image of the request from its own depth map with the B, beta, gamma (and, '
                               'with --light-model, cam2light, sigma) of this .pt file -- a shared_water.pt or a <name>.pt of an '
                               'earlier run; writes <stem>_rgb.png and <name>.pt (and <stem>_vignetting.png) per image')
    p.extras.add_argument('--check-consistency', type=Path, metavar='DIR', default=argparse.SUPPRESS,
                          help='do not fit: compare the restored J of every image of the request (DIR/<name>.pt, as this tool and the '
                               'reference write them) with the restored J of the other images on the pixels their depth maps match, '
                               'and the raw pictures likewise; writes <stem>_consistency.pt and <stem>_consistency.png per image and '
                               'consistency.pt, and prints the RMS colour difference of both')
    p.extras.add_argument('--mosaic', type=Path, metavar='DIR', default=argparse.SUPPRESS,
                          help='do not fit: drop every pixel of the images of the request that has a valid depth and a restored colour '
                               '(DIR/<name>.pt, as this tool and the reference write them) onto one plane grid that looks the way the '
                               'cameras look; the pixel seen through the least water wins its cell, nothing is blended and no hole is '
                               'filled (--mosaic-blend, --mosaic-fill); writes mosaic.png, mosaic_raw.png, mosaic_source.png and mosaic.pt and prints the size and the cover')
    p.extras.add_argument('--mosaic-gsd', type=float, metavar='G', default=argparse.SUPPRESS,
                          help='with --mosaic: metres per cell (twice the median pixel footprint of the images unless given)')
    p.extras.add_argument('--mosaic-blend', type=float, metavar='H', default=argparse.SUPPRESS,
                          help='with --mosaic: also a blended mosaic -- every cell the mean of ALL its pixels, each weighted by '
                               'max(1 - d / H, 0)^2 of the metres d of water it looked through beyond the cell\'s nearest view, summed in '
                               'fixed point (the same bits in any order); writes mosaic_blend.png and mosaic_blend_raw.png next to the '
                               'best-view files, which stay as they are, adds J_blend, raw_blend, weight, samples and blend to mosaic.pt '
                               'and prints one more line')
    p.extras.add_argument('--mosaic-fill', type=float, metavar='R', default=argparse.SUPPRESS,
                          help='with --mosaic: also close the holes -- cells no pixel landed in -- up to R metres across, by a bounded '
                               'push-pull over a pyramid of the grid (the same bits on every run); the mosaic is not extrapolated far beyond '
                               'its footprint; writes mosaic_filled.png, mosaic_raw_filled.png and mosaic_filled_mask.png (255 measured, 128 '
                               'filled, 0 empty; with --mosaic-blend also mosaic_blend_filled.png and mosaic_blend_raw_filled.png) next to the '
                               'other files, which stay as they are, adds J_filled, raw_filled, fill_level, fill and fill_levels to mosaic.pt '
                               'and prints one more line')
    p.extras.add_argument('--mosaic-feather', type=float, metavar='F', default=argparse.SUPPRESS,
                          help='with --mosaic-blend: also weight every pixel by its distance to the edge of its image\'s footprint -- the '
                               'image border, a NaN patch of the restored image, a hole of the depth map --, rising from nothing at the edge '
                               'to the full weight F source pixels inside (an integer, 1..1024; an exact distance map made on the device), '
                               'so the blend does not step where a view ends; the blended files and keys are then the feathered ones, the '
                               'best-view ones stay as they are; adds feather to mosaic.pt and prints one more line')
    p.extras.add_argument('--mosaic-bands', type=float, metavar='K', default=argparse.SUPPRESS,
                          help='with --mosaic-blend: also a multi-band blend -- every image is split into K detail bands (an integer, '
                               '1..6) and a residual, the residual is blended with the depth H (and the feather F), every finer band with '
                               'half the depth and half the feather of the one before, and the blended bands are added: the colour of the '
                               'blend with the detail of the best view; writes mosaic_multiband.png (with --mosaic-fill also '
                               'mosaic_multiband_filled.png) next to the other files, which stay as they are, adds J_multiband, bands and '
                               'band_plan to mosaic.pt and prints one more line')
    p.extras.add_argument('--mosaic-surface', type=float, metavar='T', default=argparse.SUPPRESS,
                          help='with --mosaic: also a surface test -- per cell the highest sample along the mosaic\'s view axis is found '
                               'first, and a sample that lies more than T metres below its cell\'s top takes part in nothing, so the lower '
                               'of two surfaces neither wins a cell nor is blended into it; the grid and the filled cells stay those of a '
                               'run without the flag; writes mosaic_surface.png (the height, highest ground white) and mosaic_culled.png '
                               'next to the other files, adds surface, culled and surface_tol to mosaic.pt and prints one more line')
    p.extras.add_argument('--mosaic-support', type=float, metavar='M', default=argparse.SUPPRESS,
                          help='with --mosaic-surface: the top of a cell is the highest level that at least M different images reach '
                               '(an integer, 1..4; a cell seen by fewer rests on the lowest of its per-image tops) instead of the plain '
                               'minimum, and a sample more than T metres ABOVE it takes part in nothing either, so a fish or one bad depth '
                               'patch in a single view no longer owns its cells; M = 1 is --mosaic-surface alone; writes '
                               'mosaic_culled_above.png, adds support, surface_source, culled_above, surface_top and surface_support '
                               'to mosaic.pt and prints one more line')
    p.extras.add_argument('--mosaic-gains', type=float, metavar='R', default=argparse.SUPPRESS,
                          help='with --mosaic: also a per-image gain compensation -- R rounds (an integer, 1..64) find one gain per '
                               'image and channel from the cells that two or more images share, so that images restored with a water '
                               'model each agree on the colour of the same seabed before anything is resolved or blended (fixed-point '
                               'sums: the same bits in any order); every file that is not a picture of J stays as it is; removes seams '
                               'between overlapping images, not a slow drift along a long chain; adds gains, gain_sums, gain_rms, '
                               'gain_overlap, gain_rounds and gain_limit to mosaic.pt and prints one more line')
    p.extras.add_argument('--mosaic-gain-limit', type=float, metavar='L', default=argparse.SUPPRESS,
                          help='with --mosaic-gains: every gain is kept within [1/L, L] (1..16; 2 unless given; 1 leaves every file as '
                               'it is without the flag)')
    p.extras.add_argument('--mosaic-gain-solve', type=str, metavar='S', default=argparse.SUPPRESS,
                          help='with --mosaic-gains: rounds (as without the flag) or direct -- the first round\'s gains come from one '
                               'exact least-squares solve over all pairs of overlapping images instead: removes a slow drift along '
                               'a chain of images, which the rounds do not; the remaining R - 1 rounds run after it; adds gain_solve, '
                               'gain_direct, gain_pair_index, gain_pair_words, gain_diag, gain_excluded_cells, gain_shared_cells, '
                               'gain_kept, gain_components and gain_prior to mosaic.pt and prints one more line')
    p.extras.add_argument('--mosaic-reject', type=float, metavar='T', default=argparse.SUPPRESS,
                          help='with --mosaic: also a colour consensus across views ahead of the splat -- per cell the images that reach '
                               'it (the 8 earliest when there are more) are ordered by their mean brightness there, the median one is '
                               'the reference, and a sample of another image that differs from the reference\'s mean colour by more '
                               'than T (units of J) in any channel takes part in nothing: a fish, a fin or a caustic that the rendered '
                               'depth maps do not hold no longer wins cells, enters the blend or biases --mosaic-gains; a cell seen by '
                               'fewer than 3 images rejects nothing; the grid and the filled cells stay those of a run without the '
                               'flag; T must exceed the offsets --mosaic-gains is to remove; writes mosaic_rejected.png, adds rejected, '
                               'reject_ref, reject_source, reject_views, reject_overflow, reject_per_image and reject_tol to mosaic.pt '
                               'and prints one more line')
    p.extras.add_argument('--common-stretch', action='store_true', default=argparse.SUPPRESS,
                          help='with --shared-water or --apply-water: stretch every <stem>_rgb.png between the SAME per-channel 1st '
                               'and 99th percentile, those of the valid pixels of all images of the request pooled (all ranks), '
                               'instead of each image\'s own; also writes stretch.pt (lo, hi, q, n_valid, images)')
    p.extras.add_argument('--stretch-from', type=Path, metavar='PATH', default=argparse.SUPPRESS,
                          help='stretch every <stem>_rgb*.png between the per-channel lo and hi (3 floats each) of this .pt file -- '
                               'the stretch.pt of a --common-stretch run -- instead of each image\'s own percentiles; in every mode')
    p.extras.add_argument('--trim-rounds', type=int, metavar='N', default=argparse.SUPPRESS,
                          help='rounds of --trim-outliers (1 unless given)')
    p.extras.add_argument('--view-gains', action='store_true', default=argparse.SUPPRESS,
                          help='after the fit, estimate one brightness gain per neighbour view and channel (exposure, strobe or '
                               'white-balance differences between views), divide it out of that view\'s observations and fit again '
                               'from the same start; also writes, per image, <stem>_gains.pt and prints the largest correction of '
                               'each round')
    p.extras.add_argument('--gain-rounds', type=int, metavar='N', default=argparse.SUPPRESS,
                          help='rounds of --view-gains (1 unless given)')
    p.extras.add_argument('--gain-limit', type=float, metavar='L', default=argparse.SUPPRESS,
                          help='gains of --view-gains are kept within [1/L, L] (2 unless given)')
    return p


def main(argv=None):
    parse_args(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
