"""Host driver of the HIP engine: device buffers, launch order, read-back.

PyTorch-ROCm is plumbing here (device memory, streams); every kernel lives in libsucre_hip.so.  One
``Restoration`` owns the workspace of one target image of size HxW fitted against up to ``n_views`` views (its
capacity; a target matched against fewer views lays the same buffer out for that number) and is reused across
images of the same geometry.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import threading
from dataclasses import dataclass, replace

import numpy as np
import torch

from . import _lib


@dataclass
class DeviceView:
    """What the engine needs from one sfm.Image: pixels on the GPU + float32 camera/pose matrices computed on
    the host the way the reference computes them (sfm.py:42-47, 92)."""
    depth: torch.Tensor   # (H,W) float32, cuda
    rgb: torch.Tensor     # (H,W,3) uint8, cuda (float32 for resized inputs, see Restoration(float_colour=True))
    K: torch.Tensor       # (3,3) float32, cpu
    R: torch.Tensor       # (3,3) float32, cpu   world-from-camera
    t: torch.Tensor       # (3,1) float32, cpu
    name: str = ''
    # Optional: the derived float32 matrices K^-1 and -R^T t, given by the caller instead of derived here.  torch derives
    # them on the HOST (sfm.py:42-47, 92), and MKL's float32 3x3 products differ in the last bit between CPU models, which
    # moves a handful of boundary pixels per million matches: a caller comparing against results made on another machine
    # (tests/test_gpu_baseline.py: the reference's own goldens) passes that machine's matrices.
    Kinv: torch.Tensor | None = None
    tinv: torch.Tensor | None = None

    def to_struct(self, packed: bool = False) -> _lib.SucreView:
        """sucre_view_t of this view (cached: the matrices are derived once per view, not once per target image).
        ``packed``: the neighbour-view form whose ``depth`` points to the view's ``sucre_pack_view`` records and whose
        ``rgb`` is NULL (see ``packed_records``)."""
        slot = '_struct_packed' if packed else '_struct'
        key = (self.depth.data_ptr(), self.rgb.data_ptr())
        if packed and self.__dict__.get('_packed') is not None:
            key = key + (self.__dict__['_packed'][1].data_ptr(),)   # the struct points into THESE records
        cached = self.__dict__.get(slot)
        if cached is not None and cached[0] == key:
            return cached[1]
        if packed:
            H, W = self.depth.shape
            records = self.packed_records()
            key = key + (records.data_ptr(),)
            s = camera_struct(self.K, self.R, self.t, H, W, records.data_ptr(), 0, Kinv=self.Kinv, tinv=self.tinv)
        else:
            s = self._build_struct()
        self.__dict__[slot] = (key, s)
        return s

    def packed_records(self) -> torch.Tensor:
        """Depth map and uint8 colours interleaved into 8-byte records {float32 depth, r, g, b, 0} (``sucre_pack_view``),
        built once per view on a side stream: as a neighbour the view is then matched with one gather per landing pixel
        instead of two (csrc/match.hip is bound by its gathers).  Consumers on any stream call ``wait_packed`` first."""
        key = (self.depth.data_ptr(), self.rgb.data_ptr())
        cached = self.__dict__.get('_packed')
        if cached is not None and cached[0] == key:
            return cached[1]
        assert self.rgb.dtype == torch.uint8, 'packed records hold uint8 colours'
        with _PACK_LOCK:   # the CLI decodes and submits on several threads: a view's records are built once and never replaced
            cached = self.__dict__.get('_packed')   # (a struct handed to a launch points into them)
            if cached is not None and cached[0] == key:
                return cached[1]
            H, W = self.depth.shape
            dev = self.depth.device
            out = torch.empty(H * W * 8, dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                side = _pack_stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))   # the pixels may have been produced on the caller's stream
                with torch.cuda.stream(side):
                    _lib.check(_lib.load().sucre_pack_view(C.c_void_p(self.depth.data_ptr()), C.c_void_p(self.rgb.data_ptr()), H, W,
                                                           C.c_void_p(out.data_ptr()), _stream_ptr()))
                    done = torch.cuda.Event()
                    done.record()
            self.__dict__['_packed'] = [key, out, done, True]   # one entry: records, their event and "not known complete yet"
            return out

    def repack(self) -> None:
        """Builds the records again, in place, on the CURRENT stream (same bytes; allocation-free): what a caller pays who
        meets this view for the first time -- bench.py charges it to every timed image (VERDICT round 5, weak point 5)."""
        records = self.packed_records()
        self.wait_packed()
        H, W = self.depth.shape
        with torch.cuda.device(self.depth.device):
            _lib.check(_lib.load().sucre_pack_view(C.c_void_p(self.depth.data_ptr()), C.c_void_p(self.rgb.data_ptr()), H, W,
                                                   C.c_void_p(records.data_ptr()), _stream_ptr()))

    def twin(self) -> 'DeviceView':
        """The same pixels and matrices as a view of its own: own packed records, own struct caches (bench.py gives every
        in-flight slot its own, so that one slot's ``repack`` never rewrites records another slot's match kernel is reading)."""
        return DeviceView(depth=self.depth, rgb=self.rgb, K=self.K, R=self.R, t=self.t, name=self.name, Kinv=self.Kinv, tinv=self.tinv)

    def wait_packed(self) -> None:
        """Makes the current stream wait for this view's records (nothing once they are known to be complete)."""
        entry = self.__dict__.get('_packed')
        if entry is not None and entry[3]:
            if entry[2].query():
                entry[3] = False
            else:
                torch.cuda.current_stream(self.depth.device).wait_event(entry[2])

    def as_float_colour(self) -> 'DeviceView':
        """This view with float32 colours (float32(float64(k)/255), loader.py:157-163): used when other views of the
        same restoration are resized images, whose colours are float32 already."""
        if self.rgb.dtype == torch.float32:
            return self
        twin = self.__dict__.get('_float_twin')
        if twin is None:
            twin = DeviceView(depth=self.depth, rgb=(self.rgb.to(torch.float64) / 255).to(torch.float32).contiguous(),
                              K=self.K, R=self.R, t=self.t, name=self.name)
            self.__dict__['_float_twin'] = twin
        return twin

    def _build_struct(self) -> _lib.SucreView:
        H, W = self.depth.shape
        assert self.depth.dtype == torch.float32 and self.depth.is_contiguous() and self.depth.is_cuda
        assert self.rgb.dtype in (torch.uint8, torch.float32) and self.rgb.is_contiguous() and self.rgb.shape == (H, W, 3)
        return camera_struct(self.K, self.R, self.t, H, W, self.depth.data_ptr(), self.rgb.data_ptr(), Kinv=self.Kinv, tinv=self.tinv)


def repack_views(views: list) -> None:
    """``DeviceView.repack`` for views of one size, sixteen views per launch (``sucre_pack_views``): records rebuilt in place on the
    CURRENT stream."""
    views = [v for v in views if v.rgb.dtype == torch.uint8]
    if not views:
        return
    H, W = views[0].depth.shape
    if any(tuple(v.depth.shape) != (H, W) for v in views):   # mixed sizes: one by one
        for v in views:
            v.repack()
        return
    recs = [v.packed_records() for v in views]
    for v in views:
        v.wait_packed()
    n = len(views)
    dp = (C.c_void_p * n)(*[v.depth.data_ptr() for v in views])
    cp = (C.c_void_p * n)(*[v.rgb.data_ptr() for v in views])
    op = (C.c_void_p * n)(*[r.data_ptr() for r in recs])
    with torch.cuda.device(views[0].depth.device):
        _lib.check(_lib.load().sucre_pack_views(dp, cp, op, n, H, W, _stream_ptr()))


def camera_struct(K: torch.Tensor, R: torch.Tensor, t: torch.Tensor, H: int, W: int, depth_ptr: int = 0,
                  rgb_ptr: int = 0, Kinv: torch.Tensor | None = None, tinv: torch.Tensor | None = None) -> _lib.SucreView:
    """sucre_view_t from a camera matrix and a world-from-camera pose, the derived matrices computed on the host the way
    the reference computes them (K.inverse(): sfm.py:92; Pose.inverse() = (R.T, -R.T @ t): sfm.py:42-47)."""
    K = K.to(torch.float32).cpu()
    R = R.to(torch.float32).cpu()
    t = t.to(torch.float32).cpu().view(3, 1)
    Kinv = K.inverse() if Kinv is None else Kinv.to(torch.float32).cpu().view(3, 3)      # sfm.py:92
    Rinv = R.T              # sfm.py:47
    tinv = -R.T @ t if tinv is None else tinv.to(torch.float32).cpu().view(3, 1)         # sfm.py:47
    s = _lib.SucreView()
    s.depth, s.rgb, s.H, s.W = depth_ptr or None, rgb_ptr or None, int(H), int(W)
    for name, val in (('K', K), ('Kinv', Kinv), ('R', R), ('t', t), ('Rinv', Rinv), ('tinv', tinv)):
        flat = val.contiguous().view(-1).tolist()
        setattr(s, name, (C.c_float * len(flat))(*flat))
    return s


def project_points(view: _lib.SucreView, wP: torch.Tensor) -> torch.Tensor:
    """int32[n]: the pixel ``v * W + u`` of ``view`` that each world point of ``wP`` ((3, n) float32, cuda) truncates
    into, -1 = outside the sensor -- ``Image.project_to_view`` + the cast and bound test of ``match_one_way``
    (sfm.py:103-107, 115-117) in the match kernel's float32 operation order (csrc/match.hip, project_points_kernel)."""
    assert wP.is_cuda and wP.dtype == torch.float32 and wP.dim() == 2 and wP.shape[0] == 3
    wP = wP.contiguous()
    n = wP.shape[1]
    out = torch.empty(n, dtype=torch.int32, device=wP.device)
    with torch.cuda.device(wP.device):
        _lib.check(_lib.load().sucre_project_points(C.byref(view), C.c_void_p(wP.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                                    _stream_ptr()))
    return out


_PACK_STREAMS: dict = {}
_PACK_LOCK = threading.Lock()


def _pack_stream(dev) -> 'torch.cuda.Stream':
    key = str(dev)
    if key not in _PACK_STREAMS:
        _PACK_STREAMS[key] = torch.cuda.Stream(dev)
    return _PACK_STREAMS[key]


# engine knob: neighbour views as 8-byte {depth, colour} records (one gather per landing pixel; +8 bytes per pixel and view)
PACKED_VIEWS = os.environ.get('SUCRE_PACKED_VIEWS', '1') != '0'

# engine knob: sucre_fit_run takes its J-parameter iterations in pairs of launches that touch a pixel's Adam moments once per pair
# (csrc/fit.hip, 'Paired iterations'; every result bit is the same either way); 0 = one launch per iteration
PAIRED_FIT = os.environ.get('SUCRE_PAIRED_FIT', '1') != '0'

MAX_VIEWS = 4096   # kMaxViews of csrc/layout.h: views of one restoration (after the overlap cull of sfm.Image.match_images)


def _stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Restoration:
    """Workspace + launch sequence for one target image (replaces the HDF5 spill and the host-resident
    MatchesData of the reference, loader.py:56-130)."""

    def __init__(self, height: int, width: int, n_views: int, device: str | torch.device = 'cuda', light: bool = False,
                 obs_format: str = 'f32', float_colour: bool = False):
        """``obs_format``: 'f32' = 7 B/observation, lossless (default); 'u16mm' = 5 B/observation, ranges rounded to
        the millimetre (BASELINE config 5; include/sucre_hip.h SUCRE_OBS_U16MM).  ``float_colour``: the views' colour
        images are float32 (resized inputs, --image-scale: loader.py:156-163 resizes in float64, so colours are no
        longer k/255); the observations then carry float32 colours in the extension workspace (SUCRE_EXT_COLOUR)."""
        self.lib = _lib.load()
        self.light = bool(light)
        self.float_colour = bool(float_colour)
        self.both = self.light and self.float_colour   # light model on float32 colours: two sets of extension planes
        if self.float_colour and obs_format != 'f32':
            raise NotImplementedError('float32 colours need the f32 store')
        if obs_format not in _lib.OBS_FORMATS:
            raise ValueError(f'obs_format must be one of {sorted(_lib.OBS_FORMATS)}, not {obs_format!r}')
        if self.light and obs_format != 'f32':
            raise NotImplementedError('the artificial-light model keeps float32 camera points: obs_format must be f32')
        self.obs_format = obs_format
        self._streams_used: dict = {}
        self._fmt = _lib.OBS_FORMATS[obs_format]
        self._fmt_flag = _lib.FIT_OBS_U16MM if self._fmt == _lib.OBS_U16MM else 0
        self.H, self.W, self.n_views = int(height), int(width), int(n_views)
        self.capacity = int(n_views)   # the buffers are sized for this many views; match() may use fewer
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.SucreError('the HIP engine needs a GPU device (there is no CPU fallback)')
        nbytes = self.lib.sucre_workspace_bytes(self.H, self.W, self.n_views)
        if nbytes == 0:
            raise _lib.SucreError(self.lib.sucre_last_error().decode())
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        assert self.ws.data_ptr() % 256 == 0
        self.lws = None
        if self.light or self.float_colour:  # extension workspace: camera points / float colours + 19 parameters
            lbytes = (self.lib.sucre_light_workspace_bytes_ext(self.H, self.W, self.n_views, _lib.EXT_POINTS_COLOUR) if self.both
                      else self.lib.sucre_light_workspace_bytes(self.H, self.W, self.n_views))
            self.lws = torch.empty(lbytes, dtype=torch.uint8, device=self.device)
            assert self.lws.data_ptr() % 256 == 0
        self._views_dev = None
        # the view table goes through a pinned staging buffer: a copy from pageable memory makes the host wait
        self._views_host = torch.empty(self.capacity * C.sizeof(_lib.SucreView), dtype=torch.uint8).pin_memory()
        self._views_buf = torch.empty(self.capacity * C.sizeof(_lib.SucreView), dtype=torch.uint8, device=self.device)
        self._views_copied = None
        self._keepalive = []
        self._batch_table = None
        self.trace = None
        self.steps_done = 0
        self.min_cover = None   # of the last match / import_matches: trim_outliers finalises again with it

    # -- plumbing -----------------------------------------------------------------------------------------
    def _sp(self) -> C.c_void_p:
        """The current HIP stream, remembered as one this workspace has work queued on (``return_restoration`` leaves an event
        on exactly these for the workspace's next owner)."""
        st = torch.cuda.current_stream(self.device)
        self._streams_used[st.cuda_stream] = st
        return C.c_void_p(st.cuda_stream)

    @property
    def _ext_mode(self) -> int:
        return _lib.EXT_POINTS_COLOUR if self.both else _lib.EXT_COLOUR if self.float_colour else _lib.EXT_POINTS

    @property
    def _ext_flag(self) -> int:
        return _lib.FIT_EXT_BOTH if self.both else _lib.FIT_EXT_COLOUR if self.float_colour else 0

    @property
    def _geom(self):
        return C.c_void_p(self.ws.data_ptr()), self.H, self.W, self.n_views

    def _note_stream(self) -> None:
        """A view of the workspace is being handed out on the current stream (a ``.cpu()`` or a copy the caller queues there reads the
        workspace): ``return_restoration`` must leave an event on that stream too, not only on those the C ABI was launched on
        (ADVICE round 5)."""
        if self.device.type == 'cuda':
            st = torch.cuda.current_stream(self.device)
            self._streams_used[st.cuda_stream] = st

    def _region(self, region: int, dtype: torch.dtype, count: int) -> torch.Tensor:
        self._note_stream()
        off = self.lib.sucre_ws_offset(self.H, self.W, self.n_views, region)
        if off < 0:
            raise _lib.SucreError(self.lib.sucre_last_error().decode())
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        return self.ws[off:off + nbytes].view(dtype)

    # -- matching (sfm.py:127-138 + loader.py:78-118) ---------------------------------------------------------
    def match(self, target: DeviceView, views: list[DeviceView], min_cover: float = 1e-6, packed: bool | None = None) -> None:
        """``packed``: neighbour views as ``sucre_pack_view`` records (one gather per landing pixel: -7 % on the match kernel, the
        records built once per view and cached) or as their plain depth and colour planes (two gathers).  None = the engine knob
        ``PACKED_VIEWS``.  Records pay off for a survey, whose targets share views; for ONE target, building them (0.36 ms for 65
        views at 1080p) costs eight times what they save (45 us).  Same match sets, ranges and colours either way."""
        assert 1 <= len(views) <= self.capacity, (len(views), self.capacity)
        self.min_cover = float(min_cover)
        self.n_views = len(views)   # the workspace layout is a function of (H, W, n_views) and grows with n_views
        tgt = target.to_struct()
        packed = (PACKED_VIEWS if packed is None else bool(packed)) and not self.float_colour   # (float32 colour images keep the two-gather form)
        table = (_lib.SucreView * self.n_views)(*[v.to_struct(packed) for v in views])
        if packed:
            with torch.cuda.device(self.device):
                for v in views:
                    v.wait_packed()
        nbytes = C.sizeof(table)
        if self._views_copied is not None:
            self._views_copied.synchronize()   # the previous table has left the staging buffer (it was the first thing
        self._views_host[:nbytes].copy_(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))   # of that image)
        self._views_dev = self._views_buf[:nbytes]
        with torch.cuda.device(self.device):
            self._views_dev.copy_(self._views_host[:nbytes], non_blocking=True)
            self._views_copied = torch.cuda.Event()
            self._views_copied.record()
        self._keepalive = [target, views]
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            want = torch.float32 if self.float_colour else torch.uint8
            assert all(v.rgb.dtype == want for v in views), f'this restoration takes {want} colour images'
            if self.light or self.float_colour:
                lws = C.c_void_p(self.lws.data_ptr())
                fn = (self.lib.sucre_match_views_light_fcolour if self.both else
                      self.lib.sucre_match_views_fcolour if self.float_colour else self.lib.sucre_match_views_light)
                _lib.check(fn(ws, lws, H, W, n, C.byref(tgt), C.c_void_p(self._views_dev.data_ptr()), 0, n, self._sp()))
                _lib.check(self.lib.sucre_finalize_matches_ext(ws, lws, H, W, n, float(min_cover), self._ext_mode, self._sp()))
            else:
                _lib.check(self.lib.sucre_match_views(ws, H, W, n, C.byref(tgt), C.c_void_p(self._views_dev.data_ptr()),
                                                      0, n, self._sp()))
                _lib.check(self.lib.sucre_finalize_matches_fmt(ws, H, W, n, float(min_cover), self._fmt, self._sp()))

    def import_matches(self, target: DeviceView, lists: list, min_cover: float = -1.0) -> None:
        """Fills the store from explicit per-view match lists instead of matching: ``lists[k] = (u1, v1, z, rgb_u8)``
        (int16[n], int16[n], float32[n], uint8[n,3]) -- what one group of a reference matches file provides after
        ``cP = unproject_depth(u2, v2, d)`` and ``z = ||cP||`` (loader.py:103-118, sucre.py:53).  A fifth element, a
        float32 (3, n) tensor, fills the extension planes of a ``light`` restoration (the camera points cP) or of a
        ``float_colour`` one (the colours I; ``rgb_u8`` may then be None); a restoration that is both takes (6, n): cP, then I."""
        assert 1 <= len(lists) <= self.capacity, (len(lists), self.capacity)
        self.min_cover = float(min_cover)
        self.n_views = len(lists)
        self._keepalive = [target, lists]
        self._views_dev = None
        ws, H, W, n = self._geom
        ext_mode = self._ext_mode
        with torch.cuda.device(self.device):
            for k, item in enumerate(lists):
                u1, v1, z, rgb = item[:4]
                ext = item[4] if len(item) > 4 else None
                u1 = u1.to(self.device, torch.int16).contiguous(); v1 = v1.to(self.device, torch.int16).contiguous()
                z = z.to(self.device, torch.float32).contiguous()
                assert z.numel() == u1.numel() == v1.numel()
                if rgb is not None:
                    rgb = rgb.to(self.device, torch.uint8).contiguous()
                    assert rgb.shape == (u1.numel(), 3)
                self._keepalive.append((u1, v1, z, rgb))
                rgbp = C.c_void_p(rgb.data_ptr()) if rgb is not None else None
                if self.lws is not None:
                    planes = 6 if self.both else 3   # both: the camera points, then the float32 colours
                    assert ext is not None and ext.shape == (planes, u1.numel()), f'this restoration needs ({planes}, n) extension planes'
                    ext = ext.to(self.device, torch.float32).contiguous()
                    self._keepalive.append(ext)
                    _lib.check(self.lib.sucre_import_view_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, k,
                                                              C.c_void_p(u1.data_ptr()), C.c_void_p(v1.data_ptr()),
                                                              C.c_void_p(z.data_ptr()), rgbp, C.c_void_p(ext.data_ptr()),
                                                              u1.numel(), ext_mode, self._sp()))
                else:
                    _lib.check(self.lib.sucre_import_view(ws, H, W, n, k, C.c_void_p(u1.data_ptr()), C.c_void_p(v1.data_ptr()),
                                                          C.c_void_p(z.data_ptr()), rgbp, u1.numel(), self._sp()))
            if self.lws is not None:
                _lib.check(self.lib.sucre_finalize_matches_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n,
                                                               float(min_cover), self._ext_mode, self._sp()))
            else:
                _lib.check(self.lib.sucre_finalize_matches_fmt(ws, H, W, n, float(min_cover), self._fmt, self._sp()))

    def match_map(self, k: int) -> torch.Tensor:
        """(H,W) int32: linear pixel index v2*W2+u2 in view k matched to every target pixel, -1 = none
        (dense form of sfm.Matches).  ``match`` must have been called (it uploads the view table)."""
        assert self._views_dev is not None, 'call match() first'
        out = torch.empty((self.H, self.W), dtype=torch.int32, device=self.device)
        tgt = self._keepalive[0].to_struct()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sucre_match_map(self.H, self.W, self.n_views, C.byref(tgt),
                                                C.c_void_p(self._views_dev.data_ptr()), int(k),
                                                C.c_void_p(out.data_ptr()), self._sp()))
        return out

    def view_counts(self) -> torch.Tensor:
        return self._region(_lib.WS_VIEW_COUNT, torch.int64, self.n_views)

    def view_keep(self) -> torch.Tensor:
        return self._region(_lib.WS_VIEW_KEEP, torch.int32, self.n_views)

    def store_format(self) -> torch.Tensor:
        """uint32[4] on the device: how the last ``match`` / ``import_matches`` laid the observations out -- _lib.STORE_F32,
        STORE_U16MM or STORE_Z24 (float32 ranges as 24-bit offsets of their bit patterns: the device's choice for an 'f32'
        store whose ranges span less than 2^24 patterns; same results bit for bit), the offset, the smallest and the largest
        range bit pattern."""
        return self._region(_lib.WS_STORE_FORMAT, torch.int32, 4)

    def n_obs_device(self) -> torch.Tensor:
        return self._region(_lib.WS_N_OBS, torch.int64, 1)

    def n_obs(self) -> int:
        return int(self.n_obs_device().item())

    def export_view(self, k: int):
        """Dense (z (H,W) float32, rgb (H,W,3) uint8) planes of view k's matches."""
        z = torch.empty((self.H, self.W), dtype=torch.float32, device=self.device)
        rgb = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sucre_export_view(ws, H, W, n, int(k), C.c_void_p(z.data_ptr()),
                                                  C.c_void_p(rgb.data_ptr()), self._sp()))
        return z, rgb

    def export_view_ext(self, k: int) -> torch.Tensor:
        """(3, H, W) float32: the extension planes of view k (camera points with ``light``, colours with
        ``float_colour``), zero where the view has no observation."""
        assert self.lws is not None, 'this restoration keeps no extension planes'
        out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.device)
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sucre_export_view_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, int(k),
                                                      C.c_void_p(out.data_ptr()), self._sp()))
        return out

    def export_view_colour(self, k: int) -> torch.Tensor:
        """(3, H, W) float32: the float32 colours of view k of a restoration that is both ``light`` and ``float_colour`` (its
        second set of extension planes; ``export_view_ext`` returns the first, the camera points), zero where the view has no
        observation."""
        assert self.both, 'only a light restoration on float32 colours keeps a second set of extension planes'
        out = torch.empty((3, self.H, self.W), dtype=torch.float32, device=self.device)
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sucre_export_view_ext2(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, int(k),
                                                       C.c_void_p(out.data_ptr()), self._sp()))
        return out

    def check_store(self) -> torch.Tensor:
        """uint32 per view: 0 = sound, bit 0 = non-finite range, bit 1 = negative range, bit 2 = the number of stored
        ranges differs from the view's match count (the checks of loader.py:89-101, one launch for all views)."""
        verdict = torch.empty(self.n_views, dtype=torch.int32, device=self.device)
        scratch = torch.empty(self.n_views, dtype=torch.int64, device=self.device)
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sucre_check_store(ws, H, W, n, C.c_void_p(verdict.data_ptr()),
                                                  C.c_void_p(scratch.data_ptr()), self._sp()))
        return verdict

    # -- fit (sucre.py:36-82, 124-157) --------------------------------------------------------------------------
    def fit_init(self, target: DeviceView, params0=None, J0: torch.Tensor | None = None) -> None:
        npar = 19 if (self.light or self.float_colour) else 9
        default = np.concatenate([np.full(9, 0.1), np.zeros(6), [1.0, 0.0, 0.0, 1.0]])  # sucre.py:41-46
        p0 = default.copy() if params0 is None else np.asarray(params0, np.float64).reshape(-1)
        if self.float_colour and not self.light and p0.size == 9:
            p0 = np.concatenate([p0, default[9:]])   # no light: identity pose, unit beam (never updated)
        p0 = p0.astype(np.float32).reshape(-1)[:npar] if params0 is None else p0.astype(np.float32).reshape(npar)
        p0c = (C.c_float * npar)(*p0.tolist())
        j0 = None
        if J0 is None and self.float_colour:
            J0 = target.rgb   # SUCRe.__init__: J starts at the image (sucre.py:47); NaN where depth <= 0 by the kernel
        if J0 is not None:
            j0 = J0.to(self.device, torch.float32).contiguous()
            assert j0.shape == (self.H, self.W, 3)
            self._keepalive.append(j0)
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            j0p = C.c_void_p(j0.data_ptr()) if j0 is not None else None
            if self.light or self.float_colour:
                _lib.check(self.lib.sucre_fit_init_light(ws, C.c_void_p(self.lws.data_ptr()), H, W, n,
                                                         None if self.float_colour else C.c_void_p(target.rgb.data_ptr()),
                                                         C.c_void_p(target.depth.data_ptr()), p0c, j0p, self._sp()))
            else:
                _lib.check(self.lib.sucre_fit_init(ws, H, W, n, C.c_void_p(target.rgb.data_ptr()),
                                                   C.c_void_p(target.depth.data_ptr()), p0c, j0p, self._sp()))
        self.steps_done = 0

    def fit(self, num_iter: int = 200, lr: float = 0.05, use_closed_form: bool = False, betas=(0.9, 0.999),
            eps: float = 1e-8, record_trace: bool = True, keep_J: bool = False, paired: bool | None = None) -> torch.Tensor | None:
        """Enqueues ``num_iter`` Adam iterations without any host sync; returns the (num_iter,10) float64
        device trace (cost, B, beta, gamma per iteration) or None.  In closed-form mode the C ABI appends the
        final ``update_J`` of sucre.py:156 to a ``sucre_fit_run`` call unless ``keep_J``: then J stays the J(theta_k)
        the last iteration k solved, next to theta_{k+1} -- what the reference holds when it plots at a --save-interval
        stop (sucre.py:141,153).  A fit split into several calls: with ``keep_J`` in every call and one ``update_J()``
        behind the last, the launches are those of the unsplit fit and so are the bits.  Without it the appended
        ``update_J`` leaves J(theta_{k+1}) where the unsplit fit has J(theta_k); the light-model kernel re-solves J from
        zero and does not notice, the plain one-pass kernel (fit.hip, AccOne) measures its sums from the J it finds, so
        the split fit ends in the same state up to rounding only (tests/test_gpu_snapshots.py).
        ``paired`` (J-parameter mode of the plain model; None: the engine knob ``SUCRE_PAIRED_FIT``): the iterations of this call
        run as pairs of launches (and a single one if ``num_iter`` is odd) or, False, one by one -- nothing is pending between
        calls, and state, J, parameters and trace are bit for bit the same either way (tests/test_gpu_paired.py)."""
        ext = self.light or self.float_colour
        width = 20 if ext else 10
        trace = torch.zeros((num_iter, width), dtype=torch.float64, device=self.device) if record_trace else None
        flags = (_lib.FIT_CLOSED_FORM if use_closed_form else 0) | self._fmt_flag | self._ext_flag
        if keep_J and use_closed_form:
            flags |= _lib.FIT_KEEP_J
        if not ext and not use_closed_form and not (PAIRED_FIT if paired is None else paired):
            flags |= _lib.FIT_UNPAIRED
        ws, H, W, n = self._geom
        tp = C.c_void_p(trace.data_ptr()) if trace is not None else None
        with torch.cuda.device(self.device):
            if ext:
                _lib.check(self.lib.sucre_fit_run_light(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, self.steps_done,
                                                        int(num_iter), float(lr), float(betas[0]), float(betas[1]),
                                                        float(eps), flags, tp, self._sp()))
            else:
                _lib.check(self.lib.sucre_fit_run(ws, H, W, n, self.steps_done, int(num_iter), float(lr),
                                                  float(betas[0]), float(betas[1]), float(eps), flags, tp,
                                                  self._sp()))
        self.steps_done += int(num_iter)
        if trace is not None and self.float_colour and not self.light:
            trace = trace[:, :10]   # the light columns are constants here
        self.trace = trace
        return trace

    def update_J(self) -> None:
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            if self.light or self.float_colour:
                _lib.check(self.lib.sucre_update_J_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, self._ext_flag, self._sp()))
            else:
                _lib.check(self.lib.sucre_update_J_fmt(ws, H, W, n, self._fmt, self._sp()))

    def residuals(self):
        """Per-pixel and per-view residuals of the fit as it stands (``sucre_fit_residuals``): ``(count, ssr, view_stats)`` on
        the device -- int32 (H,W) observations per pixel over the kept views, float32 (H,W,3) sum of r^2 per channel, float64
        (n_views,4) per view {observations, sum r^2 R, G, B}, zeros for a view that is not kept -- with
        r = I - l (J e^(-beta z) + B (1 - e^(-gamma z))) (sucre.py:79-82, 144) at the current parameters and J.  One pass over
        the dense store, enqueued on the current stream without a host wait; the workspace is only read, so the call may sit
        anywhere between fits.  Works on a matched and on an imported store."""
        count = torch.empty((self.H, self.W), dtype=torch.int32, device=self.device)
        ssr = torch.empty((self.H, self.W, 3), dtype=torch.float32, device=self.device)
        stats = torch.empty((self.n_views, 4), dtype=torch.float64, device=self.device)
        nbytes = self.lib.sucre_residual_scratch_bytes(self.H, self.W, self.n_views)
        if nbytes == 0:
            raise _lib.SucreError(self.lib.sucre_last_error().decode())
        # torch's caching allocator keeps the block for this stream until the launches queued here have run
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ws, H, W, n = self._geom
        outs = (C.c_void_p(count.data_ptr()), C.c_void_p(ssr.data_ptr()), C.c_void_p(stats.data_ptr()), C.c_void_p(scratch.data_ptr()))
        with torch.cuda.device(self.device):
            if self.light or self.float_colour:
                _lib.check(self.lib.sucre_fit_residuals_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, self._ext_flag, *outs, self._sp()))
            else:
                _lib.check(self.lib.sucre_fit_residuals(ws, H, W, n, self._fmt, *outs, self._sp()))
        return count, ssr, stats

    def uncertainty(self):
        """The float64 statistics behind the standard errors of B, beta, gamma and J at the fit as it stands
        (``sucre_fit_uncertainty``): ``(count, jterms, sums)`` on the device -- int32 (H,W) observations per pixel over the kept
        views, float32 (H,W,3,4) per channel ``{1 / A_p, k_B, k_beta, k_gamma}`` (0 where ``count`` is 0), float64
        [``_lib.UNCERTAINTY_WORDS``] = N, P, pixels without a finite positive A_p, then per channel H_BB, H_Bbeta, H_Bgamma,
        H_betabeta, H_betagamma, H_gammagamma, SSR: the Gauss-Newton normal matrix of (B, beta, gamma) with every pixel's J
        eliminated (csrc/uncertainty.h).  ``water_uncertainty(sums)`` and ``j_standard_error(jterms, count, result)`` turn them
        into covariances and sigma_J.  One pass over the dense store, enqueued on the current stream without a host wait; the
        workspace is only read; two calls give the same bits.  The light model is refused: its ten parameters would have to join
        (B, beta, gamma)."""
        if self.light:
            raise NotImplementedError('uncertainty: not built for the light model -- the lamp\'s ten parameters would have to join '
                                      'B, beta, gamma, and errors conditional on a fixed lamp would understate')
        count = torch.empty((self.H, self.W), dtype=torch.int32, device=self.device)
        jterms = torch.empty((self.H, self.W, 3, 4), dtype=torch.float32, device=self.device)
        sums = torch.empty(_lib.UNCERTAINTY_WORDS, dtype=torch.float64, device=self.device)
        nbytes = self.lib.sucre_uncertainty_scratch_bytes(self.H, self.W, self.n_views)
        if nbytes == 0:
            raise _lib.SucreError(self.lib.sucre_last_error().decode())
        # torch's caching allocator keeps the block for this stream until the launches queued here have run
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ws, H, W, n = self._geom
        outs = (C.c_void_p(count.data_ptr()), C.c_void_p(jterms.data_ptr()), C.c_void_p(sums.data_ptr()), C.c_void_p(scratch.data_ptr()))
        with torch.cuda.device(self.device):
            if self.float_colour:
                _lib.check(self.lib.sucre_fit_uncertainty_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, self._ext_flag, *outs, self._sp()))
            else:
                _lib.check(self.lib.sucre_fit_uncertainty(ws, H, W, n, self._fmt, *outs, self._sp()))
        return count, jterms, sums

    def trim_outliers(self, k_sigma: float, residuals=None):
        """One round of the outlier trim (``sucre_trim_outliers``): drops from the store every observation of a kept view whose
        residual at the fit as it stands has r_c^2 > tau^2_c = float32(k_sigma^2 S_c / N) in any channel (N, S_c: observations
        and sums of r^2 over the kept views) -- except at a pixel that would lose all its observations, which keeps them all --
        and finalises the store again with the ``min_cover`` of the last ``match`` / ``import_matches``: view totals, kept views
        (a view may now fall below ``min_cover``), ``n_obs``, the store's format, the compaction and the plans are what a plain
        run on the survivors would have.  ``residuals``: what ``residuals()`` returned for this very state (run here if None).
        Returns ``(dropped, view_dropped, thresholds)`` on the device: int32 (H,W), int64 (n_views), float32 [3] = tau^2.
        Everything is enqueued on the current stream without a host wait.  The fit must start over: ``steps_done`` is 0 and the
        caller calls ``fit_init`` again -- with the same initial values the refit is bit for bit a plain run on a store into
        which only the survivors were imported.  ``match_map`` keeps returning the untrimmed matches (it is geometry)."""
        k_sigma = float(k_sigma)
        if not (np.isfinite(k_sigma) and k_sigma > 0.0):
            raise ValueError(f'trim_outliers: k_sigma must be finite and > 0, not {k_sigma!r}')
        if self.min_cover is None:
            raise _lib.SucreError('trim_outliers: call match() or import_matches() first')
        stats = (self.residuals() if residuals is None else residuals)[2]
        assert stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and stats.shape == (self.n_views, 4)
        dropped = torch.empty((self.H, self.W), dtype=torch.int32, device=self.device)
        view_dropped = torch.empty(self.n_views, dtype=torch.int64, device=self.device)
        thresholds = torch.empty(3, dtype=torch.float32, device=self.device)
        nbytes = self.lib.sucre_trim_scratch_bytes(self.H, self.W, self.n_views)
        if nbytes == 0:
            raise _lib.SucreError(self.lib.sucre_last_error().decode())
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ws, H, W, n = self._geom
        args = (k_sigma, C.c_void_p(stats.data_ptr()), C.c_void_p(dropped.data_ptr()), C.c_void_p(view_dropped.data_ptr()),
                C.c_void_p(thresholds.data_ptr()), C.c_void_p(scratch.data_ptr()))
        with torch.cuda.device(self.device):
            if self.lws is not None:
                lws = C.c_void_p(self.lws.data_ptr())
                _lib.check(self.lib.sucre_trim_outliers_ext(ws, lws, H, W, n, self._ext_flag, *args, self._sp()))
                _lib.check(self.lib.sucre_finalize_matches_ext(ws, lws, H, W, n, self.min_cover, self._ext_mode, self._sp()))
            else:
                _lib.check(self.lib.sucre_trim_outliers(ws, H, W, n, self._fmt, *args, self._sp()))
                _lib.check(self.lib.sucre_finalize_matches_fmt(ws, H, W, n, self.min_cover, self._fmt, self._sp()))
        self.steps_done = 0
        return dropped, view_dropped, thresholds

    def _gain_scratch(self) -> torch.Tensor:
        nbytes = self.lib.sucre_gain_scratch_bytes(self.H, self.W, self.n_views)
        if nbytes == 0:
            raise _lib.SucreError(self.lib.sucre_last_error().decode())
        # torch's caching allocator keeps the block for this stream until the launches queued here have run
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def view_gains(self, limit: float = 2.0):
        """One multiplicative gain per kept view and channel at the fit as it stands (``sucre_view_gains``): the least-squares
        answer ``g = sum I Ihat / sum Ihat^2`` to ``I = g Ihat`` over the view's observations, with
        Ihat = l (J e^(-beta z) + B (1 - e^(-gamma z))) (sucre.py:79-82, 144) at the current parameters and J -- the number the
        residual pass evaluates.  Returns ``(gains, inv, sums)`` on the device: float64 (n_views,3) clamped to
        [1 / limit, limit], float32 (n_views,3) = float32(1 / g), float64 (n_views,7) per view {observations, sum I Ihat R, G, B,
        sum Ihat^2 R, G, B}.  g = 1 and inv = 1 exactly for a view that is not kept or has nothing to estimate from.  A pure
        read, enqueued on the current stream without a host wait; two calls give the same bits."""
        limit = float(limit)
        if not (np.isfinite(limit) and limit >= 1.0):
            raise ValueError(f'view_gains: limit must be finite and >= 1, not {limit!r}')
        gains = torch.empty((self.n_views, 3), dtype=torch.float64, device=self.device)
        inv = torch.empty((self.n_views, 3), dtype=torch.float32, device=self.device)
        sums = torch.empty((self.n_views, 7), dtype=torch.float64, device=self.device)
        scratch = self._gain_scratch()
        ws, H, W, n = self._geom
        outs = (limit, C.c_void_p(gains.data_ptr()), C.c_void_p(inv.data_ptr()), C.c_void_p(sums.data_ptr()), C.c_void_p(scratch.data_ptr()))
        with torch.cuda.device(self.device):
            if self.lws is not None:
                _lib.check(self.lib.sucre_view_gains_ext(ws, C.c_void_p(self.lws.data_ptr()), H, W, n, self._ext_flag, *outs, self._sp()))
            else:
                _lib.check(self.lib.sucre_view_gains(ws, H, W, n, self._fmt, *outs, self._sp()))
        return gains, inv, sums

    def apply_view_gains(self, inv: torch.Tensor) -> torch.Tensor:
        """Divides per-view gains out of the store (``sucre_apply_view_gains``): every observation of a kept view k has its
        colours multiplied by ``inv[k]`` (float32 (n_views,3) on the device, what ``view_gains`` returned) -- uint8 colours
        become min(255, rintf(float(k) inv_c)), float32 colours I inv_c -- and the store is finalised again with the
        ``min_cover`` of the last ``match`` / ``import_matches``, which rebuilds what the fit reads; ranges, counts and the set of
        kept views stay.  Returns ``view_clipped`` on the device: int64 (n_views), the uint8 values per view that met the 255
        clamp.  Everything is enqueued on the current stream without a host wait.  The fit must start over: ``steps_done`` is 0
        and the caller calls ``fit_init`` again -- with the same initial values the refit is bit for bit a plain run on a store
        into which the corrected colours were imported."""
        if self.min_cover is None:
            raise _lib.SucreError('apply_view_gains: call match() or import_matches() first')
        assert inv.is_cuda and inv.dtype == torch.float32 and inv.is_contiguous() and inv.shape == (self.n_views, 3)
        view_clipped = torch.empty(self.n_views, dtype=torch.int64, device=self.device)
        scratch = self._gain_scratch()
        ws, H, W, n = self._geom
        args = (C.c_void_p(inv.data_ptr()), C.c_void_p(view_clipped.data_ptr()), C.c_void_p(scratch.data_ptr()))
        with torch.cuda.device(self.device):
            if self.lws is not None:
                lws = C.c_void_p(self.lws.data_ptr())
                _lib.check(self.lib.sucre_apply_view_gains_ext(ws, lws, H, W, n, self._ext_flag, *args, self._sp()))
                _lib.check(self.lib.sucre_finalize_matches_ext(ws, lws, H, W, n, self.min_cover, self._ext_mode, self._sp()))
            else:
                _lib.check(self.lib.sucre_apply_view_gains(ws, H, W, n, *args, self._sp()))
                _lib.check(self.lib.sucre_finalize_matches_fmt(ws, H, W, n, self.min_cover, self._fmt, self._sp()))
        self.steps_done = 0
        return view_clipped

    def params(self) -> torch.Tensor:
        """B[3], beta[3], gamma[3] (+ cam2light[6], sigma[4] with the light model) on the device."""
        if self.light or self.float_colour:
            self._note_stream()
            off = self.lib.sucre_light_params_offset(self.H, self.W, self.n_views)
            return self.lws[off:off + (76 if self.light else 36)].view(torch.float32)
        return self._region(_lib.WS_PARAMS, torch.float32, 9)

    def J(self) -> torch.Tensor:
        out = torch.empty((self.H, self.W, 3), dtype=torch.float32, device=self.device)
        ws, H, W, n = self._geom
        with torch.cuda.device(self.device):
            _lib.check(self.lib.sucre_export_J(ws, H, W, n, C.c_void_p(out.data_ptr()), self._sp()))
        return out


WATER_NAMES = ('B', 'beta', 'gamma')   # the order of every 3-vector and 3x3 matrix of water_uncertainty


def water_uncertainty(sums) -> dict:
    """Covariance of (B, beta, gamma) per channel from the 24 float64 words of ``Restoration.uncertainty`` (or of
    ``sucre.pooled_uncertainty``), on the host in float64 numpy: ``s2 = SSR / dof`` with ``dof = N - P - 3``, ``cov = s2 H^-1``.
    H is scaled by its diagonal before it is inverted (its entries span orders of magnitude; the scaled matrix has condition
    number 1e3 - 3e4 on the project's scenes).  Returns a dict of arrays, first axis the channel R, G, B, parameters in the order
    ``WATER_NAMES``: ``cov`` (3,3,3), ``se`` (3,3), ``corr`` (3,3,3), ``cond`` (3,) of the scaled matrix, ``s2`` (3,), ``normal``
    (3,3,3) = H, ``well_posed`` (3,) bool, and the scalars ``dof``, ``n_obs``, ``n_pixels`` (int).  A channel with ``dof <= 0``, with
    an H or SSR that is not finite, with an H that is not positive definite, or of an image in which some observed pixel had no
    finite positive A_p (word 2) gets NaN and ``well_posed`` False; nothing raises.
    Gauss-Newton at the point the sums were taken at, not necessarily a minimum; observations count as independent with one
    variance per channel, so errors that views share (depth maps, poses) are not in it."""
    w = np.asarray(sums.detach().cpu().numpy() if torch.is_tensor(sums) else sums, np.float64).reshape(-1)
    if w.size != _lib.UNCERTAINTY_WORDS:
        raise ValueError(f'water_uncertainty: {_lib.UNCERTAINTY_WORDS} words expected, not {w.size}')
    head_ok = bool(np.isfinite(w[:3]).all())
    n_obs, n_pixels = (int(round(w[0])), int(round(w[1]))) if head_ok else (0, 0)
    dof = n_obs - n_pixels - 3
    out = {'cov': np.full((3, 3, 3), np.nan), 'se': np.full((3, 3), np.nan), 'corr': np.full((3, 3, 3), np.nan),
           'cond': np.full(3, np.nan), 's2': np.full(3, np.nan), 'normal': np.zeros((3, 3, 3)), 'well_posed': np.zeros(3, bool),
           'dof': dof, 'n_obs': n_obs, 'n_pixels': n_pixels}
    for c in range(3):
        hBB, hBb, hBg, hbb, hbg, hgg, ssr = w[3 + 7 * c:10 + 7 * c]
        Hc = np.array([[hBB, hBb, hBg], [hBb, hbb, hbg], [hBg, hbg, hgg]])
        out['normal'][c] = Hc
        d = np.diag(Hc)
        if not (head_ok and w[2] == 0 and dof > 0 and np.isfinite(Hc).all() and np.isfinite(ssr) and ssr >= 0 and (d > 0).all()):
            continue
        scale = np.sqrt(d)
        Hs = Hc / np.outer(scale, scale)
        try:
            np.linalg.cholesky(Hs)   # positive definite, or not determined
            inv = np.linalg.inv(Hs)
        except np.linalg.LinAlgError:
            continue
        if not (np.isfinite(inv).all() and (np.diag(inv) > 0).all()):
            continue
        s2 = ssr / dof
        cov = s2 * inv / np.outer(scale, scale)
        root = np.sqrt(np.diag(inv))
        out['cov'][c], out['se'][c], out['s2'][c] = cov, np.sqrt(np.diag(cov)), s2
        out['corr'][c] = inv / np.outer(root, root)
        out['cond'][c] = np.linalg.cond(Hs)
        out['well_posed'][c] = True
    return out


def j_standard_error(jterms: torch.Tensor, count: torch.Tensor, result: dict) -> torch.Tensor:
    """float32 (H,W,3): ``sigma_J = sqrt(s2 / A_p + k_p^T cov k_p)`` per pixel and channel from the ``jterms`` and ``count`` of
    ``Restoration.uncertainty`` and the dict of ``water_uncertainty`` -- torch in float64 where ``jterms`` lives.  NaN where
    ``count`` is 0, where the pixel had no finite positive A_p, and in a channel that is not well posed."""
    t = jterms.to(torch.float64)
    cov = torch.as_tensor(np.asarray(result['cov'], np.float64), device=t.device)   # (3 channels, 3, 3)
    s2 = torch.as_tensor(np.asarray(result['s2'], np.float64), device=t.device)
    k = t[..., 1:]                                                       # (H, W, 3, 3)
    var = s2 * t[..., 0] + torch.einsum('hwci,cij,hwcj->hwc', k, cov, k)
    seen = ((count > 0) & (t[..., 0] > 0).all(dim=-1)).unsqueeze(-1)
    posed = torch.as_tensor(np.asarray(result['well_posed'], bool), device=t.device)
    return torch.where(seen & posed, var.sqrt(), torch.full_like(var, float('nan'))).to(torch.float32)


def fit_batch(restorations: list, num_iter: int = 200, lr: float = 0.05, use_closed_form: bool = False, betas=(0.9, 0.999),
              eps: float = 1e-8, record_trace: bool = True, keep_J: bool = False) -> list:
    """``Restoration.fit`` for several INDEPENDENT images at once -- the reference's loop over images (sucre.py:243-261) with
    the iterations of all of them advancing together, one launch per iteration (``sucre_fit_run_batch``).  Every image keeps
    its own B, beta, gamma, J, Adam state and trace, bit for bit what ``fit`` gives it alone; what the batch saves is the
    per-launch cost (small images are dominated by it) and the idle end of every image's pass.  The images must have one
    size, sit on one device, stand at the same step and use the same observation format; their view counts may differ.
    Returns the list of (num_iter, 10) device traces (or of None)."""
    rs = list(restorations)
    if not rs:
        raise ValueError('fit_batch: no image')
    r0 = rs[0]
    for r in rs:
        if r.light or r.float_colour:
            raise NotImplementedError('fit_batch: the extension-plane modes (light model, float32 colours) are fitted one by one')
        # (not asserts: under python -O images at different Adam steps would be stepped with one bias correction, silently --
        # ADVICE round 5.  The float32 forms of the store -- words, 24- or 26-bit codes -- may mix: each workspace says its own.)
        if (r.H, r.W, str(r.device), r._fmt_flag, r.steps_done) != (r0.H, r0.W, str(r0.device), r0._fmt_flag, r0.steps_done):
            raise ValueError('fit_batch: one image size, device, observation format and Adam step per batch -- got '
                             f'{(r.H, r.W, str(r.device), r.obs_format, r.steps_done)} next to {(r0.H, r0.W, str(r0.device), r0.obs_format, r0.steps_done)}')
    if len({r.ws.data_ptr() for r in rs}) != len(rs):
        raise ValueError('fit_batch: every image needs its own workspace')
    n = len(rs)
    traces = [torch.zeros((num_iter, 10), dtype=torch.float64, device=r0.device) if record_trace else None for _ in rs]
    flags = (_lib.FIT_CLOSED_FORM if use_closed_form else 0) | r0._fmt_flag
    if keep_J and use_closed_form:
        flags |= _lib.FIT_KEEP_J
    lib = r0.lib
    table = torch.empty(lib.sucre_batch_bytes(n), dtype=torch.uint8, device=r0.device)
    ws = (C.c_void_p * n)(*[r.ws.data_ptr() for r in rs])
    tr = (C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in traces])
    nv = (C.c_int * n)(*[int(r.n_views) for r in rs])
    with torch.cuda.device(r0.device):
        sp = None
        for r in rs:
            sp = r._sp()
        _lib.check(lib.sucre_fit_run_batch(C.c_void_p(table.data_ptr()), n, ws, tr, r0.H, r0.W, nv, r0.steps_done, int(num_iter),
                                           float(lr), float(betas[0]), float(betas[1]), float(eps), flags, sp))
    for r, t in zip(rs, traces):
        r.steps_done += int(num_iter)
        r.trace = t
        r._batch_table = table   # the launches read the table: it lives until the workspace's next batch (replaced, not appended:
                                 # a fit driven one iteration per call would otherwise keep one table per call -- ADVICE round 5)
    return traces


def select_ranks(J: torch.Tensor, ranks: list[int]) -> torch.Tensor:
    """(3, len(ranks)) float32: per channel of the (H,W,3) float32 device image ``J``, the values at the given 0-based
    ranks among the valid pixels (no NaN in any channel), ascending -- exact order statistics by radix select on the
    device (csrc/plot.hip); the image does not move."""
    lib = _lib.load()
    assert J.is_cuda and J.dtype == torch.float32 and J.is_contiguous() and J.dim() == 3 and J.shape[2] == 3
    assert 1 <= len(ranks) <= 8
    out = torch.empty((3, len(ranks)), dtype=torch.float32, device=J.device)
    scratch = torch.empty(lib.sucre_select_scratch_bytes(), dtype=torch.uint8, device=J.device)
    arr = (C.c_uint64 * len(ranks))(*[int(r) for r in ranks])
    with torch.cuda.device(J.device):
        _lib.check(lib.sucre_select_ranks(C.c_void_p(J.data_ptr()), J.shape[0], J.shape[1], len(ranks), arr,
                                          C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), _stream_ptr()))
    return out


def count_valid(J: torch.Tensor) -> int:
    """Pixels of the (H,W,3) float32 device image ``J`` without a NaN in any channel (``valid``, sucre.py:86-87)."""
    lib = _lib.load()
    assert J.is_cuda and J.dtype == torch.float32 and J.is_contiguous() and J.dim() == 3 and J.shape[2] == 3
    count = torch.empty(1, dtype=torch.int64, device=J.device)
    with torch.cuda.device(J.device):
        _lib.check(lib.sucre_count_valid(C.c_void_p(J.data_ptr()), J.shape[0], J.shape[1], C.c_void_p(count.data_ptr()),
                                         _stream_ptr()))
    return int(count.item())


def plot_stretch(J: torch.Tensor, lo, hi) -> torch.Tensor:
    """(H,W,3) uint8: SUCRe.plot_J's clip / shift / scale / x255 / truncate (sucre.py:88-94) of the device image ``J``
    between the per-channel percentiles ``lo`` and ``hi`` (3 float32 each); invalid pixels black."""
    lib = _lib.load()
    assert J.is_cuda and J.dtype == torch.float32 and J.is_contiguous() and J.dim() == 3 and J.shape[2] == 3
    out = torch.empty(J.shape, dtype=torch.uint8, device=J.device)
    lo_c = (C.c_float * 3)(*[float(x) for x in lo])
    hi_c = (C.c_float * 3)(*[float(x) for x in hi])
    with torch.cuda.device(J.device):
        _lib.check(lib.sucre_plot_stretch(C.c_void_p(J.data_ptr()), J.shape[0], J.shape[1], lo_c, hi_c,
                                          C.c_void_p(out.data_ptr()), _stream_ptr()))
    return out


class PoolSelect:
    """The pooled radix select (``sucre_pool_select_*``, csrc/pool.hip) phase by phase: exact order statistics of the valid
    pixels of many device images without concatenating or moving them.  ``begin()``; then for ``pass_`` 0..3: ``add(Js, pass_)``
    any number of times, the histograms ``hist`` summed over the ranks by the caller, ``locate(pass_, ranks)``; ``values()``.
    Pass 0 does not depend on the ranks: ``hist[0, 0].sum()`` after its ``add`` calls is the pooled number of valid pixels, and
    ``ranks`` (0-based, at most 8, each below that number) are given to ``locate(0, ranks)`` only."""

    def __init__(self, device):
        lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.SucreError('PoolSelect runs on a GPU device (there is no CPU fallback)')
        n = int(lib.sucre_pool_select_bytes())
        self.state = torch.empty((n + 7) // 8, dtype=torch.int64, device=self.device)
        # a VIEW of the state's head, uint64 hist[3][8][256] (counts stay far below 2^63): what dist.all_reduce_sum sums
        self.hist = self.state[:_lib.POOL_HIST_WORDS].view(3, _lib.POOL_MAX_RANKS, 256)
        self.n_ranks = None
        self._out = None
        self._keep = []

    def _sp(self) -> C.c_void_p:
        return C.c_void_p(self.state.data_ptr())

    def begin(self) -> None:
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sucre_pool_select_begin(self._sp(), _stream_ptr()))
        self.n_ranks = None
        self._out = None
        self._keep = []

    def add(self, Js: list, pass_: int, n_ranks: int | None = None) -> None:
        """Adds the histograms of pass ``pass_`` over the (H,W,3) float32 contiguous device images ``Js`` (any sizes, empty ones
        and an empty list included), in chunks of the table limit.  ``n_ranks``: what ``locate(0, ranks)`` fixed, unless given."""
        lib = _lib.load()
        n_ranks = int(n_ranks if n_ranks is not None else (self.n_ranks or 1))
        Js = list(Js)
        for J in Js:
            if not (J.is_cuda and J.device == self.device and J.dtype == torch.float32 and J.is_contiguous() and J.dim() == 3 and J.shape[2] == 3):
                raise ValueError('PoolSelect.add: every image must be an (H,W,3) float32 contiguous tensor on the select\'s device')
        with torch.cuda.device(self.device):
            if not Js:   # (the argument checks still run)
                _lib.check(lib.sucre_pool_select_pass(self._sp(), int(pass_), None, 0, None, n_ranks, _stream_ptr()))
            for i0 in range(0, len(Js), _lib.POOL_MAX_IMAGES):
                chunk = Js[i0:i0 + _lib.POOL_MAX_IMAGES]
                arr = (_lib.PoolImage * len(chunk))()
                for e, J in zip(arr, chunk):
                    if J.numel() and J.data_ptr() % 16:   # a view into a larger buffer: the kernel loads 16 bytes at once
                        J = J.clone()
                        self._keep.append(J)
                    e.J, e.n_px = (J.data_ptr() if J.numel() else None), J.shape[0] * J.shape[1]
                # (torch's caching allocator keeps a freed block for this stream until the launches queued here have run)
                table = torch.empty(lib.sucre_pool_table_bytes(len(chunk)), dtype=torch.uint8, device=self.device)
                _lib.check(lib.sucre_pool_select_pass(self._sp(), int(pass_), C.c_void_p(table.data_ptr()), len(chunk), arr, n_ranks,
                                                      _stream_ptr()))

    def locate(self, pass_: int, ranks=None) -> None:
        lib = _lib.load()
        arr = None
        if int(pass_) == 0:
            if ranks is None or not 1 <= len(ranks) <= _lib.POOL_MAX_RANKS:
                raise ValueError(f'PoolSelect.locate: pass 0 takes 1..{_lib.POOL_MAX_RANKS} ranks')
            self.n_ranks = len(ranks)
            arr = (C.c_uint64 * len(ranks))(*[int(r) for r in ranks])
            self._out = torch.empty((3, self.n_ranks), dtype=torch.float32, device=self.device)
        elif self.n_ranks is None:
            raise ValueError('PoolSelect.locate: pass 0 comes first (it takes the ranks)')
        with torch.cuda.device(self.device):
            _lib.check(lib.sucre_pool_select_locate(self._sp(), int(pass_), self.n_ranks, arr, C.c_void_p(self._out.data_ptr()),
                                                    _stream_ptr()))

    def values(self) -> torch.Tensor:
        """(3, n_ranks) float32 device tensor: per channel the values at the ranks, once ``locate(3)`` has been called."""
        return self._out


def pooled_percentiles(Js: list, q=(1.0, 99.0), group=None):
    """``(P, n)``: ``P[c, i] = float32(np.percentile(pool_c.astype(float64), q[i]))`` over the pool of the valid pixels (no NaN in
    any channel) of all the (H,W,3) float32 device images ``Js`` -- of any sizes, on one device -- of ALL ranks of ``group``, as
    a (3, len(q)) float32 numpy array, and ``n``, the pooled number of valid pixels.  Exact: the order statistics come from the
    pooled radix select (``PoolSelect``; the histograms of every pass are summed over the ranks by ``dist.all_reduce_sum``, so
    every rank obtains the same numbers), the ranks and the interpolation are numpy's 'linear' method in float64
    (``sucre.percentile_plan64``), rounded once.  At most 4 percentiles.  ``Js`` may be empty on a rank whose group has other
    members (the device is then the current one); ``ValueError`` if the pool holds no valid pixel."""
    from . import dist as sdist
    from .sucre import percentile_plan64
    q = [float(x) for x in q]
    if not 1 <= len(q) <= _lib.POOL_MAX_RANKS // 2:
        raise ValueError(f'pooled_percentiles: 1..{_lib.POOL_MAX_RANKS // 2} percentiles, got {len(q)}')
    Js = list(Js)
    dev = Js[0].device if Js else torch.device('cuda', torch.cuda.current_device())
    sel = PoolSelect(dev)
    sel.begin()
    n, plans = 0, None
    for pass_ in range(4):
        sel.add(Js, pass_, n_ranks=2 * len(q))
        sdist.all_reduce_sum(sel.hist, group)
        if pass_ == 0:
            n = int(sel.hist[0, 0].sum().item())
            if n == 0:
                raise ValueError('pooled_percentiles: the pool holds no valid pixel')
            plans = [percentile_plan64(n, x) for x in q]
            sel.locate(0, [r for below, above, _ in plans for r in (below, above)])
        else:
            sel.locate(pass_)
    stats = sel.values().cpu().numpy().astype(np.float64)   # (3, 2 len(q))
    P = np.empty((3, len(q)), np.float32)
    for c in range(3):
        for i, (_, _, t) in enumerate(plans):
            P[c, i] = np.float32(_lerp64(stats[c, 2 * i], stats[c, 2 * i + 1], t))
    return P, n


def _lerp64(a: float, b: float, t: float) -> float:
    """numpy's ``_lerp`` in float64: ``a + (b - a) t``, formed from the upper end when ``t >= 0.5``."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    diff = b - a
    return b - diff * (1 - t) if t >= 0.5 else a + diff * t


def invert_images(views: list, params, light: bool = False) -> list:
    """Single-view inversion (``sucre_invert_images``): J of every view of ``views`` from its OWN depth map and colours at the
    given water parameters -- ``SUCRe.update_J`` (sucre.py:66-77) with one observation per pixel, the image itself:
    ``J = (I - l B (1 - e^(-gamma z))) a / a^2``, ``a = l e^(-beta z)``, ``z = ||K^-1 d [u+.5, v+.5, 1]||``, NaN where ``depth <= 0``;
    bit for bit what ``Restoration.update_J`` leaves after ``match(view, [view])`` wherever the image matches itself in full.
    No ``Restoration``, no matching, no neighbour.  ``params``: 9 host floats B, beta, gamma -- 19 with ``light`` (+ cam2light,
    sigma) -- as an array or a CPU tensor.  The views may differ in size; their colours are all uint8 or all float32
    (``ValueError`` otherwise).  One launch per 4096 views on the current stream, no host wait.  Returns one (H,W,3) float32
    device tensor per view."""
    views = list(views)
    if not views:
        raise ValueError('invert_images: no view')
    dtypes = {v.rgb.dtype for v in views}
    if len(dtypes) != 1 or not dtypes <= {torch.uint8, torch.float32}:
        raise ValueError(f'invert_images: the views\' colours must be all uint8 or all float32, not {sorted(str(d) for d in dtypes)}')
    if torch.is_tensor(params):
        params = params.detach().cpu().numpy()
    p = np.asarray(params, np.float64).reshape(-1)
    need = 19 if light else 9
    if p.size != need:
        raise ValueError(f'invert_images: {need} parameters expected ({"B, beta, gamma, cam2light, sigma" if light else "B, beta, gamma"}), got {p.size}')
    dev = views[0].depth.device
    if dev.type != 'cuda' or any(v.depth.device != dev or v.rgb.device != dev for v in views):
        raise _lib.SucreError('invert_images: the views must sit on one GPU device (there is no CPU fallback)')
    lib = _lib.load()
    pc = (C.c_float * need)(*p.astype(np.float32).tolist())
    flags = (_lib.INVERT_LIGHT if light else 0) | (_lib.INVERT_FLOAT_COLOUR if torch.float32 in dtypes else 0)
    outs = []
    with torch.cuda.device(dev):
        for i0 in range(0, len(views), _lib.INVERT_MAX_IMAGES):
            chunk = views[i0:i0 + _lib.INVERT_MAX_IMAGES]
            n = len(chunk)
            arr = (_lib.InvertImage * n)()
            keep = []
            for e, v in zip(arr, chunk):
                s = v.to_struct()   # (checks shapes and dtypes; Kinv derived the way the reference derives it, cached)
                depth, rgb = v.depth, v.rgb
                if depth.data_ptr() % 16 or rgb.data_ptr() % 16:   # views into larger buffers: the kernel loads 16 bytes at once
                    depth, rgb = depth.clone(), rgb.clone()
                    keep += [depth, rgb]
                H, W = depth.shape
                J = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
                e.depth, e.rgb, e.J, e.H, e.W, e.Kinv = depth.data_ptr(), rgb.data_ptr(), J.data_ptr(), H, W, s.Kinv
                outs.append(J)
            # (the table, like `keep`: torch's caching allocator keeps a freed block for this stream until the launches queued
            # here have run)
            table = torch.empty(lib.sucre_invert_bytes(n), dtype=torch.uint8, device=dev)
            _lib.check(lib.sucre_invert_images(C.c_void_p(table.data_ptr()), n, arr, pc, flags, _stream_ptr()))
    return outs


def view_consistency(target: DeviceView, J_target: torch.Tensor, views: list, Js: list):
    """Cross-view colour consistency of restored images (``sucre_view_consistency``): every pixel of ``target`` is matched
    against every view of ``views`` -- ``Restoration.match_map``'s matches, by the same device function, no map in memory -- and
    the restored colours ``a = J_target[v1,u1]`` and ``b = Js[k][v2,u2]`` of every pair without a NaN are compared.  Returns
    ``(count, ssd, stats)`` on the device: int32 (H,W) views with a valid pair at the pixel, float32 (H,W,3) sum of (a - b)^2 over
    them, float64 (n_views, 26) per view {matches, valid pairs, sum d^2, a^2, b^2, a b of J per channel, the same four sums of
    the raw uint8 colours / 255 of the same pairs}.  ``Js[k]``: (H_k,W_k,3) float32 on the views' device, or None -- the view then
    takes no part and its row is zero.  The views may differ in size; their colours must be uint8 (a view with float32 colours --
    a resized input -- is given without them: its raw sums are zero).  Two launches on the current stream, no host wait; no
    ``Restoration`` and no workspace.  Two calls on the same inputs give the same bits."""
    views, Js = list(views), list(Js)
    n = len(views)
    if not 1 <= n <= MAX_VIEWS:
        raise ValueError(f'view_consistency: {n} views, need 1..{MAX_VIEWS}')
    if len(Js) != n:
        raise ValueError(f'view_consistency: {n} views but {len(Js)} restored images')
    H, W = target.depth.shape
    dev = target.depth.device
    if dev.type != 'cuda':
        raise _lib.SucreError('view_consistency: the views must sit on a GPU device (there is no CPU fallback)')

    def plain(v: DeviceView) -> _lib.SucreView:   # uint8 colours or none; never the packed form
        if v.rgb.dtype == torch.uint8:
            return v.to_struct()
        H_, W_ = v.depth.shape
        return camera_struct(v.K, v.R, v.t, H_, W_, v.depth.data_ptr(), 0, Kinv=v.Kinv, tinv=v.tinv)

    def restored(J, v: DeviceView, what: str) -> torch.Tensor:
        if J.device != dev or J.dtype != torch.float32 or tuple(J.shape) != tuple(v.depth.shape) + (3,):
            raise ValueError(f'view_consistency: {what} must be float32 {tuple(v.depth.shape) + (3,)} on {dev}, '
                             f'not {J.dtype} {tuple(J.shape)} on {J.device}')
        return J.contiguous()

    J_target = restored(J_target, target, 'J_target')
    Js = [None if J is None else restored(J, v, f'Js[{k}]') for k, (J, v) in enumerate(zip(Js, views))]
    lib = _lib.load()
    tgt = plain(target)
    table = (_lib.SucreView * n)(*[plain(v) for v in views])
    ptrs = (C.c_void_p * n)(*[None if J is None else J.data_ptr() for J in Js])
    count = torch.empty((H, W), dtype=torch.int32, device=dev)
    ssd = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    stats = torch.empty((n, _lib.CONSISTENCY_STATS), dtype=torch.float64, device=dev)
    nbytes = lib.sucre_consistency_scratch_bytes(H, W, n)
    if nbytes == 0:
        raise _lib.SucreError(lib.sucre_last_error().decode())
    with torch.cuda.device(dev):
        # the view table and the pointer array in one pinned staging buffer (torch's host allocator keeps it until the copy has
        # run), and, like the scratch, in device blocks the caching allocator keeps for this stream until the launches have run
        host = torch.frombuffer(bytearray(bytes(table) + bytes(ptrs)), dtype=torch.uint8).pin_memory()
        staged = host.to(dev, non_blocking=True)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.sucre_view_consistency(H, W, n, C.byref(tgt), C.c_void_p(staged.data_ptr()), C.c_void_p(J_target.data_ptr()),
                                              C.c_void_p(staged.data_ptr() + C.sizeof(table)), C.c_void_p(count.data_ptr()),
                                              C.c_void_p(ssd.data_ptr()), C.c_void_p(stats.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                              _stream_ptr()))
    return count, ssd, stats


def mosaic_max_cells() -> int:
    """Cells a mosaic may have: SUCRE_MOSAIC_MAX_CELLS, 2^27 unless set (37 bytes per cell: key, pixel word and the five outputs;
    124 with a blend: 64 more for the accumulator's eight int64 words and 23 for the four blended outputs; a fill adds at most 30:
    19 for its three outputs and up to 11 for the pyramid, 32-byte records on a third as many cells -- 49 with a blend, whose two
    filled outputs take 15 and whose own levels 4; a multi-band blend of K bands adds 64 (K + 1) + 12: its K + 1 accumulators and
    ``J_multiband`` -- and 19 more with a fill, ``J_multiband_filled`` and the pass's levels and dropped raw picture; a surface test
    adds 12: the ``top`` word, ``surface`` and ``culled``; a support of M views 8 M + 16 more: the ``rank`` words, ``support``,
    ``surface_source``, ``culled_above`` and ``surface_top``; a gain compensation adds 72: the ``span`` pair and the
    reference accumulator ``acc_gain``, eight int64 words of its own)."""
    return int(os.environ.get('SUCRE_MOSAIC_MAX_CELLS', 1 << 27))


MOSAIC_BLEND_RANGE = (1e-6, 1e6)   # blend depths H a mosaic takes, metres
MOSAIC_MAX_SAMPLES = 1 << 20       # samples of one cell from which the blend's int64 sums may pass 2^62 (csrc/mosaic.h)
MOSAIC_FILL_RANGE = (1e-6, 1e6)    # fill reaches R a mosaic takes, metres
MOSAIC_FEATHER_RANGE = (1, 1024)   # feather widths F a blend takes, source pixels (csrc/mosaic.h, "The feather")
MOSAIC_BANDS_RANGE = (1, 6)        # detail bands K a multi-band blend takes (csrc/bands.h): filter steps 1 .. 2^(K-1) source pixels
MOSAIC_SURFACE_RANGE = (1e-6, 1e6)   # surface tolerances T a mosaic takes, metres (csrc/surface.h)
MOSAIC_SUPPORT_RANGE = (1, 4)        # views M whose agreement a supported surface asks for (csrc/support.h)
MOSAIC_GAIN_ROUNDS_RANGE = (1, 64)      # rounds R of the per-image gain compensation (csrc/gains_mosaic.h)
MOSAIC_GAIN_LIMIT_RANGE = (1.0, 16.0)   # limits L a gain is clamped to: 1/L <= g <= L
MOSAIC_GAIN_LIMIT = 2.0                 # the limit unless one is given
MOSAIC_GAIN_MAX_PIXELS = 1 << 26        # pixels of one image from which the gain sums' int64 words may pass 2^62
MOSAIC_GAIN_SOLVES = ('rounds', 'direct')   # how the first round's gains are found (csrc/gains_direct.h: 'direct')
MOSAIC_GAIN_PRIOR = 2.0 ** -20              # mu of the direct solve: the weight of (g - 1)^2 against the data term
MOSAIC_GAIN_DIRECT_CELL_BYTES = 292         # the direct solve's slots: 32 + 256 + 4 bytes per cell
MOSAIC_GAIN_DIRECT_MEMORY = 0.8             # the share of the free device memory the direct solve's state may take
MOSAIC_REJECT_RANGE = (1e-6, 1e6)           # colour tolerances T a consensus rejection takes, units of J (csrc/reject.h)
MOSAIC_REJECT_CELL_BYTES = 292              # the consensus' slots: 32 + 256 + 4 bytes per cell, freed after the consensus
MOSAIC_REJECT_MEMORY = 0.8                  # the share of the free device memory the consensus' state may take
MOSAIC_VALUES = {   # field of MosaicOptions -> (what it is, range, integral, unit, type of the checked value, the command line's letter,
    # the command line's words for it), in the order checked.  A choice has its values in place of the range and None for
    # ``integral``, the unit and the words.
    'blend': ('blend depth H', MOSAIC_BLEND_RANGE, False, 'metres', np.float32, 'H', 'a finite depth'),
    'fill': ('fill reach R', MOSAIC_FILL_RANGE, False, 'metres', float, 'R', 'a finite reach'),
    'feather': ('feather width F', MOSAIC_FEATHER_RANGE, True, 'source pixels', int, 'F', 'an integer'),
    'bands': ('band count K', MOSAIC_BANDS_RANGE, True, 'bands', int, 'K', 'an integer'),
    'surface': ('surface tolerance T', MOSAIC_SURFACE_RANGE, False, 'metres', np.float32, 'T', 'a finite tolerance'),
    'support': ('supporting views M', MOSAIC_SUPPORT_RANGE, True, 'views', int, 'M', 'an integer'),
    'gains': ('gain rounds R', MOSAIC_GAIN_ROUNDS_RANGE, True, 'rounds', int, 'R', 'an integer'),
    'gain_limit': ('gain limit L', MOSAIC_GAIN_LIMIT_RANGE, False, 'times', float, 'L', 'a finite limit'),
    'gain_solve': ('gain solve', MOSAIC_GAIN_SOLVES, None, None, str, 'S', None),
    'reject': ('reject tolerance T', MOSAIC_REJECT_RANGE, False, 'colour units', np.float32, 'T', 'a finite tolerance'),
}
MOSAIC_NEEDS = [   # (field, the field it only goes with, why), in the order MosaicOptions.checked looks at them, after every value
    ('feather', 'blend', 'a feather is a factor of the blend\'s weight; give the blend depth too (blend=H)'),
    ('bands', 'blend', 'the bands are blended with the blend\'s weights; give the blend depth too (blend=H)'),
    ('support', 'surface', 'the support decides which top the surface test measures against; give the tolerance too (surface=T)'),
    ('gain_limit', 'gains', 'the limit clamps the gains the rounds find; give the rounds too (gains=R)'),
    ('gain_solve', 'gains', 'the solve finds the gains of the first round; give the rounds too (gains=R)'),
]


def _mosaic_refusal(field: str, text: str, needs: str = None) -> ValueError:
    """A ValueError whose ``field`` tells a caller which of its flags to name: the field of ``MosaicOptions`` at fault, or 'grid'
    where ``Mosaic.begin`` finds no grid to make.  ``needs``: the field that ``field`` was given without (a row of ``MOSAIC_NEEDS``),
    None for every other refusal."""
    e = ValueError(text)
    e.field, e.needs = field, needs
    return e


def _mosaic_value(field: str, value):
    """``value`` as ``MOSAIC_VALUES[field]`` describes it, or ValueError unless it is finite, within the range and, where the
    table says so, an integral number and no bool -- or, for a choice, one of its strings."""
    what, span, integral, unit, kind, _, _ = MOSAIC_VALUES[field]
    if integral is None:
        if not isinstance(value, str) or value not in span:
            raise _mosaic_refusal(field, f'mosaic {what} must be one of {" or ".join(span)}, not {value!r}')
        return value
    lo, hi = span
    try:
        x = float(value)
    except (TypeError, ValueError):
        x = float('nan')
    # The comparison is in float64.  A value that has the checked type already -- the float32 H of a checked record on its way
    # through begin -- meets the ends as that type holds them, so that float32(1e-6), which lies below 1e-6, passes a second check.
    if type(value) is kind:
        lo, hi = kind(lo), kind(hi)
    ok = bool(np.isfinite(x)) and float(lo) <= x <= float(hi)
    if ok and integral:
        ok = not isinstance(value, bool) and x == int(x)
    if not ok:
        raise _mosaic_refusal(field, f'mosaic {what} must be {"an integer" if integral else "finite and"} within [{lo:g}, {hi:g}] {unit}, '
                                     f'not {value}')
    return kind(x)


# One value each as the table describes it (the returned type: its fifth column), or ValueError with ``field``; a whole request goes
# through ``MosaicOptions.checked``.

def mosaic_blend_depth(blend) -> np.float32:
    """``blend`` as the float32 blend depth H, or ValueError unless it is finite and within ``MOSAIC_BLEND_RANGE``."""
    return _mosaic_value('blend', blend)


def mosaic_feather_px(feather) -> int:
    """``feather`` as the feather width F in source pixels, or ValueError unless it is an integral number within
    ``MOSAIC_FEATHER_RANGE``."""
    return _mosaic_value('feather', feather)


def mosaic_fill_reach(fill) -> float:
    """``fill`` as the reach R in metres, or ValueError unless it is finite and within ``MOSAIC_FILL_RANGE``."""
    return _mosaic_value('fill', fill)


def mosaic_band_count(bands) -> int:
    """``bands`` as the number K of detail bands of a multi-band blend, or ValueError unless it is an integral number, no bool,
    within ``MOSAIC_BANDS_RANGE``."""
    return _mosaic_value('bands', bands)


def mosaic_surface_tol(surface) -> np.float32:
    """``surface`` as the float32 tolerance T of the surface test in metres, or ValueError unless it is finite and within
    ``MOSAIC_SURFACE_RANGE``."""
    return _mosaic_value('surface', surface)


def mosaic_support_views(support) -> int:
    """``support`` as the number M of views a supported surface rests on, or ValueError unless it is an integral number, no bool,
    within ``MOSAIC_SUPPORT_RANGE``."""
    return _mosaic_value('support', support)


def mosaic_gain_rounds(gains) -> int:
    """``gains`` as the number R of rounds of the gain compensation, or ValueError unless it is an integral number, no bool, within
    ``MOSAIC_GAIN_ROUNDS_RANGE``."""
    return _mosaic_value('gains', gains)


def mosaic_gain_limit(gain_limit) -> float:
    """``gain_limit`` as the limit L of a gain, or ValueError unless it is finite and within ``MOSAIC_GAIN_LIMIT_RANGE``."""
    return _mosaic_value('gain_limit', gain_limit)


def mosaic_gain_solve_name(gain_solve) -> str:
    """``gain_solve`` itself, or ValueError unless it is one of the strings of ``MOSAIC_GAIN_SOLVES``."""
    return _mosaic_value('gain_solve', gain_solve)


def mosaic_reject_tol(reject) -> np.float32:
    """``reject`` as the float32 tolerance T of the colour consensus in units of ``J``, or ValueError unless it is finite and within
    ``MOSAIC_REJECT_RANGE``."""
    return _mosaic_value('reject', reject)


def mosaic_gain_solve(sums, G, limit):
    """One solve of the gain compensation (csrc/gains_mosaic.h) on the host, in float64: ``sums`` (n, 10) integers -- per image the
    sample count n_i, ``sum Xq Mq`` x 3, ``sum Xq Xq`` x 3 (the last three words are not read) --, ``G`` (n, 3) the gains of the pass
    that made them, ``limit`` L.  Per channel: ``g_i = float(A) / float(B)`` where ``n_i > 0``, ``A > 0`` and ``B > 0``, otherwise
    the gain the image had; over the images with ``n_i > 0`` ``s = fsum(float(n_i) g_i) / fsum(float(n_i))`` and ``g_i / s`` -- the
    gauge: the overlap-weighted mean gain is 1 --; then ``min(max(g_i, 1 / L), L)``, then float32.  An image with ``n_i = 0`` keeps
    exactly 1.  Returns (n, 3) float32 (numpy)."""
    sums = [[int(x) for x in row] for row in np.asarray(sums).tolist()]
    old = np.asarray(G, dtype=np.float32).reshape(len(sums), 3)
    L = float(limit)
    lo = 1.0 / L
    out = np.ones((len(sums), 3), np.float32)
    seen = [i for i, row in enumerate(sums) if row[0] > 0]
    n_all = math.fsum(float(sums[i][0]) for i in seen)
    for c in range(3):
        g = {}
        for i in seen:
            A, B = sums[i][1 + c], sums[i][4 + c]
            g[i] = float(A) / float(B) if A > 0 and B > 0 else float(old[i, c])
        if not seen:
            continue
        s = math.fsum(float(sums[i][0]) * g[i] for i in seen) / n_all
        for i in seen:
            out[i, c] = np.float32(min(max(g[i] / s if s > 0 else g[i], lo), L))
    return out


def _device_free_bytes(device) -> int:
    """The free memory of ``device`` in bytes, as the driver reports it now."""
    with torch.cuda.device(device):
        return int(torch.cuda.mem_get_info()[0])


def mosaic_gain_pair_matrix(pairs, word: int) -> np.ndarray:
    """Word ``word`` of ``pairs`` -- (n, n, 4) integers, the upper triangle as ``sucre_mosaic_gain_pairs`` leaves it -- as the
    symmetric (n, n) float64 matrix (an int64 becomes the nearest float64, as ``float()`` of the integer would)."""
    upper = np.triu(np.asarray(pairs)[:, :, word].astype(np.int64))
    return upper.astype(np.float64) + np.triu(upper, 1).T.astype(np.float64)


def mosaic_gain_direct_unclamped(pairs, diag, prior=MOSAIC_GAIN_PRIOR):
    """The solution of the direct solve's normal equations before gauge and clamp: ``(x, kept)``, ``x`` (n, 3) float64 -- per
    channel, over the images with ``n_i > 0`` and ``Q_i > 0``, the ``g`` of ``(A + mu diag(Q)) g = mu Q`` (``A_ii = Q_i - P_ii``,
    ``A_ij = -P_ij``) by ``numpy.linalg.solve``; NaN for every other image --, ``kept`` the channels whose solve raises or returns
    a gain that is not finite and positive (their column is NaN)."""
    diag = np.asarray(diag).astype(np.int64).reshape(-1, 4)
    mu = float(prior)
    x = np.full((len(diag), 3), np.nan, np.float64)
    kept = []
    for c in range(3):
        act = np.nonzero((diag[:, 0] > 0) & (diag[:, 1 + c] > 0))[0]
        if len(act) == 0:
            continue
        Q = diag[act, 1 + c].astype(np.float64)
        M = -mosaic_gain_pair_matrix(pairs, c)[np.ix_(act, act)]
        M[np.diag_indices(len(act))] += Q * (1.0 + mu)
        try:
            g = np.linalg.solve(M, mu * Q)
        except np.linalg.LinAlgError:
            g = None
        if g is None or not bool(np.all(np.isfinite(g) & (g > 0))):
            kept.append(c)
            continue
        x[act, c] = g
    return x, kept


def mosaic_gain_solve_direct(pairs, diag, G, limit, prior=MOSAIC_GAIN_PRIOR):
    """The direct solve of the gain compensation (csrc/gains_direct.h) on the host, in float64: ``pairs`` (n, n, 4) integers, the
    upper triangle -- per pair of images ``P_ij`` x 3 and the cells they share --, ``diag`` (n, 4) integers -- per image the sample
    count n_i and ``Q_i = sum Xq Xq`` x 3 --, ``G`` (n, 3) the gains the images have, ``limit`` L, ``prior`` mu.  Per channel, over the
    images with ``n_i > 0`` and ``Q_i > 0``: ``A_ii = Q_i - P_ii``, ``A_ij = -P_ij``, and ``(A + mu diag(Q)) g = mu Q`` by
    ``numpy.linalg.solve`` (``mosaic_gain_direct_unclamped``) -- the minimum of ``g^T A g + mu sum Q_i (g_i - 1)^2``; A alone is
    singular exactly when the images can be made to agree, and the prior pulls a group of images that shares nothing with the rest
    towards 1.  A channel whose solve raises or returns a gain that is not finite and positive keeps the gains it had, untouched,
    and is reported.  Then the gauge of ``mosaic_gain_solve`` -- over the images with ``n_i > 0`` the n-weighted ``fsum`` mean is 1 --,
    the clamp to ``[1 / L, L]`` and float32.  What an image outside the solve keeps: one with ``n_i = 0`` keeps the gain it had, to
    the bit (it is in no shared cell that counts, and outside the gauge); one with ``n_i > 0`` and ``Q_i = 0`` enters the gauge
    with the gain it had, as an image whose sums are not positive does in ``mosaic_gain_solve``, and so comes out as that gain
    over the gauge's mean, clamped.  Returns ``(gains (n, 3) float32 (numpy), kept)``, ``kept`` the list of the reported channels."""
    x, kept = mosaic_gain_direct_unclamped(pairs, diag, prior)
    counts = np.asarray(diag).astype(np.int64).reshape(-1, 4)[:, 0]
    old = np.asarray(G, dtype=np.float32).reshape(len(counts), 3)
    L = float(limit)
    lo = 1.0 / L
    out = old.copy()
    seen = np.nonzero(counts > 0)[0].tolist()
    if not seen:
        return out, kept
    weight = [float(counts[i]) for i in seen]
    n_all = math.fsum(weight)
    for c in range(3):
        if c in kept:
            continue
        g = [float(old[i, c]) if np.isnan(x[i, c]) else float(x[i, c]) for i in seen]
        s = math.fsum(w * gi for w, gi in zip(weight, g)) / n_all
        for i, gi in zip(seen, g):
            out[i, c] = np.float32(min(max(gi / s if s > 0 else gi, lo), L))
    return out, kept


def mosaic_gain_groups(pairs, diag) -> int:
    """The connected groups of the overlap graph: over the images with ``diag[i][0] > 0``, joined where ``pairs[i][j][3] > 0``
    (a breadth-first walk over the boolean adjacency: every image's row is read once)."""
    live = np.asarray(diag).astype(np.int64).reshape(-1, 4)[:, 0] > 0
    adj = mosaic_gain_pair_matrix(pairs, 3) > 0
    todo, groups = live.copy(), 0
    while todo.any():
        groups += 1
        front = np.zeros_like(todo)
        front[np.argmax(todo)] = True
        while front.any():
            todo &= ~front
            front = adj[front].any(axis=0) & todo
    return groups


def mosaic_gain_rms(sums) -> list:
    """``[sqrt(sum_i word(7 + c) / sum_i word 0) / 16384 for c in 0..2]`` of one pass's ``sums`` (n, 10), Python integers under a
    float64 root; zeros when no sample lies in a shared cell."""
    rows = [[int(x) for x in row] for row in np.asarray(sums).tolist()]
    n = sum(row[0] for row in rows)
    return [math.sqrt(sum(row[7 + c] for row in rows) / n) / 16384.0 if n else 0.0 for c in range(3)]


def mosaic_band_plan(H, F, K) -> list:
    """The ``K + 1`` pairs ``(H_j, F_j)`` a multi-band blend of blend depth ``H``, feather ``F`` (None: none) and ``K`` detail bands
    blends its bands with, detail band 0 (the finest) first and the residual last: the residual takes the user's ``(H, F)``, detail
    band j ``H_j = max(float32(H) 2^(j-K), float32(1e-6))`` -- an exact scaling: the transition halves with every finer band -- and
    ``F_j = max(F >> (K - j), 1)``.  ``H_j``: np.float32; ``F_j``: int, or None without a feather."""
    H, K = mosaic_blend_depth(H), mosaic_band_count(K)
    F = None if F is None else mosaic_feather_px(F)
    floor = np.float32(1e-6)
    plan = [(max(np.float32(H * np.float32(2.0 ** (j - K))), floor), None if F is None else max(F >> (K - j), 1)) for j in range(K)]
    return plan + [(H, F)]


@dataclass(frozen=True)
class MosaicOptions:
    """What a mosaic can be asked for beyond the best view, None: not asked for.  ``blend``, the blend depth H in metres;
    ``feather``, with a blend, the feather width F in source pixels; ``fill``, the reach R in metres of the hole filling;
    ``bands``, with a blend, the number K of detail bands of the multi-band blend; ``surface``, the tolerance T in metres of the
    surface test; ``support``, with a surface, the number M of views the top must rest on; ``gains``, the rounds R of the per-image
    gain compensation; ``gain_limit``, with gains, the limit L of a gain; ``gain_solve``, with gains, 'direct' for the direct solve
    in place of the first round's ('rounds': the rounds alone); ``reject``, the tolerance T in units of ``J`` of the colour
    consensus across views.  The ranges, units and checked types are the rows of ``MOSAIC_VALUES``."""
    blend: float = None
    feather: int = None
    fill: float = None
    bands: int = None
    surface: float = None
    support: int = None
    gains: int = None
    gain_limit: float = None
    gain_solve: str = None
    reject: float = None

    def over(self, **fields) -> 'MosaicOptions':
        """The record with ``fields`` laid over it; TypeError for a name that is no field."""
        return replace(self, **fields) if fields else self

    def asked(self) -> dict:
        """The fields that were asked for (not None), by name, in the record's order."""
        return {f: getattr(self, f) for f in self.__dataclass_fields__ if getattr(self, f) is not None}

    def checked(self, who: str = 'MosaicOptions') -> 'MosaicOptions':
        """The record with every value as the type of its row of ``MOSAIC_VALUES``; the one place that checks a request.
        ValueError (``field``: the option at fault) for a value its row does not take, the rows in the table's order, and then for
        an option given without the one it goes with, the rows of ``MOSAIC_NEEDS`` in their order, in the name of ``who``.  With
        gains and no limit the limit is ``MOSAIC_GAIN_LIMIT``; the solve 'rounds' is None, the rounds alone.  A checked record
        passes a second check unchanged."""
        values = {f: None if getattr(self, f) is None else _mosaic_value(f, getattr(self, f)) for f in MOSAIC_VALUES}
        for field, needs, why in MOSAIC_NEEDS:
            if values[field] is not None and values[needs] is None:
                raise _mosaic_refusal(field, f'{who}: {why}', needs)
        if values['gains'] is not None and values['gain_limit'] is None:
            values['gain_limit'] = MOSAIC_GAIN_LIMIT
        if values['gain_solve'] == 'rounds':
            values['gain_solve'] = None
        return MosaicOptions(**values)


def mosaic_fill_levels(R, gsd, Hm: int, Wm: int) -> int:
    """L, the levels of the fill's pyramid above the ``Hm`` x ``Wm`` mosaic (csrc/fill.h): the smallest integer >= 1 with
    ``gsd 2^L >= R`` in float64 -- every hole up to R metres across is closed then --, capped at the first level that is 1x1."""
    R, gsd, Hm, Wm = mosaic_fill_reach(R), float(gsd), int(Hm), int(Wm)
    if not (np.isfinite(gsd) and gsd > 0) or Hm < 1 or Wm < 1:
        raise ValueError(f'mosaic_fill_levels: gsd {gsd} must be finite and > 0 and the mosaic {Wm} x {Hm} at least 1 x 1')
    cap = max(1, (max(Hm, Wm) - 1).bit_length())   # halvings (rounded up) until the longer side is 1
    L = 1
    while L < cap and gsd * 2.0 ** L < R:
        L += 1
    return L


def mosaic_cells(lo: float, hi: float, gsd: float) -> int:
    """``(int)((hi - lo) / gsd) + 1``, the float32 subtraction and IEEE division the kernels apply to a pixel."""
    with np.errstate(all='ignore'):
        return int((np.float32(hi) - np.float32(lo)) / np.float32(gsd)) + 1


_NAN = float('nan')
MOSAIC_OUTPUTS = {   # key of Mosaic.result() -> (group, trailing shape, dtype, value of an empty cell, PNG of --mosaic, how it is made)
    # groups: 'best' (the best view; begin), 'blend' (begin with a blend), 'bands' (begin with bands), 'fill' (fill), 'blend_fill'
    # (fill with a blend), 'bands_fill' (fill with bands), 'surface' (begin with a surface tolerance), 'support' (begin with a
    # support), 'reject' (begin with a reject tolerance; csrc/reject.h).  Mosaic.result() puts the groups in its own order, not the
    # rows'.  An empty value of None: the kernel writes every cell.  How: 'stretch'
    # (sucre._mosaic_picture), 'bytes', 'source', 'mask', 'height', 'count'.
    'J': ('best', (3,), torch.float32, _NAN, 'mosaic.png', 'stretch'),
    'raw': ('best', (3,), torch.uint8, 0, 'mosaic_raw.png', 'bytes'),
    'source': ('best', (), torch.int32, -1, 'mosaic_source.png', 'source'),
    'pixel': ('best', (), torch.int32, -1, None, None),
    'range': ('best', (), torch.float32, _NAN, None, None),
    'J_blend': ('blend', (3,), torch.float32, _NAN, 'mosaic_blend.png', 'stretch'),
    'raw_blend': ('blend', (3,), torch.uint8, 0, 'mosaic_blend_raw.png', 'bytes'),
    'weight': ('blend', (), torch.float32, 0, None, None),
    'samples': ('blend', (), torch.int32, 0, None, None),
    'J_multiband': ('bands', (3,), torch.float32, _NAN, 'mosaic_multiband.png', 'stretch'),
    'surface': ('surface', (), torch.float32, _NAN, 'mosaic_surface.png', 'height'),
    'culled': ('surface', (), torch.int32, 0, 'mosaic_culled.png', 'count'),
    'fill_level': ('fill', (), torch.int32, None, 'mosaic_filled_mask.png', 'mask'),
    'J_filled': ('fill', (3,), torch.float32, None, 'mosaic_filled.png', 'stretch'),
    'raw_filled': ('fill', (3,), torch.uint8, None, 'mosaic_raw_filled.png', 'bytes'),
    'J_blend_filled': ('blend_fill', (3,), torch.float32, None, 'mosaic_blend_filled.png', 'stretch'),
    'raw_blend_filled': ('blend_fill', (3,), torch.uint8, None, 'mosaic_blend_raw_filled.png', 'bytes'),
    'J_multiband_filled': ('bands_fill', (3,), torch.float32, None, 'mosaic_multiband_filled.png', 'stretch'),
    'support': ('support', (), torch.int32, 0, None, None),
    'surface_source': ('support', (), torch.int32, -1, None, None),
    'culled_above': ('support', (), torch.int32, 0, 'mosaic_culled_above.png', 'count'),
    'surface_top': ('support', (), torch.float32, _NAN, None, None),
    'rejected': ('reject', (), torch.int32, 0, 'mosaic_rejected.png', 'count'),
    'reject_ref': ('reject', (3,), torch.float32, _NAN, None, None),
    'reject_source': ('reject', (), torch.int32, -1, None, None),
    'reject_views': ('reject', (), torch.int32, 0, None, None),
    'reject_overflow': ('reject', (), torch.bool, False, None, None),
}
MOSAIC_REJECT_OUTPUTS = {key: row for key, row in MOSAIC_OUTPUTS.items() if row[0] == 'reject'}   # the rows a colour consensus adds


class Mosaic:
    """The seabed mosaic (``sucre_mosaic_*``, csrc/mosaic.h) phase by phase, in the style of ``PoolSelect``: every pixel with a
    valid depth and a restored colour without NaN is dropped onto the grid ``axes`` (3,3 float32, rows e1, e2, e3) x ``gsd`` metres
    per cell, and the pixel with the smallest (range bits, ordinal, pixel index) wins its cell.  ``run(batches, options)`` drives
    every phase below in its order (``mosaic_of`` and ``sucre.mosaic`` go through it); by hand: ``add_bounds(views, Js)`` any number
    of times; ``begin(bounds=None)`` -- waits for the bounds (or takes the caller's ``(lo_s, lo_t, hi_s, hi_t)``; pixels outside
    are dropped), allocates and returns ``(Hm, Wm)``; then ``splat``, ``resolve`` and ``gather``, each over ALL the images (in any
    batches, every batch with the ordinal of its first image) before the next phase starts; ``result()``, whose keys, shapes,
    dtypes and empty values are the rows of ``MOSAIC_OUTPUTS``.  ``views``:
    ``DeviceView`` with uint8 colours; ``Js``: their (H,W,3) float32 device images.  The words a later all-reduce over ranks would
    combine are tensors: ``bounds_words`` (int32 x 4), ``key`` (int64, min), ``pix`` (int32 bit patterns of uint32, unsigned min).

    What is asked for beyond the best view is ONE ``MosaicOptions``, a record of ten fields (``blend, feather, fill, bands, surface,
    support, gains, gain_limit, gain_solve, reject``; the rows of ``MOSAIC_VALUES``): ``begin``, ``run`` and ``mosaic_of`` take the
    record, or its fields as keywords laid over it -- ``begin(blend=H)`` below is that --, and ``MosaicOptions.checked`` is the one
    place that checks them.  What a phase sees of the images is ONE chain of copies, ``_seen``: ``J`` -> culled (with a surface) ->
    rejected (with a colour consensus) -> gained (once a gain pass has run), every stage in one transient buffer of its own.
    ``add_reject_claim`` and ``add_reject_sums`` see the culled images; ``splat`` -- the one phase that counts what the culling
    stages take --, ``add_span``, ``add_gain_sums``, ``add_gain_slots`` and ``add_gain_diag`` the culled and rejected ones, un-gained;
    ``add_gain_reference`` those times the gains as they stand; ``resolve``, ``gather``, ``accumulate`` and ``accumulate_bands`` the
    gained ones.

    The blend: ``begin(blend=H)`` also allocates ``acc`` ((Hm Wm, 8) int64, zeros: per cell the fixed-point sums ``wq Jq`` x 3,
    ``wq rgb`` x 3, ``wq`` and the sample count -- csrc/mosaic.h, "The blend"; the tensor a later all-reduce (sum) over ranks would
    combine, next to ``key`` (min) and ``pix``) and four more outputs; ``accumulate`` over ALL the images once ``splat`` has seen
    every one of them, then ``normalize()``; ``result()`` then holds ``J_blend``, ``raw_blend``, ``weight`` and ``samples`` as well.

    Hole filling: ``fill(R)`` once ``gather`` (with a blend: ``normalize`` too) is through -- a bounded push-pull over a pyramid of
    the grid (csrc/fill.h) that closes every hole up to ``R`` metres across and reaches at most ``3 x 2^L`` cells beyond the
    footprint; ``result()`` then also holds ``J_filled``, ``raw_filled`` and ``fill_level`` (with a blend ``J_blend_filled`` and
    ``raw_blend_filled``).  The other outputs are not touched.

    The feather: ``begin(blend=H, feather=F)`` -- every sample's weight takes one more factor, ``min(sqrt(dist2) / F, 1)`` of the
    sample's distance in source pixels to the nearest pixel of its image that does not take part or lies outside it (csrc/mosaic.h,
    "The feather"), so the blend no longer steps where a view's footprint ends.  ``accumulate`` then forms the batch's exact integer
    map on the device first, in a buffer sized to the largest batch seen; ``J_blend``, ``raw_blend``, ``weight`` and ``samples`` are
    the feathered ones, ``result()`` holds ``feather`` (= F), and ``feather_counts`` (int64 x 2, device) counts the pixels that took
    part within F pixels of an edge and all of them.  ``feather_map(views, Js, F)`` returns the maps themselves; it needs no
    ``begin``.

    The bands: ``begin(blend=H, bands=K)`` -- a multi-band blend next to the blend (csrc/bands.h).  Every image is split in source
    space into K detail bands and a residual (``band_stack``); band j is blended by the blend's own accumulate with
    ``mosaic_band_plan(H, F, K)[j]`` into slice j of ``acc_bands`` ((K + 1, Hm Wm, 8) int64, zeros; the residual last, its words
    3..7 equal to ``acc``'s), so the low frequencies of a cell are the consensus of every view and the fine detail comes from the
    nearest one.  ``accumulate_bands`` over ALL the images once ``splat`` has seen every one of them -- every image is loaded once
    for all its bands --, then ``combine_bands()``; ``result()`` then holds ``J_multiband`` and ``bands`` (= K), after ``fill`` also
    ``J_multiband_filled``.  ``acc``, ``feather_counts`` and every other output are not touched.  Three band buffers of 12 bytes per
    pixel of the largest batch are held.

    The surface test: ``begin(surface=T)`` -- T in metres (``MOSAIC_SURFACE_RANGE``; csrc/surface.h).  ``top`` (int32 bit patterns of
    uint32, all ones: empty) holds per cell the order key of the smallest coordinate along e3, the highest sample, of all the
    pixels that take part; it is the tensor a later all-reduce (unsigned min) over ranks would combine, next to ``key`` and
    ``pix``.  ``add_surface(views, Js, first_ordinal)`` over ALL the images, after ``begin`` and before ``splat``; from then on
    ``splat``, ``resolve``, ``gather``, ``accumulate`` and ``accumulate_bands`` see, through ``culled_images``, a copy of every
    ``J`` with NaN where a sample lies more than T below its cell's top: such a sample takes part in nothing.  The grid is that of
    all the pixels that take part, and the set of filled cells does not change.  ``result()`` then holds ``surface`` ((Hm,Wm)
    float32, the top's coordinate along e3 -- smaller is higher --, NaN: empty), ``culled`` ((Hm,Wm) int32, the samples culled per
    cell) and ``surface_tol`` (= T, a float); ``surface_counts`` (int64 x 2, device) counts the culled samples and the samples with
    a cell.  One buffer of 12 bytes per padded pixel of the largest batch is held.

    The supported surface: ``begin(surface=T, support=M)`` -- M views (``MOSAIC_SUPPORT_RANGE``; csrc/support.h).  The plain
    minimum lets one spurious high sample of one image own its cell; with a support the top of a cell is the highest level that M
    different images reach (a view listed twice has two ordinals and counts twice), a cell seen by fewer than M images rests on the
    lowest of its per-image tops, and a sample more than T ABOVE the top is culled like one more than T below it.  ``rank``
    ((M, Hm Wm) int64, all ones: empty) holds per cell the M smallest per-image ``order key << 32 | ordinal``, one image each;
    ``add_support(views, Js, first_ordinal, level)`` over ALL the images for level 0, then for level 1, ... (``add_surface`` is not
    called), then ``finish_support()``, which writes ``top``; everything after that is the surface test's.  ``result()`` then also
    holds ``support`` ((Hm,Wm) int32: the images that reach the cell, at most M; 0: empty), ``surface_source`` (int32: the ordinal
    of the image whose top the cell rests on; -1), ``culled_above`` (int32), ``surface_top`` (float32: the plain minimum, level 0;
    NaN) and ``surface_support`` (= M); ``surface`` is the supported top.  ``support_counts`` (int64 x 3, device): samples culled
    below, culled above, samples with a cell; ``surface_counts`` is its first and last word.  With M = 1 every output of the
    surface test keeps its bits.

    The gain compensation: ``begin(gains=R, gain_limit=L)`` -- R rounds (``MOSAIC_GAIN_ROUNDS_RANGE``), every gain within
    ``[1 / L, L]`` (``MOSAIC_GAIN_LIMIT_RANGE``; ``MOSAIC_GAIN_LIMIT`` unless given; csrc/gains_mosaic.h).  One gain per image and
    channel, from the cells that two or more images share, so that the images agree on the colour of the same seabed before
    anything is resolved or blended.  ``begin`` allocates ``span`` ((Hm Wm, 2) int32 bit patterns of uint32: min and max ordinal per
    cell; all ones, 0: empty), ``acc_gain`` ((Hm Wm, 8) int64, the reference pass's accumulator, a tensor of its own: 64 bytes per
    cell besides the blend's ``acc``), ``gain_table`` ((n, 3) float32, ones) and ``gain_sums_words`` ((R + 1, n, 16) int64, ten words
    used) -- the last two at the first pass, which learns n, the images of the request, from its batches.  ``add_span(views, Js,
    first_ordinal)`` over ALL the images once ``splat`` has seen them all; then R times ``gain_pass(batches)`` and ``solve_gains()``,
    and one more ``gain_pass`` that measures the final state (by hand a pass is ``begin_gain_pass(n)``, ``add_gain_reference`` over
    ALL the images, then ``add_gain_sums`` over ALL of them, then ``end_gain_pass()``).  From the first pass on ``resolve``,
    ``gather``, ``accumulate`` and ``accumulate_bands`` see, through ``gained_images``, every (culled) ``J`` times its image's gain.
    ``span``, ``acc_gain`` and the sums are the tensors a later all-reduce (min / max, sum, sum) over ranks would combine.
    ``result()`` then also holds ``gains`` (n,3) float32, ``gain_sums`` (passes so far, n, 10) int64, ``gain_rms`` (passes, 3)
    float64 -- row r: the RMS disagreement in the shared cells at the gains entering pass r --, ``gain_overlap`` (n,) int64 -- the
    samples of every image in shared cells --, ``gain_rounds`` (= R) and ``gain_limit`` (= L).  One more buffer of 12 bytes per
    padded pixel of the largest batch is held.  A finite positive gain makes and removes no NaN, so every output that is not a
    ``J`` keeps its bits, and L = 1 keeps every output's.

    The direct solve: ``begin(gains=R, gain_solve='direct')`` (csrc/gains_direct.h) -- the rounds' objective solved exactly, once,
    in place of the first round's solve: what a drift along a chain of images takes the rounds on the order of N^2 rounds for.  After
    the first pass ``add_gain_slots(views, Js, first_ordinal)`` over ALL the images (the first call allocates ``slot_ord``
    ((Hm Wm, 8) int32 bit patterns, all ones: free), ``slot_sum`` ((Hm Wm, 8, 4) int64), ``slot_over`` ((Hm Wm,) int32),
    ``gain_pairs_words`` ((n, n, 4) int64) and ``gain_diag_words`` ((n, 16) int64, four words used): 292 bytes per cell and
    32 n^2 + 128 n, refused beyond ``MOSAIC_GAIN_DIRECT_MEMORY`` of the free device memory before any of it is allocated), then
    ``gain_pairs()``, then ``add_gain_diag`` over ALL the images, then ``solve_gains_direct()`` (``mosaic_gain_solve_direct``, on the
    host).  ``result()`` then also holds ``gain_solve`` ('direct'), ``gain_direct`` (n,3) float32 -- the table that solve produced --,
    ``gain_pair_index`` (P,2) int32 and ``gain_pair_words`` (P,4) int64 -- the pairs i <= j with a shared cell, ascending: P_ij x 3
    and the cells --, ``gain_diag`` (n,4) int64, ``gain_excluded_cells`` -- shared cells that more than 8 images reach, left out --,
    ``gain_shared_cells`` -- all the shared cells --, ``gain_kept`` -- the channels (0..2) that kept their gains because their system
    has no finite positive solution --, ``gain_components`` -- connected groups of the overlap graph -- and ``gain_prior``.  ``gain_rms[1]`` shows what the solve achieved.

    The colour consensus: ``begin(reject=T)`` -- T in units of ``J`` (``MOSAIC_REJECT_RANGE``; csrc/reject.h).  A transient object
    that the rendered depth maps do not hold has the seabed's height and its own colour; no height test sees it.  ``begin``
    allocates ``reject_slot_ord`` ((Hm Wm, 8) int32 bit patterns, all ones: free), ``reject_slot_sum`` ((Hm Wm, 8, 4) int64) and
    ``reject_slot_over`` ((Hm Wm,) int32): 292 bytes per cell, refused beyond ``MOSAIC_REJECT_MEMORY`` of the free device memory before
    anything is allocated.  After the surface phase and before ``splat``: ``add_reject_claim(views, Js, first_ordinal)`` over ALL the
    images -- a cell's words end as the 8 smallest ordinals that reach it, in any order of arrival --, then ``add_reject_sums`` over
    ALL of them, then ``finish_reject()``: the images of a cell that three or more reach are ordered by their mean brightness there,
    the lower median is the cell's reference, and the slots are freed.  From then on ``splat`` and every later phase, the gains'
    included, see through ``rejected_images`` a copy of every (culled) ``J`` with NaN where a sample of another image differs from
    its cell's reference by more than T in any channel.  The reference image's samples never go, so the grid and the set of filled
    cells do not change.  ``result()`` then also holds the rows of ``MOSAIC_REJECT_OUTPUTS`` -- ``rejected`` (Hm,Wm) int32,
    ``reject_ref`` (Hm,Wm,3) float32 (NaN: no consensus), ``reject_source`` (int32, -1), ``reject_views`` (int32: the images that hold
    slots, at most 8), ``reject_overflow`` (bool: more than 8 reach the cell) --, ``reject_per_image`` (n,2) int64 -- samples in
    cells with a reference, samples rejected -- and ``reject_tol`` (= T).  ``reject_slot_ord`` (min-merge of the sorted words),
    ``reject_slot_sum`` (sum) and ``rejected`` (sum) are the tensors a later all-reduce over ranks would combine.  One more buffer
    of 12 bytes per padded pixel of the largest batch is held."""

    def __init__(self, axes, gsd, device):
        _lib.load()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.SucreError('Mosaic runs on a GPU device (there is no CPU fallback)')
        if self.device.index is None:   # 'cuda' names the current GPU: the views' tensors carry its index
            self.device = torch.device('cuda', torch.cuda.current_device())
        a = torch.as_tensor(axes).detach().cpu().to(torch.float32).reshape(-1)
        if a.numel() != 9 or not bool(torch.isfinite(a).all()):
            raise ValueError('Mosaic: axes must be nine finite numbers (3x3, rows e1, e2, e3)')
        self.axes = a.reshape(3, 3).clone()
        self.gsd = np.float32(gsd)
        if not (np.isfinite(self.gsd) and self.gsd > 0):
            raise ValueError(f'Mosaic: gsd must be finite and > 0, not {gsd}')
        self._axes_c = (C.c_float * 9)(*a.tolist())
        self.bounds_words = torch.tensor([-1, -1, 0, 0], dtype=torch.int32, device=self.device)   # two min keys, two max keys
        self._reset()

    def _reset(self, options: MosaicOptions = MosaicOptions()) -> None:
        """All the state a ``begin`` decides, as it is before the grid is fixed: the checked ``options`` under their public names,
        no tensor, no pass counted, nothing held."""
        self.grid = None
        self.Hm = self.Wm = self.lo = self.hi = None
        self.key = self.pix = None
        self._out = {}        # the outputs allocated so far (rows of MOSAIC_OUTPUTS)
        self._copies = {}     # stage of the chain -> its transient buffer of J copies (_copy)
        self._held = {}       # stage of the chain -> the copies run() holds when one batch is the whole request
        self.blend, self.feather, self.bands, self.surface, self.support = options.blend, options.feather, options.bands, options.surface, options.support
        self.gains, self.gain_limit, self.gain_solve, self.reject = options.gains, options.gain_limit, options.gain_solve, options.reject
        self.inv_h = self.acc = None
        self.feather_counts = self._feather_buf = None
        self.fill_reach = self.fill_levels = self.pyramid = None
        self.band_plan = self.acc_bands = self._band_bufs = None
        self.top = self.surface_counts = None
        self.rank = self.support_counts = None
        self.span = self.acc_gain = self.gain_table = self.gain_sums_words = None
        self._gain_passes, self._gain_open, self._splatted = 0, False, False
        self.slot_ord = self.slot_sum = self.slot_over = self.gain_pairs_words = self.gain_diag_words = None
        self.gain_direct, self.gain_kept, self._paired = None, None, False
        self.reject_slot_ord = self.reject_slot_sum = self.reject_slot_over = self.reject_counts = None
        self._reject_state, self._reject_n = None, 0

    def _images(self, views: list, Js: list):
        views, Js = list(views), list(Js)
        if len(views) != len(Js):
            raise ValueError(f'Mosaic: {len(views)} views but {len(Js)} restored images')
        if not 1 <= len(views) <= MAX_VIEWS:
            raise ValueError(f'Mosaic: {len(views)} images in one call, need 1..{MAX_VIEWS}')
        arr = (_lib.MosaicImage * len(views))()
        keep = []
        for e, v, J in zip(arr, views, Js):
            H, W = v.depth.shape
            if v.rgb.dtype != torch.uint8:
                raise ValueError(f'Mosaic: {v.name or "a view"} has {v.rgb.dtype} colours; the raw mosaic takes uint8')
            if v.depth.device != self.device or J.device != self.device or J.dtype != torch.float32 or tuple(J.shape) != (H, W, 3):
                raise ValueError(f'Mosaic: the restored image of {v.name or "a view"} must be float32 {(H, W, 3)} on {self.device}, '
                                 f'not {J.dtype} {tuple(J.shape)} on {J.device}')
            s = v.to_struct()   # (checks shapes and dtypes; Kinv derived the way the reference derives it, cached)
            J = J.contiguous()
            keep.append(J)
            e.depth, e.rgb, e.J, e.H, e.W = v.depth.data_ptr(), v.rgb.data_ptr(), J.data_ptr(), H, W
            e.Kinv, e.R, e.t = s.Kinv, s.R, s.t
        # (the table, like `keep`: torch's caching allocator keeps a freed block for this stream until the launches queued here
        # have run)
        table = torch.empty(_lib.load().sucre_mosaic_table_bytes(len(views)), dtype=torch.uint8, device=self.device)
        return arr, len(views), table, keep

    def _call(self, entry: str, *args) -> None:
        """One entry of the library on the current stream: ``entry(*args, stream)``, the tensors of ``args`` as their addresses."""
        args = [C.c_void_p(x.data_ptr()) if torch.is_tensor(x) else x for x in args]
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), entry)(*args, _stream_ptr()))

    def _walk(self, entry: str, images, *rest) -> None:
        """One entry that walks images: ``entry(table, n, images, *rest, stream)`` with ``images`` as ``_images`` returns them."""
        arr, n, table, _ = images
        self._call(entry, table, n, arr, *rest)

    def _allocate(self, group: str) -> None:
        """The outputs of ``group`` (``MOSAIC_OUTPUTS``), every cell empty."""
        for key, (of, tail, dtype, empty, _, _) in MOSAIC_OUTPUTS.items():
            if of == group:
                shape = (self.Hm, self.Wm) + tail
                self._out[key] = torch.empty(shape, dtype=dtype, device=self.device) if empty is None \
                    else torch.full(shape, empty, dtype=dtype, device=self.device)

    @staticmethod
    def _offsets(arr) -> list:
        """Per image of ``arr`` the index of its first pixel in a buffer of the band-buffer layout (csrc/bands.h): image after image,
        every one rounded up to ``MOSAIC_BLOCK_PX`` = 256 pixels."""
        first, at = [], 0
        for e in arr:
            first.append(at)
            at += -(-(e.H * e.W) // _lib.MOSAIC_BLOCK_PX) * _lib.MOSAIC_BLOCK_PX
        return first

    def _per_image(self, buf, arr, channels: int = 3) -> list:
        """Per image of ``arr`` its (H,W,channels) view -- (H,W) for one channel -- into ``buf``, a buffer of that layout."""
        return [buf[at * channels:(at + e.H * e.W) * channels].view(*((e.H, e.W, channels) if channels > 1 else (e.H, e.W)))
                for e, at in zip(arr, self._offsets(arr))]

    def _band_bytes(self, images) -> int:
        """The bytes of one float32 x 3 buffer of that layout for ``images`` (``sucre_mosaic_band_bytes``)."""
        arr, n, _, _ = images
        lib = _lib.load()
        n_bytes = lib.sucre_mosaic_band_bytes(n, arr)
        if n_bytes == 0:
            raise _lib.SucreError(f'sucre_mosaic_band_bytes: {lib.sucre_last_error().decode()}')
        return n_bytes

    def _copy(self, stage: str, entry: str, images, head, tail=()) -> list:
        """A walking entry that writes a copy of every ``J`` in that layout: ``entry(.., *head, buffer, *tail, stream)`` into the ONE
        transient buffer of ``stage``, grown to the largest batch seen (12 bytes per padded pixel).  Returns the per-image
        (H,W,3) views into it: the stage's next call overwrites them.  Only enqueues."""
        n_bytes = self._band_bytes(images)
        buf = self._copies.get(stage)
        if buf is None or buf.numel() * 4 < n_bytes:
            buf = self._copies[stage] = torch.empty(n_bytes // 4, dtype=torch.float32, device=self.device)
        self._walk(entry, images, *head, buf, *tail)
        return self._per_image(buf, images[0])

    def add_bounds(self, views: list, Js: list) -> None:
        self._walk('sucre_mosaic_bounds', self._images(views, Js), self._axes_c, self.bounds_words)

    def bounds(self):
        """``(lo_s, lo_t, hi_s, hi_t)`` float32 of what ``add_bounds`` has seen (waits for it), or None when no pixel took part."""
        k = self.bounds_words.cpu().numpy().view(np.uint32)
        if k[0] == 0xffffffff:
            return None
        bits = np.where(k & 0x80000000, k & 0x7fffffff, ~k).astype(np.uint32)   # key_value of csrc/order_key.h
        return tuple(bits.view(np.float32).tolist())

    def begin(self, bounds=None, options: MosaicOptions = None, **fields):
        """Fixes the grid and allocates what ``options`` (a ``MosaicOptions``; ``fields``: fields of the record laid over it, so
        ``begin(blend=H, feather=F)`` is a request too) ask for; checked here (``MosaicOptions.checked``), before anything is
        allocated.  ``blend``: a pixel whose range exceeds its cell's smallest one by d gets the weight ``max(1 - d / H, 0)^2``;
        without it the best view alone.  ``fill`` is checked and not acted on: the hole filling is a call of its own (``fill(R)``; ``run``
        makes it)."""
        options = (options or MosaicOptions()).over(**fields).checked('Mosaic.begin')
        blend, feather, bands, surface, support = options.blend, options.feather, options.bands, options.surface, options.support
        gains, reject = options.gains, options.reject
        if bounds is None:
            bounds = self.bounds()
            if bounds is None:
                raise _mosaic_refusal('grid', 'Mosaic.begin: no pixel takes part (no valid depth with a restored colour), so there are no bounds')
        lo_s, lo_t, hi_s, hi_t = (np.float32(x) for x in bounds)
        if not all(np.isfinite(x) for x in (lo_s, lo_t, hi_s, hi_t)) or hi_s < lo_s or hi_t < lo_t:
            raise _mosaic_refusal('grid', f'Mosaic.begin: bounds {tuple(float(x) for x in (lo_s, lo_t, hi_s, hi_t))} are not finite and ordered')
        Wm, Hm = mosaic_cells(lo_s, hi_s, self.gsd), mosaic_cells(lo_t, hi_t, self.gsd)
        limit = mosaic_max_cells()
        if Wm * Hm > limit or max(Wm, Hm) > 1 << 24:   # before anything is allocated
            raise _mosaic_refusal('grid', f'mosaic of {Wm} x {Hm} cells of {float(self.gsd):.6g} m: more than the {limit} cells allowed '
                                          f'(SUCRE_MOSAIC_MAX_CELLS); give a coarser grid with --mosaic-gsd'
                                          + ('' if support is None else f' (a support of {support} views holds {8 * support} more bytes per cell: '
                                                                        f'the rank words)'))
        if reject is not None:   # before anything is allocated
            need, free = MOSAIC_REJECT_CELL_BYTES * Wm * Hm, _device_free_bytes(self.device)
            if need > MOSAIC_REJECT_MEMORY * free:
                raise _mosaic_refusal('reject', f'mosaic reject: {Wm} x {Hm} cells need {need} bytes for the consensus '
                                                f'({MOSAIC_REJECT_CELL_BYTES} per cell), more than {MOSAIC_REJECT_MEMORY:g} of the {free} free '
                                                f'on the device; give a coarser grid with --mosaic-gsd')
        self._reset(options)
        self.Hm, self.Wm, self.lo, self.hi = Hm, Wm, (lo_s, lo_t), (hi_s, hi_t)
        g = _lib.MosaicGrid()
        g.axes, g.gsd, g.lo_s, g.lo_t, g.Hm, g.Wm = self._axes_c, float(self.gsd), float(lo_s), float(lo_t), Hm, Wm
        self.grid = g
        dev = self.device
        self.key = torch.full((Hm * Wm,), -1, dtype=torch.int64, device=dev)    # all ones: empty
        self.pix = torch.full((Hm * Wm,), -1, dtype=torch.int32, device=dev)
        self._allocate('best')
        if feather is not None:
            self.feather_counts = torch.zeros(2, dtype=torch.int64, device=dev)
        if blend is not None:
            self.inv_h = np.float32(1) / blend
            self.acc = torch.zeros((Hm * Wm, _lib.MOSAIC_ACC_WORDS), dtype=torch.int64, device=dev)
            self._allocate('blend')
        if bands is not None:
            self.band_plan = mosaic_band_plan(blend, feather, bands)
            self.acc_bands = torch.zeros((bands + 1, Hm * Wm, _lib.MOSAIC_ACC_WORDS), dtype=torch.int64, device=dev)
            self._allocate('bands')
        if surface is not None:
            self.top = torch.full((Hm * Wm,), -1, dtype=torch.int32, device=dev)    # all ones: empty
            self.surface_counts = torch.zeros(2, dtype=torch.int64, device=dev)
            self._allocate('surface')
        if support is not None:
            self.rank = torch.full((support, Hm * Wm), -1, dtype=torch.int64, device=dev)    # all ones: empty; 8 M bytes per cell
            self.support_counts = torch.zeros(3, dtype=torch.int64, device=dev)
            self.surface_counts = self.support_counts[::2]   # culled below, samples with a cell: the surface test's two, the same memory
            self._allocate('support')
        if gains is not None:
            self.span = torch.tensor([-1, 0], dtype=torch.int32, device=dev).repeat(Hm * Wm, 1)    # all ones, 0: empty; 8 bytes per cell
            self.acc_gain = torch.zeros((Hm * Wm, _lib.MOSAIC_ACC_WORDS), dtype=torch.int64, device=dev)   # 64 bytes per cell
        if reject is not None:
            slots = _lib.MOSAIC_REJECT_CELL_IMAGES
            self.reject_slot_ord = torch.full((Hm * Wm, slots), -1, dtype=torch.int32, device=dev)    # all ones: free
            self.reject_slot_sum = torch.zeros((Hm * Wm, slots, 4), dtype=torch.int64, device=dev)
            self.reject_slot_over = torch.zeros((Hm * Wm,), dtype=torch.int32, device=dev)
            self._allocate('reject')
            self._reject_state = 'claim'
        return Hm, Wm

    def _begun(self, what: str) -> None:
        if self.grid is None:
            raise ValueError(f'Mosaic.{what}: begin() comes first (it fixes the grid)')

    def _surfaced(self, what: str) -> None:
        self._begun(what)
        if self.surface is None:
            raise ValueError(f'Mosaic.{what}: begin() was not given a surface tolerance, so there is no surface to test against')

    def add_surface(self, views: list, Js: list, first_ordinal: int, plain_atomic: bool = False) -> None:
        """Lowers ``top`` to the highest sample of every cell the images reach.  Over ALL the images, in any batches, after
        ``begin`` and before ``splat``.  ``plain_atomic``: the atomic min for every pixel, without the load that filters them."""
        self._surfaced('add_surface')
        self._walk('sucre_mosaic_surface', self._images(views, Js), int(first_ordinal), C.byref(self.grid), self.top,
                   _lib.MOSAIC_PLAIN_ATOMIC if plain_atomic else 0)

    def _supported(self, what: str) -> None:
        self._surfaced(what)
        if self.support is None:
            raise ValueError(f'Mosaic.{what}: begin() was not given a support, so there are no ranks to fill')

    def add_support(self, views: list, Js: list, first_ordinal: int, level: int, plain_atomic: bool = False) -> None:
        """Lowers level ``level`` of ``rank`` (``sucre_mosaic_support``): the smallest ``order key << 32 | ordinal`` among the
        samples of the images that hold none of the cell's levels below.  Over ALL the images, in any batches, for level 0, then
        for level 1, ..., after ``begin`` and before ``finish_support``.  ``plain_atomic``: as ``add_surface``."""
        self._supported('add_support')
        self._walk('sucre_mosaic_support', self._images(views, Js), int(first_ordinal), C.byref(self.grid), int(self.support), int(level),
                   self.rank, _lib.MOSAIC_PLAIN_ATOMIC if plain_atomic else 0)

    def finish_support(self) -> None:
        """``top``, ``support`` and ``surface_source`` of every cell from its ranks (``sucre_mosaic_support_top``), once
        ``add_support`` has run every level over every image and before ``splat``.  Only enqueues."""
        self._supported('finish_support')
        self._call('sucre_mosaic_support_top', C.byref(self.grid), int(self.support), self.rank, self.top, self._out['support'],
                   self._out['surface_source'])

    def culled_images(self, views: list, Js: list, first_ordinal: int, count: bool = False) -> list:
        """The batch's ``Js`` as the phases after the surface test see them: per image an (H,W,3) float32 copy of ``J`` with NaN in
        every channel of a pixel that does not take part or lies more than T below its cell's top (``sucre_mosaic_cull``).  Valid
        once ``add_surface`` has seen every image.  The images are views into ONE transient buffer, sized to the largest batch
        seen (12 bytes per pixel, every image rounded up to 256 pixels): the next call overwrites them.  ``count``: the culled
        samples are added to ``culled`` and ``surface_counts`` -- to be asked for in one phase alone, so that every sample is
        counted once (``splat`` does).  With a support the cull has two sides (``sucre_mosaic_cull_supported``): a sample more than T
        above its cell's supported top goes too, counted in ``culled_above`` and ``support_counts``.  Only enqueues."""
        self._surfaced('culled_images')
        head = (int(first_ordinal), C.byref(self.grid), self.top, C.c_float(float(self.surface)))
        o = self._out
        if self.support is None:
            tail = (o['culled'], self.surface_counts) if count else (None, None)
            return self._copy('cull', 'sucre_mosaic_cull', self._images(views, Js), head, tail)
        tail = (o['culled'], o['culled_above'], self.support_counts) if count else (None, None, None)
        return self._copy('cull', 'sucre_mosaic_cull_supported', self._images(views, Js), head, tail)

    def _seen(self, views: list, Js: list, first_ordinal: int, upto: str, count: bool = False) -> list:
        """The batch's ``Js`` as a phase sees them: through the stages of the one chain -- 'cull' (with a surface test:
        ``culled_images``), 'reject' (with a colour consensus: its cull of the copy so far), 'gain' (once a gain pass has run: the
        copy so far times the gains) -- up to and including ``upto``, each stage of the copy the stage before it left; a stage
        that was not begun passes its input on.  A stage ``run`` holds (one batch is the whole request) is not made again: the
        same bits.  ``count``: the culling stages add what they take to their counters -- one phase alone asks (``splat``)."""
        stages = (('cull', self.surface is not None, lambda J: self.culled_images(views, J, first_ordinal, count)),
                  ('reject', self.reject is not None, lambda J: self._reject_cull(views, J, first_ordinal, count)),
                  ('gain', self._gain_passes > 0, lambda J: self._apply_gains(views, J, first_ordinal)))
        for stage, begun, make in stages:
            if begun:
                Js = self._held[stage] if stage in self._held else make(Js)
            if stage == upto:
                return Js
        raise ValueError(f'Mosaic: no stage {upto!r}')

    # ---- the colour consensus across views (csrc/reject.h) ----

    def _rejecting(self, what: str) -> None:
        self._begun(what)
        if self.reject is None:
            raise ValueError(f'Mosaic.{what}: begin() was not given a reject tolerance, so there is no consensus to form')

    def add_reject_claim(self, views: list, Js: list, first_ordinal: int, plain_atomic: bool = False) -> None:
        """Lowers ``reject_slot_ord`` to the 8 smallest ordinals of every cell the images reach and sets ``reject_slot_over`` where
        a ninth arrives (``sucre_mosaic_reject_claim``), over the (culled) images.  Over ALL the images, in any batches and any
        order, after ``begin`` (with a surface: after ``add_surface`` / ``finish_support``) and before ``add_reject_sums``.
        ``plain_atomic``: every sample walks the whole chain of atomic minima."""
        self._rejecting('add_reject_claim')
        if self._reject_state != 'claim':
            raise ValueError('Mosaic.add_reject_claim: add_reject_sums() has read the slots already: the claim sees every image first')
        images = self._images(views, self._seen(views, Js, first_ordinal, 'cull'))
        self._walk('sucre_mosaic_reject_claim', images, int(first_ordinal), C.byref(self.grid), self.reject_slot_ord,
                   self.reject_slot_over, _lib.MOSAIC_PLAIN_ATOMIC if plain_atomic else 0)
        self._reject_n = max(self._reject_n, int(first_ordinal) + images[1])

    def add_reject_sums(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """Adds every sample's 1 and quantised colour to its image's slot of its cell (``sucre_mosaic_reject_sums``) where the image
        is one of the cell's eight, over the (culled) images.  Over ALL the images, in any batches and any order, once
        ``add_reject_claim`` has seen every image and before ``finish_reject``.  ``plain``: every sample for itself."""
        self._rejecting('add_reject_sums')
        if self._reject_state == 'done':
            raise ValueError('Mosaic.add_reject_sums: finish_reject() has formed the consensus already')
        images = self._images(views, self._seen(views, Js, first_ordinal, 'cull'))
        if int(first_ordinal) + images[1] > self._reject_n:
            raise ValueError(f'Mosaic.add_reject_sums: ordinals {int(first_ordinal)}..{int(first_ordinal) + images[1] - 1}, but the claim has '
                             f'seen {self._reject_n} images: add_reject_claim() over every image comes first (the slots must be final)')
        self._reject_state = 'sums'
        self._walk('sucre_mosaic_reject_sums', images, int(first_ordinal), C.byref(self.grid), self.reject_slot_ord, self.reject_slot_sum,
                   _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)

    def finish_reject(self) -> None:
        """The consensus of every cell from its slots (``sucre_mosaic_reject_consensus``): ``reject_ref``, ``reject_source`` and
        ``reject_views``; ``reject_overflow`` from the flags.  Once ``add_reject_sums`` has seen every image and before ``splat``.
        Waits, and raises ValueError (``field``: 'reject') when an image holds ``MOSAIC_MAX_SAMPLES`` = 2^20 samples or more in
        one cell (the integer comparison of two means may overflow).  Frees the slots (292 bytes per cell); ``reject_counts``
        ((n, 16) int64, two words used) is allocated for the n images the claim has seen."""
        self._rejecting('finish_reject')
        if self._reject_state != 'sums':
            raise ValueError('Mosaic.finish_reject: add_reject_claim() and then add_reject_sums() over every image come first'
                             if self._reject_state == 'claim' else 'Mosaic.finish_reject: the consensus has been formed already')
        o = self._out
        big = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._call('sucre_mosaic_reject_consensus', C.byref(self.grid), self.reject_slot_ord, self.reject_slot_sum, o['reject_ref'],
                   o['reject_source'], o['reject_views'], big)
        n_big = int(big)
        if n_big:
            raise _mosaic_refusal('reject', f'mosaic reject: {n_big} times an image holds {MOSAIC_MAX_SAMPLES} samples or more in one cell, and '
                                            f'from there on the comparison of two images\' means may overflow; give a finer grid with --mosaic-gsd')
        o['reject_overflow'].copy_((self.reject_slot_over != 0).view(self.Hm, self.Wm))
        self.reject_slot_ord = self.reject_slot_sum = self.reject_slot_over = None
        self.reject_counts = torch.zeros((self._reject_n, _lib.MOSAIC_GAIN_ROW_WORDS), dtype=torch.int64, device=self.device)
        self._reject_state = 'done'

    def rejected_images(self, views: list, Js: list, first_ordinal: int, count: bool = False) -> list:
        """The batch's ``Js`` as the phases after the colour consensus see them: per image an (H,W,3) float32 copy of the (culled)
        ``J`` with NaN in every channel of a pixel that does not take part, or whose cell has a reference, whose image is not the
        cell's ``reject_source`` and whose colour differs from ``reject_ref`` by more than T in any channel
        (``sucre_mosaic_reject_cull``).  Valid once ``finish_reject`` has run.  Views into ONE transient buffer of its own, sized to
        the largest batch seen: the next call overwrites them.  ``count``: the rejected samples are added to ``rejected`` and
        ``reject_counts`` -- to be asked for in one phase alone (``splat`` does).  Only enqueues."""
        return self._reject_cull(views, self._seen(views, Js, first_ordinal, 'cull'), first_ordinal, count)

    def _reject_cull(self, views: list, Jc: list, first_ordinal: int, count: bool = False) -> list:
        """``rejected_images`` of the culled ``Jc``: the chain's stage 'reject'."""
        self._rejecting('rejected_images')
        if self._reject_state != 'done':
            raise ValueError('Mosaic.rejected_images: finish_reject() comes first (there is no consensus to test against yet)')
        images = self._images(views, Jc)
        n = images[1]
        if int(first_ordinal) + n > self._reject_n:
            raise ValueError(f'Mosaic.rejected_images: ordinals {int(first_ordinal)}..{int(first_ordinal) + n - 1}, but the claim has seen '
                             f'{self._reject_n} images')
        o = self._out
        return self._copy('reject', 'sucre_mosaic_reject_cull', images,
                          (int(first_ordinal), C.byref(self.grid), o['reject_ref'], o['reject_source'], C.c_float(float(self.reject))),
                          (o['rejected'] if count else None, int(self._reject_n), self.reject_counts if count else None))

    # ---- the gain compensation (csrc/gains_mosaic.h) ----

    def _gaining(self, what: str) -> None:
        self._begun(what)
        if self.gains is None:
            raise ValueError(f'Mosaic.{what}: begin() was not given gain rounds, so there are no gains to find')

    def _spanned(self, what: str) -> None:
        self._gaining(what)
        if self._splatted is False:
            raise ValueError(f'Mosaic.{what}: splat() comes first (the reference pass reads every cell\'s smallest range)')

    def add_span(self, views: list, Js: list, first_ordinal: int, plain_atomic: bool = False) -> None:
        """Lowers and raises ``span`` to the smallest and the largest ordinal of the samples of every cell the images reach
        (``sucre_mosaic_gain_span``).  Over ALL the images, in any batches, once ``splat`` has seen every image and before the first
        gain pass.  ``plain_atomic``: both atomics for every pixel, without the loads that filter them."""
        self._spanned('add_span')
        self._walk('sucre_mosaic_gain_span', self._images(views, self._seen(views, Js, first_ordinal, 'reject')), int(first_ordinal),
                   C.byref(self.grid), self.span, _lib.MOSAIC_PLAIN_ATOMIC if plain_atomic else 0)

    def _apply_gains(self, views: list, Jc: list, first_ordinal: int) -> list:
        """``Jc`` times the gains of their ordinals (``sucre_mosaic_gain_apply``), the chain's stage 'gain': views into the ONE
        transient buffer of that stage, sized to the largest batch seen: the next call overwrites them."""
        images = self._images(views, Jc)
        n, table = images[1], self.gain_table
        if int(first_ordinal) + n > table.shape[0]:
            raise ValueError(f'Mosaic: ordinals {int(first_ordinal)}..{int(first_ordinal) + n - 1} but the gain table holds '
                             f'{table.shape[0]} images (begin_gain_pass fixes the count)')
        return self._copy('gain', 'sucre_mosaic_gain_apply', images, (int(first_ordinal), table, int(table.shape[0])))

    def gained_images(self, views: list, Js: list, first_ordinal: int) -> list:
        """The batch's ``Js`` as the phases after the gain compensation see them: per image the (H,W,3) float32 culled and rejected
        ``J`` (``J`` itself without a surface test and a consensus) times the image's gain, one float32 multiply per channel; a
        NaN stays a NaN.  Valid once a gain pass has begun (the gain table exists then).  Views into one transient buffer; only
        enqueues."""
        self._gaining('gained_images')
        if self.gain_table is None:
            raise ValueError('Mosaic.gained_images: no gain pass has begun, so there is no gain table yet')
        return self._apply_gains(views, self._seen(views, Js, first_ordinal, 'reject'), first_ordinal)

    def begin_gain_pass(self, n_images: int) -> None:
        """Opens a pass at the gains as they stand: zeroes ``acc_gain``; the first one allocates ``gain_table`` (ones) and
        ``gain_sums_words`` for ``n_images``, the images of the whole request."""
        self._spanned('begin_gain_pass')
        if self._gain_passes > self.gains:
            raise ValueError(f'Mosaic.begin_gain_pass: the {self.gains} rounds and the measuring pass have run')
        if self.gain_table is None:
            n = int(n_images)
            if not 1 <= n <= MAX_VIEWS:
                raise ValueError(f'Mosaic.begin_gain_pass: {n} images, need 1..{MAX_VIEWS}')
            self.gain_table = torch.ones((n, 3), dtype=torch.float32, device=self.device)
            self.gain_sums_words = torch.zeros((self.gains + 1, n, _lib.MOSAIC_GAIN_ROW_WORDS), dtype=torch.int64, device=self.device)
        elif int(n_images) != self.gain_table.shape[0]:
            raise ValueError(f'Mosaic.begin_gain_pass: {int(n_images)} images, but the first pass saw {self.gain_table.shape[0]}')
        self.acc_gain.zero_()
        self._gain_open = True

    def _in_gain_pass(self, what: str) -> None:
        self._gaining(what)
        if not self._gain_open:
            raise ValueError(f'Mosaic.{what}: begin_gain_pass() comes first')

    def add_gain_reference(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """The reference of the open pass: the blend's accumulate over the gained images into ``acc_gain`` with the smallest normal
        float32 as ``inv_h``, so that every sample weighs 4096 -- the per-sample mean.  Over ALL the images before ``add_gain_sums``."""
        self._in_gain_pass('add_gain_reference')
        Jg = self._apply_gains(views, self._seen(views, Js, first_ordinal, 'reject'), first_ordinal)
        self._walk('sucre_mosaic_accumulate', self._images(views, Jg), int(first_ordinal), C.byref(self.grid), self.key,
                   C.c_float(2.0 ** -126), self.acc_gain, _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)

    def check_gain_reference(self) -> None:
        """Waits for the reference and raises ValueError (``field``: 'gains') when a cell holds ``MOSAIC_MAX_SAMPLES`` = 2^20 samples
        or more (its 64-bit sums may have wrapped).  ``gain_pass`` calls it in the first pass: the counts do not change after it."""
        self._gaining('check_gain_reference')
        most = int(self.acc_gain[:, 7].max())
        if most >= MOSAIC_MAX_SAMPLES:
            raise _mosaic_refusal('gains', f'mosaic gains: a cell holds {most} samples, and from {MOSAIC_MAX_SAMPLES} on its 64-bit sums '
                                           f'may overflow; give a finer grid with --mosaic-gsd')

    def add_gain_sums(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """The ten sums per image of the open pass (``sucre_mosaic_gain_sums``) over the un-gained (culled) images, once
        ``add_gain_reference`` has seen every image.  An image of more than ``MOSAIC_GAIN_MAX_PIXELS`` pixels is refused before any
        launch.  ``plain``: one set of atomics per 256 pixels (the same words)."""
        self._in_gain_pass('add_gain_sums')
        for v in views:
            H, W = v.depth.shape
            if H * W > MOSAIC_GAIN_MAX_PIXELS:
                raise _mosaic_refusal('gains', f'mosaic gains: {v.name or "a view"} has {W} x {H} pixels, more than the '
                                               f'{MOSAIC_GAIN_MAX_PIXELS} whose 64-bit sums stay below 2^62')
        images = self._images(views, self._seen(views, Js, first_ordinal, 'reject'))
        if int(first_ordinal) + images[1] > self.gain_table.shape[0]:
            raise ValueError(f'Mosaic.add_gain_sums: ordinals {int(first_ordinal)}..{int(first_ordinal) + images[1] - 1} but the gain '
                             f'table holds {self.gain_table.shape[0]} images')
        self._walk('sucre_mosaic_gain_sums', images, int(first_ordinal), C.byref(self.grid), self.span, self.acc_gain, self.gain_table,
                   int(self.gain_table.shape[0]), self.gain_sums_words[self._gain_passes], _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)

    def end_gain_pass(self) -> None:
        """Closes the open pass: its sums are row ``passes so far`` of ``gain_sums``."""
        self._in_gain_pass('end_gain_pass')
        self._gain_open = False
        self._gain_passes += 1

    def gain_pass(self, batches, plain: bool = False) -> None:
        """One whole pass at the gains as they stand over ``batches`` (as ``run`` takes them): ``begin_gain_pass``, the reference
        over every batch, in the first pass ``check_gain_reference``, the sums over every batch, ``end_gain_pass``."""
        batches = list(batches)
        self._spanned('gain_pass')
        if self.gain_table is None:   # the first pass learns the images of the request
            self.begin_gain_pass(max(first + len(load()[0]) for first, load in batches))
        else:
            self.begin_gain_pass(self.gain_table.shape[0])
        for first, load in batches:
            self.add_gain_reference(*load(), first, plain=plain)
        if self._gain_passes == 0:
            self.check_gain_reference()
        for first, load in batches:
            self.add_gain_sums(*load(), first, plain=plain)
        self.end_gain_pass()

    def gain_sums(self) -> torch.Tensor:
        """(passes so far, n, 10) int64 on the device: the sums of every closed pass."""
        self._gaining('gain_sums')
        if self.gain_sums_words is None:
            raise ValueError('Mosaic.gain_sums: no gain pass has begun')
        return self.gain_sums_words[:self._gain_passes, :, :_lib.MOSAIC_GAIN_WORDS].contiguous()

    def solve_gains(self) -> torch.Tensor:
        """The gains of the next pass from the sums of the last closed one (``mosaic_gain_solve``, on the host: waits); returns the
        (n,3) float32 device table."""
        self._gaining('solve_gains')
        if self._gain_passes == 0 or self._gain_open:
            raise ValueError('Mosaic.solve_gains: a whole gain pass comes first (gain_pass, or begin_gain_pass .. end_gain_pass)')
        sums = self.gain_sums_words[self._gain_passes - 1, :, :_lib.MOSAIC_GAIN_WORDS].cpu().numpy()
        solved = mosaic_gain_solve(sums, self.gain_table.cpu().numpy(), self.gain_limit)
        self.gain_table.copy_(torch.from_numpy(solved))
        return self.gain_table

    # ---- the direct solve (csrc/gains_direct.h) ----

    def _direct(self, what: str) -> None:
        self._gaining(what)
        if self.gain_solve != 'direct':
            raise ValueError(f"Mosaic.{what}: begin() was not given gain_solve='direct'")
        if self._gain_passes == 0 or self._gain_open:
            raise ValueError(f'Mosaic.{what}: a whole gain pass comes first (it fixes the images of the request and checks the cells)')

    def _begin_direct(self) -> None:
        """Allocates the direct solve's state, or refuses (``field``: 'gain_solve') what does not fit into
        ``MOSAIC_GAIN_DIRECT_MEMORY`` of the free device memory (``_device_free_bytes``), before any of it is allocated."""
        n, cells = int(self.gain_table.shape[0]), self.Hm * self.Wm
        need = MOSAIC_GAIN_DIRECT_CELL_BYTES * cells + 32 * n * n + 8 * _lib.MOSAIC_GAIN_ROW_WORDS * n
        free = _device_free_bytes(self.device)
        if need > MOSAIC_GAIN_DIRECT_MEMORY * free:
            raise _mosaic_refusal('gain_solve', f'mosaic gain solve direct: {self.Wm} x {self.Hm} cells and {n} images need {need} bytes '
                                                f'({MOSAIC_GAIN_DIRECT_CELL_BYTES} per cell, 32 per pair of images), more than '
                                                f'{MOSAIC_GAIN_DIRECT_MEMORY:g} of the {free} free on the device; give a coarser grid with '
                                                f'--mosaic-gsd, fewer than {n} images, or leave the solve to the rounds')
        dev = self.device
        self.slot_ord = torch.full((cells, _lib.MOSAIC_GAIN_CELL_IMAGES), -1, dtype=torch.int32, device=dev)    # all ones: free
        self.slot_sum = torch.zeros((cells, _lib.MOSAIC_GAIN_CELL_IMAGES, 4), dtype=torch.int64, device=dev)
        self.slot_over = torch.zeros((cells,), dtype=torch.int32, device=dev)
        self.gain_pairs_words = torch.zeros((n, n, 4), dtype=torch.int64, device=dev)
        self.gain_diag_words = torch.zeros((n, _lib.MOSAIC_GAIN_ROW_WORDS), dtype=torch.int64, device=dev)

    def _direct_images(self, what: str, views: list, Js: list, first_ordinal: int):
        images = self._images(views, self._seen(views, Js, first_ordinal, 'reject'))
        if int(first_ordinal) + images[1] > self.gain_table.shape[0]:
            raise ValueError(f'Mosaic.{what}: ordinals {int(first_ordinal)}..{int(first_ordinal) + images[1] - 1} but the gain '
                             f'table holds {self.gain_table.shape[0]} images')
        return images

    def add_gain_slots(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """Per shared cell, the count and the colour sums of every image that reaches it (``sucre_mosaic_gain_slots``), over the
        un-gained (culled) images.  Over ALL the images, in any batches, after the first gain pass and before ``gain_pairs``.
        ``plain``: every sample for itself (the same words)."""
        self._direct('add_gain_slots')
        if self._paired:
            raise ValueError('Mosaic.add_gain_slots: gain_pairs() has read the slots already')
        images = self._direct_images('add_gain_slots', views, Js, first_ordinal)
        if self.slot_ord is None:
            self._begin_direct()
        self._walk('sucre_mosaic_gain_slots', images, int(first_ordinal), C.byref(self.grid), self.span, self.slot_ord, self.slot_sum,
                   self.slot_over, _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)

    def _slotted(self, what: str) -> None:
        self._direct(what)
        if self.slot_ord is None:
            raise ValueError(f'Mosaic.{what}: add_gain_slots() over every image comes first')

    def gain_pairs(self, plain: bool = False, table_entries: int = 0) -> None:
        """The pair sums of every shared cell that did not overflow (``sucre_mosaic_gain_pairs``), once, when ``add_gain_slots`` has
        seen every image.  ``plain``: global atomics per cell and pair; ``table_entries``: the size of a workgroup's table, a
        power of two up to ``_lib.MOSAIC_GAIN_PAIR_TABLE``, 0 for that (the same words either way)."""
        self._slotted('gain_pairs')
        if self._paired:
            raise ValueError('Mosaic.gain_pairs: the pairs have been added already')
        self._call('sucre_mosaic_gain_pairs', C.byref(self.grid), self.span, self.slot_ord, self.slot_sum, self.slot_over,
                   int(self.gain_table.shape[0]), self.gain_pairs_words, int(table_entries), _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)
        self._paired = True

    def add_gain_diag(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """Per image the count and ``sum Xq Xq`` of its samples in shared cells that did not overflow (``sucre_mosaic_gain_diag``),
        over the un-gained (culled) images, once ``add_gain_slots`` has seen every image.  ``plain``: one set of atomics per 256 pixels."""
        self._slotted('add_gain_diag')
        images = self._direct_images('add_gain_diag', views, Js, first_ordinal)
        self._walk('sucre_mosaic_gain_diag', images, int(first_ordinal), C.byref(self.grid), self.span, self.slot_over,
                   int(self.gain_table.shape[0]), self.gain_diag_words, _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)

    def gain_diag(self) -> torch.Tensor:
        """(n, 4) int64 on the device: per image n_i and ``sum Xq Xq`` x 3."""
        self._slotted('gain_diag')
        return self.gain_diag_words[:, :4].contiguous()

    def solve_gains_direct(self) -> torch.Tensor:
        """The gains of the next pass from the pairs and the diag (``mosaic_gain_solve_direct``, on the host: waits), in place of
        ``solve_gains`` after the first pass; returns the (n,3) float32 device table.  ``gain_kept``: the channels that kept
        their gains."""
        self._slotted('solve_gains_direct')
        if not self._paired:
            raise ValueError('Mosaic.solve_gains_direct: gain_pairs() and add_gain_diag() over every image come first')
        solved, kept = mosaic_gain_solve_direct(self.gain_pairs_words.cpu().numpy(), self.gain_diag().cpu().numpy(),
                                                self.gain_table.cpu().numpy(), self.gain_limit)
        self.gain_table.copy_(torch.from_numpy(solved))
        self.gain_direct, self.gain_kept = self.gain_table.clone(), kept
        return self.gain_table

    def splat(self, views: list, Js: list, first_ordinal: int, plain_atomic: bool = False) -> None:
        self._begun('splat')
        self._splatted = True
        seen = self._seen(views, Js, first_ordinal, 'gain', count=self._gain_passes == 0)   # the one phase that counts what is culled
        self._walk('sucre_mosaic_splat', self._images(views, seen), int(first_ordinal), C.byref(self.grid), self.key,
                   _lib.MOSAIC_PLAIN_ATOMIC if plain_atomic else 0)

    def resolve(self, views: list, Js: list, first_ordinal: int) -> None:
        self._begun('resolve')
        self._walk('sucre_mosaic_resolve', self._images(views, self._seen(views, Js, first_ordinal, 'gain')), int(first_ordinal),
                   C.byref(self.grid), self.key, self.pix)

    def gather(self, views: list, Js: list, first_ordinal: int) -> None:
        self._begun('gather')
        self._walk('sucre_mosaic_gather', self._images(views, self._seen(views, Js, first_ordinal, 'gain')), int(first_ordinal),
                   C.byref(self.grid), self.key, self.pix, *(self._out[k] for k in ('J', 'raw', 'source', 'pixel', 'range')))

    def _blending(self, what: str) -> None:
        self._begun(what)
        if self.blend is None:
            raise ValueError(f'Mosaic.{what}: begin() was not given a blend depth, so there is nothing to blend into')

    def accumulate(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """Adds the images' weighted samples to ``acc``.  Valid once ``splat`` has seen every image (``key`` holds every cell's
        smallest range then).  ``plain``: eight atomics per pixel instead of eight per run of a wave's lanes (the same ``acc``).
        With a feather the batch's map is formed first (``sucre_mosaic_feather``) and the feathered phase reads it."""
        self._blending('accumulate')
        images = self._images(views, self._seen(views, Js, first_ordinal, 'gain'))
        head = (int(first_ordinal), C.byref(self.grid), self.key, C.c_float(float(self.inv_h)))
        tail = (self.acc, _lib.MOSAIC_PLAIN_ATOMIC if plain else 0)
        if self.feather is None:
            return self._walk('sucre_mosaic_accumulate', images, *head, *tail)
        self._feather_buf, words = self._feather_pass(images, self.feather, self._feather_buf)
        with torch.cuda.device(self.device):
            if len({tuple(d2.shape) for d2 in words}) == 1:   # one size: the maps as one strided tensor, two reductions
                H, W = words[0].shape
                pitch = -(-(H * W) // _lib.MOSAIC_BLOCK_PX) * _lib.MOSAIC_BLOCK_PX
                words = [torch.as_strided(words[0], (len(words), H * W), (pitch, 1))]
            for d2 in words:
                self.feather_counts += torch.stack([((d2 > 0) & (d2 < self.feather ** 2)).sum(), (d2 > 0).sum()])
        self._walk('sucre_mosaic_accumulate_feathered', images, *head, self.feather, self._feather_buf, *tail)

    def _feather_pass(self, images, F: int, buf=None):
        """Enqueues ``sucre_mosaic_feather`` over ``images`` (as ``_images`` returns them) into ``buf`` (a new buffer when None or
        too small) and returns the buffer and, per image, the (H,W) int32 view of its ``dist2`` words in it."""
        arr, n, table, _ = images
        lib = _lib.load()
        n_bytes = lib.sucre_mosaic_feather_bytes(n, arr)
        if n_bytes == 0:
            raise _lib.SucreError(f'sucre_mosaic_feather_bytes: {lib.sucre_last_error().decode()}')
        if buf is None or buf.numel() < n_bytes:
            buf = torch.empty(n_bytes, dtype=torch.uint8, device=self.device)    # (4-byte aligned: the allocator's blocks are)
        self._walk('sucre_mosaic_feather', images, int(F), buf)
        words = buf[:n_bytes // 6 * 4].view(torch.int32)   # the dist2 words; the uint16 scratch sits behind them
        return buf, self._per_image(words, arr, 1)

    def feather_map(self, views: list, Js: list, F) -> list:
        """Per image the (H,W) int32 ``dist2`` of csrc/mosaic.h, "The feather": ``min(D2, F^2)`` with D2 the squared distance in
        pixels from a pixel that takes part to the nearest one that does not or lies outside the image; 0 for a pixel that does
        not take part.  Needs no ``begin``; only enqueues (reading a map waits for it)."""
        F = mosaic_feather_px(F)
        _, maps = self._feather_pass(self._images(views, Js), F)
        return [m.clone() for m in maps]

    def _band_buffers(self, images, bufs=None):
        """Three float32 buffers of one band each for ``images`` (``sucre_mosaic_band_bytes``; ``bufs`` when they are large enough)
        and, per image, the index of its first pixel in them."""
        n_bytes = self._band_bytes(images)
        if bufs is None or bufs[0].numel() * 4 < n_bytes:
            bufs = [torch.empty(n_bytes // 4, dtype=torch.float32, device=self.device) for _ in range(3)]
        return bufs, self._offsets(images[0])

    def _band_levels(self, images, K: int, bufs):
        """Enqueues the K levels of ``sucre_mosaic_band_split`` over ``images``, S ping-ponging between ``bufs[0]`` and ``bufs[1]``,
        and yields after each ``(j, buffer)``: the detail band D_j in ``bufs[2]`` for j < K, then ``(K, the buffer of S_K)``.  A
        yielded buffer is overwritten by the next level: the caller enqueues what reads it before it goes on."""
        S, D = bufs[:2], bufs[2]
        for level in range(K):
            self._walk('sucre_mosaic_band_split', images, level, None if level == 0 else S[(level - 1) % 2], S[level % 2], D)
            yield level, D
        yield K, S[(K - 1) % 2]

    def band_stack(self, views: list, Js: list, K) -> list:
        """Per image the K + 1 (H,W,3) float32 tensors ``D_0 .. D_(K-1), S_K`` of csrc/bands.h: the detail bands of an a-trous
        ``[1, 2, 1]`` filter normalised over the pixels that take part, finest first, and the residual; NaN at a pixel that does not
        take part.  Needs no ``begin``; only enqueues (reading a band waits for it)."""
        K = mosaic_band_count(K)
        images = self._images(views, Js)
        bufs, _ = self._band_buffers(images)
        stacks = [[] for _ in images[0]]
        for _, buf in self._band_levels(images, K, bufs):
            for stack, band in zip(stacks, self._per_image(buf, images[0])):
                stack.append(band.clone())
        return stacks

    def _banding(self, what: str) -> None:
        self._blending(what)
        if self.bands is None:
            raise ValueError(f'Mosaic.{what}: begin() was not given a band count, so there are no bands to blend')

    def _accumulate_band(self, images, first, j: int, buf, first_ordinal: int, flags: int, feather_buf) -> None:
        """Band ``j`` of ``images`` -- in ``buf``, image i's block at pixel ``first[i]`` -- into slice ``j`` of ``acc_bands``: the
        accumulate entry with the band as the images' J and ``band_plan[j]``; ``feather_buf``: a map of these images made at
        ``F_j`` or wider (not read without a feather)."""
        arr, n, table, keep = images
        band = (_lib.MosaicImage * n)()
        C.memmove(band, arr, C.sizeof(band))
        for e, at in zip(band, first):
            e.J = buf.data_ptr() + at * 12
        H_j, F_j = self.band_plan[j]
        head = (int(first_ordinal), C.byref(self.grid), self.key, C.c_float(float(np.float32(1) / H_j)))
        if F_j is None:
            return self._walk('sucre_mosaic_accumulate', (band, n, table, keep), *head, self.acc_bands[j], flags)
        self._walk('sucre_mosaic_accumulate_feathered', (band, n, table, keep), *head, F_j, feather_buf, self.acc_bands[j], flags)

    def accumulate_bands(self, views: list, Js: list, first_ordinal: int, plain: bool = False) -> None:
        """Splits the images into their band stacks and adds every band's weighted samples to its slice of ``acc_bands``: the
        blend's accumulate entry (the feathered one with a feather) with the band as the images' J and the band's
        ``(H_j, F_j)`` of ``band_plan``.  Valid once ``splat`` has seen every image.  With a feather the batch's map is formed once,
        at the user's F and from the true J, and every band reads it: ``dist2 = min(D2, F^2)`` tells ``dist2 >= F_j^2`` and holds
        every root below it for any ``F_j <= F``.  ``plain``: as ``accumulate``.  ``acc`` and ``feather_counts`` are not touched."""
        self._banding('accumulate_bands')
        images = self._images(views, self._seen(views, Js, first_ordinal, 'gain'))
        self._band_bufs, first = self._band_buffers(images, self._band_bufs)
        if self.feather is not None:
            self._feather_buf, _ = self._feather_pass(images, self.feather, self._feather_buf)
        flags = _lib.MOSAIC_PLAIN_ATOMIC if plain else 0
        for j, buf in self._band_levels(images, self.bands, self._band_bufs):
            self._accumulate_band(images, first, j, buf, first_ordinal, flags, self._feather_buf)

    def combine_bands(self) -> None:
        """The per-cell pass from ``acc_bands`` to ``J_multiband``: every band's quotient as ``normalize`` forms the blend's, added
        in float32 from the residual to the finest band.  Valid once ``accumulate_bands`` has seen every image (``normalize`` has
        checked the sample bound: the residual's counts are the blend's); only enqueues."""
        self._banding('combine_bands')
        self._call('sucre_mosaic_band_combine', C.byref(self.grid), self.bands + 1, self.acc_bands, self._out['J_multiband'])

    def normalize(self, check: bool = True) -> None:
        """The per-cell pass from ``acc`` to the four blended outputs; waits for it, and raises ValueError when a cell holds
        ``MOSAIC_MAX_SAMPLES`` = 2^20 samples or more (its 64-bit sums may have wrapped).  ``check=False`` only enqueues the
        pass (for measurements: the caller looks at ``samples`` itself)."""
        self._blending('normalize')
        o = self._out
        self._call('sucre_mosaic_normalize', C.byref(self.grid), self.acc, o['J_blend'], o['raw_blend'], o['weight'], o['samples'])
        if not check:
            return
        most = int(o['samples'].max())
        if most >= MOSAIC_MAX_SAMPLES:
            raise _mosaic_refusal('blend', f'mosaic blend: a cell holds {most} samples, and from {MOSAIC_MAX_SAMPLES} on its 64-bit sums '
                                           f'may overflow; give a finer grid with --mosaic-gsd')

    def fill(self, R) -> int:
        """Closes the holes up to ``R`` metres across (``MOSAIC_FILL_RANGE``; ValueError before anything is allocated) and returns
        L, the levels used (``mosaic_fill_levels``).  Valid once ``gather`` has seen every image and, with a blend, ``normalize``
        has run.  ``J_filled`` / ``raw_filled`` are ``J`` / ``raw`` with every cell without a source (``source < 0``) replaced by
        the pyramid's value where one reaches it (``fill_level``: 0 measured, 1..L the coarsest level a filled cell drew on, -1
        still empty; NaN and 0 there); with a blend ``J_blend_filled`` / ``raw_blend_filled`` come from ``J_blend`` / ``raw_blend``
        and the same ``source`` through the same pyramid buffer, with bands ``J_multiband_filled`` from ``J_multiband`` and
        ``raw_blend`` likewise (that pass's raw picture is dropped: there is no multi-band raw mosaic).  Only enqueues.  Like the other phases it cannot tell whether
        the phases before it have seen every image: called earlier on a begun mosaic it fills from the grid as it stands then
        (from an empty grid: nothing, every cell -1)."""
        self._begun('fill')
        R = mosaic_fill_reach(R)   # (not through a MosaicOptions: there None is "no fill", here it is a value to refuse)
        L = mosaic_fill_levels(R, self.gsd, self.Hm, self.Wm)
        lib, dev, Hm, Wm = _lib.load(), self.device, self.Hm, self.Wm
        n_bytes = lib.sucre_mosaic_fill_bytes(Hm, Wm, L)
        if n_bytes == 0:
            raise _lib.SucreError(f'sucre_mosaic_fill_bytes: {lib.sucre_last_error().decode()}')
        self.fill_reach, self.fill_levels = R, L
        self.pyramid = torch.empty(n_bytes, dtype=torch.uint8, device=dev)    # (256-byte aligned: the allocator's blocks are)
        pairs = [('fill', 'J', 'raw', 'J_filled', 'raw_filled')]
        if self.blend is not None:
            pairs.append(('blend_fill', 'J_blend', 'raw_blend', 'J_blend_filled', 'raw_blend_filled'))
        if self.bands is not None:
            pairs.append(('bands_fill', 'J_multiband', 'raw_blend', 'J_multiband_filled', None))
        o = self._out
        for group, J, raw, J_to, raw_to in pairs:
            with torch.cuda.device(dev):
                self._allocate(group)
                # (the blend's own levels are not a result: a blended colour is always finite, a best-view one need not be)
                level = o['fill_level'] if group == 'fill' else torch.empty_like(o['fill_level'])
                raw_filled = torch.empty_like(o[raw]) if raw_to is None else o[raw_to]
            base = (Hm, Wm, L, o[J], o[raw], o['source'], self.pyramid)
            self._call('sucre_mosaic_fill_pull', *base)
            self._call('sucre_mosaic_fill_push', *base, o[J_to], raw_filled, level)
        return L

    def result(self) -> dict:
        """``J`` (Hm,Wm,3) float32 (NaN: empty), ``raw`` (Hm,Wm,3) uint8 (0), ``source`` and ``pixel`` (Hm,Wm) int32 (-1), ``range``
        (Hm,Wm) float32 (NaN), on the device, complete once ``gather`` has seen every image.  With a blend also ``J_blend``
        (Hm,Wm,3) float32 (NaN), ``raw_blend`` (Hm,Wm,3) uint8 (0), ``weight`` (Hm,Wm) float32 -- the sum of the samples' weights,
        each at most 1 -- (0) and ``samples`` (Hm,Wm) int32 (0), complete once ``normalize`` has run.  After ``fill`` also
        ``J_filled`` (Hm,Wm,3) float32 (NaN: still empty), ``raw_filled`` (Hm,Wm,3) uint8 (0), ``fill_level`` (Hm,Wm) int32 (-1)
        and, with a blend, ``J_blend_filled`` and ``raw_blend_filled``.  With a feather also ``feather``, the width F (an int).  With
        bands also ``J_multiband`` (Hm,Wm,3) float32 (NaN), complete once ``combine_bands`` has run, and ``bands``, the count K (an
        int); after ``fill`` also ``J_multiband_filled``.  With a surface test also ``surface`` (Hm,Wm) float32 (NaN) -- the value of
        ``top`` as it stands, complete once ``add_surface`` has seen every image --, ``culled`` (Hm,Wm) int32 (0), complete once
        ``splat`` has, and ``surface_tol``, the tolerance T (a float, the float32 value).  With a support ``surface`` is the
        supported top, complete once ``finish_support`` has run, and the result also holds ``support`` (Hm,Wm) int32 (0),
        ``surface_source`` (Hm,Wm) int32 (-1), ``culled_above`` (Hm,Wm) int32 (0), ``surface_top`` (Hm,Wm) float32 (NaN) -- the plain
        minimum, the value of level 0 of ``rank`` -- and ``surface_support``, the count M (an int).  With a gain compensation also, after
        every other key, ``gains`` (n,3) float32, ``gain_sums`` (passes, n, 10) int64, ``gain_rms`` (passes, 3) float64 (CPU),
        ``gain_overlap`` (n,) int64, ``gain_rounds`` (= R, an int) and ``gain_limit`` (= L, a float)."""
        self._begun('result')
        def heights(k):   # key_value of csrc/order_key.h, per cell; all ones: NaN
            bits = torch.where(k < 0, k & 0x7fffffff, ~k).view(torch.float32)
            return torch.where(k == -1, torch.full_like(bits, _NAN), bits).view(self.Hm, self.Wm)
        if self.surface is not None:
            self._out['surface'].copy_(heights(self.top))
        if self.support is not None:
            self._out['surface_top'].copy_(heights((self.rank[0] >> 32).to(torch.int32)))
        of = self._outputs   # the groups in result()'s own order, which is not the order of the table's rows
        return {**of('best', 'blend', 'bands', 'surface'), **({} if self.feather is None else {'feather': self.feather}),
                **({} if self.bands is None else {'bands': self.bands}),
                **({} if self.surface is None else {'surface_tol': float(self.surface)}),
                **({} if self.support is None else {**of('support'), 'surface_support': int(self.support)}),
                **self._reject_result(), **of('fill', 'blend_fill', 'bands_fill'), **self._gain_result()}

    def _outputs(self, *groups) -> dict:
        """The allocated outputs of ``groups`` (``MOSAIC_OUTPUTS``), in the order they were allocated."""
        return {key: t for key, t in self._out.items() if MOSAIC_OUTPUTS[key][0] in groups}

    def _reject_result(self) -> dict:
        """The keys of ``result()`` that a colour consensus adds (none without one): the rows of ``MOSAIC_REJECT_OUTPUTS``,
        ``reject_per_image`` (n,2) int64 -- per image the samples in cells that have a reference and the samples rejected; no row
        before ``finish_reject`` -- and ``reject_tol`` (= T, a float, the float32 value)."""
        if self.reject is None:
            return {}
        per = torch.zeros((0, 2), dtype=torch.int64, device=self.device) if self.reject_counts is None else self.reject_counts[:, :2].contiguous()
        return {**self._outputs('reject'), 'reject_per_image': per, 'reject_tol': float(self.reject)}

    def _gain_result(self) -> dict:
        """The keys of ``result()`` that a gain compensation adds (none without one); waits for the sums."""
        if self.gains is None:
            return {}
        n = 0 if self.gain_table is None else self.gain_table.shape[0]
        sums = torch.zeros((0, n, _lib.MOSAIC_GAIN_WORDS), dtype=torch.int64, device=self.device) if n == 0 else self.gain_sums()
        host = sums.cpu().numpy()
        rms = torch.tensor([mosaic_gain_rms(p) for p in host], dtype=torch.float64).reshape(len(host), 3)
        overlap = sums[-1, :, 0].clone() if len(host) else torch.zeros(n, dtype=torch.int64, device=self.device)
        gains = torch.ones((0, 3), dtype=torch.float32, device=self.device) if n == 0 else self.gain_table.clone()
        return {'gains': gains, 'gain_sums': sums, 'gain_rms': rms, 'gain_overlap': overlap, 'gain_rounds': int(self.gains),
                'gain_limit': float(self.gain_limit), **self._gain_direct_result()}

    def _gain_direct_result(self) -> dict:
        """The keys of ``result()`` that a direct solve adds (none before ``solve_gains_direct``); waits."""
        if self.gain_direct is None:
            return {}
        pairs, diag = self.gain_pairs_words.cpu(), self.gain_diag().cpu()
        index = (pairs[:, :, 3] > 0).nonzero()      # ascending (i, j); only the upper triangle is written
        span = self.span.cpu().numpy().view(np.uint32)
        shared = span[:, 0] < span[:, 1]
        excluded = int((shared & (self.slot_over.cpu().numpy() != 0)).sum())
        dev = self.device
        return {'gain_solve': 'direct', 'gain_direct': self.gain_direct.clone(), 'gain_pair_index': index.to(torch.int32).to(dev),
                'gain_pair_words': pairs[index[:, 0], index[:, 1]].contiguous().to(dev), 'gain_diag': diag.to(dev), 'gain_excluded_cells': excluded,
                'gain_shared_cells': int(shared.sum()), 'gain_kept': [int(c) for c in self.gain_kept],
                'gain_components': mosaic_gain_groups(pairs.numpy(), diag.numpy()), 'gain_prior': float(MOSAIC_GAIN_PRIOR)}

    def run(self, batches, options: MosaicOptions = None, bounds=None, plain_atomic: bool = False, **fields) -> 'Mosaic':
        """Every phase over every batch, in the one order there is.  ``batches``: a sequence of ``(first_ordinal, load)``,
        ``load()`` returning the batch's ``(views, Js)`` -- called once per phase, so a caller may hold only some of the images at a
        time; ``options``: a ``MosaicOptions`` (``fields``: fields of the record laid over it), checked here;
        ``plain_atomic``: every phase that has one in its plain form.  The order: the bounds (unless ``bounds`` is given), ``begin``;
        with a surface ``add_surface`` -- or, with a support of M views, ``add_support`` over every batch for level 0, then for
        level 1, ... and ``finish_support``: M passes, and ``add_surface`` does not run --; with a reject tolerance
        ``add_reject_claim`` over every batch, then ``add_reject_sums`` over every batch, then ``finish_reject``; ``splat``; with
        gains ``add_span`` over every batch, R times ``gain_pass`` and ``solve_gains`` -- with the direct solve the first pass is
        followed by ``add_gain_slots`` over every batch, ``gain_pairs``, ``add_gain_diag`` over every batch and
        ``solve_gains_direct`` in place of the first ``solve_gains`` --, and one more ``gain_pass`` that measures the final state;
        ``resolve`` and ``gather``; with a blend ``accumulate`` and then ``normalize``; with bands ``accumulate_bands`` and then
        ``combine_bands``; with a fill ``fill``.  What a phase sees is the chain of ``_seen``: the claim and the sums of the
        consensus see the culled images; the splat, the span and the sums, slots and diag of the gains the culled and rejected ones;
        the gains' reference those times the gains as they stand; resolve, gather, accumulate and the bands the gained ones.  Every
        stage of the chain is made anew per phase and batch, unless one batch is the whole request: then each stage is made once,
        when the phases that fill it are through, and held until the run ends -- the same bits.  Returns the mosaic."""
        batches = list(batches)
        options = (options or MosaicOptions()).over(**fields).checked('Mosaic.run')
        if bounds is None:
            for _, load in batches:
                self.add_bounds(*load())
        self.begin(bounds, **{f: x for f, x in options.asked().items() if f != 'fill'})   # (the fill is a call of its own, below)

        def over_batches(phase, *args, **kw):
            for first, load in batches:
                phase(*load(), first, *args, **kw)

        def hold(stage, make, **kw):   # one batch is the whole request: the stage's copy is made once
            if len(batches) == 1:
                first, load = batches[0]
                self._held[stage] = make(*load(), first, **kw)

        self._held = {}
        try:
            if options.surface is not None:
                if options.support is None:
                    over_batches(self.add_surface, plain_atomic=plain_atomic)
                else:
                    for level in range(options.support):
                        over_batches(self.add_support, level, plain_atomic=plain_atomic)
                    self.finish_support()
                hold('cull', self.culled_images, count=True)
            if options.reject is not None:
                over_batches(self.add_reject_claim, plain_atomic=plain_atomic)
                over_batches(self.add_reject_sums, plain=plain_atomic)
                self.finish_reject()
                hold('reject', self.rejected_images, count=True)
            over_batches(self.splat, plain_atomic=plain_atomic)
            if options.gains is not None:
                over_batches(self.add_span, plain_atomic=plain_atomic)
                for r in range(options.gains):
                    self.gain_pass(batches, plain=plain_atomic)
                    if r == 0 and options.gain_solve == 'direct':
                        over_batches(self.add_gain_slots, plain=plain_atomic)
                        self.gain_pairs(plain=plain_atomic)
                        over_batches(self.add_gain_diag, plain=plain_atomic)
                        self.solve_gains_direct()
                    else:
                        self.solve_gains()
                self.gain_pass(batches, plain=plain_atomic)
                hold('gain', self.gained_images)
            over_batches(self.resolve)
            over_batches(self.gather)
            if options.blend is not None:
                over_batches(self.accumulate, plain=plain_atomic)
                self.normalize()
            if options.bands is not None:
                over_batches(self.accumulate_bands, plain=plain_atomic)
                self.combine_bands()
        finally:
            self._held = {}
        if options.fill is not None:
            self.fill(options.fill)
        return self


def mosaic_of(views: list, Js: list, axes, gsd, bounds=None, batch: int = 32, plain_atomic: bool = False, options: MosaicOptions = None,
              **fields) -> 'Mosaic':
    """``Mosaic.run`` over device-resident ``views`` / ``Js`` (ordinal = position in the list), ``batch`` images per call;
    ``options``: a ``MosaicOptions`` (``fields``: fields of the record laid over it -- ``blend=H``, ``fill=R``, ``surface=T``, ...),
    checked before anything is allocated; ``plain_atomic``: every phase that has one in its plain form."""
    views, Js = list(views), list(Js)
    if not views:
        raise ValueError('mosaic_of: no view')
    if len(views) > MAX_VIEWS:
        raise ValueError(f'mosaic_of: {len(views)} images, at most {MAX_VIEWS}')
    options = (options or MosaicOptions()).over(**fields).checked('mosaic_of')   # before anything is allocated
    batches = [(i, lambda i=i: (views[i:i + batch], Js[i:i + batch])) for i in range(0, len(views), batch)]
    return Mosaic(axes, gsd, views[0].depth.device).run(batches, options, bounds, plain_atomic)


def device_views_from_scene(scene, device='cuda') -> list[DeviceView]:
    """Uploads a synthetic scene (sucre_amd.synth) the way the loaders would: float32 depth, uint8 colour."""
    out = []
    for v in scene.views:
        out.append(DeviceView(depth=v.depth_f32().to(device).contiguous(), rgb=v.rgb_u8.to(device).contiguous(),
                              K=scene.K, R=v.R, t=v.t, name=v.name,
                              Kinv=getattr(scene, 'Kinv_given', None), tinv=getattr(v, 'tinv_given', None)))
    return out


class HipWaterBackend:
    """dist.WaterBackend over a Restoration: split grad/step launches around the host's all-reduce."""

    def __init__(self, restoration: Restoration, lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 use_closed_form: bool = False, trace: torch.Tensor | None = None):
        if restoration.light or restoration.float_colour:
            raise NotImplementedError('shared water parameters run on the plain water model with uint8 colours')
        self.r = restoration
        self.hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps))
        self.flags = (_lib.FIT_CLOSED_FORM if use_closed_form else 0) | restoration._fmt_flag
        self.trace = trace
        self._sums = restoration._region(_lib.WS_SUMS, torch.float64, 12)

    def grad_device(self):
        return self.r.device

    def n_obs(self) -> int:
        return self.r.n_obs()

    def set_n_obs_total(self, n: int) -> None:
        ws, H, W, nv = self.r._geom
        with torch.cuda.device(self.r.device):
            _lib.check(self.r.lib.sucre_set_n_obs_total(ws, H, W, nv, int(n), self.r._sp()))

    def grad(self, step: int) -> torch.Tensor:
        ws, H, W, nv = self.r._geom
        with torch.cuda.device(self.r.device):
            _lib.check(self.r.lib.sucre_fit_grad(ws, H, W, nv, int(step), *self.hyper, self.flags, self.r._sp()))
        return self._sums

    def step(self, step: int) -> None:
        ws, H, W, nv = self.r._geom
        row = C.c_void_p(self.trace[step - 1].data_ptr()) if self.trace is not None else None
        with torch.cuda.device(self.r.device):
            _lib.check(self.r.lib.sucre_fit_step(ws, H, W, nv, int(step), *self.hyper, row, self.r._sp()))
        self.r.steps_done = int(step)


class HipWaterGroup:
    """dist.WaterBackend over ALL the restorations of this rank (BASELINE config 4: a 512-image scene, 64 images per
    GPU, all sharing B, beta, gamma) with one launch and one collective per iteration: ``grad`` runs the gradient pass
    of every image in a single launch (csrc/fit.hip, group_iter_kernel) and returns the rank's ten sums for the
    all-reduce; the Adam step those sums call for is taken in the prologue of the next ``grad`` launch (``step`` only
    notes it) and ``finish`` takes the last one.  ``trace``: optional (T, 10) float64 device tensor.

    Light-model restorations (all of the group, uint8 colours) share the lamp too: one B, beta, gamma, cam2light, sigma
    (csrc/light.hip, sucre_light_group_*).  ``grad`` then runs every image's own gradient launch and one tail and returns
    the 19 sums, ``params0`` has 19 values, ``trace`` is (T, 20), and ``finish`` leaves the shared parameters in every
    image (``Restoration.params()``) and, in closed-form mode, every image's final J."""

    def __init__(self, restorations: list, lr: float = 0.05, betas=(0.9, 0.999), eps: float = 1e-8,
                 use_closed_form: bool = False, trace: torch.Tensor | None = None, params0=None):
        rs = [getattr(r, 'r', r) for r in restorations]      # Restoration objects (or HipWaterBackend wrappers)
        assert rs, 'need at least one image'
        if any(r.float_colour for r in rs):
            raise NotImplementedError('shared water parameters run on uint8 colours (no float32-colour restorations)')
        self.light = bool(rs[0].light)
        if any(r.light != self.light for r in rs):
            raise NotImplementedError('a shared-water group is all light-model restorations or all plain ones, not a mix')
        assert len({(r.obs_format, str(r.device)) for r in rs}) == 1, 'one device and one observation format per group'
        self.rs = rs
        self.lib = rs[0].lib
        self.device = rs[0].device
        self.hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps))
        self.closed = bool(use_closed_form)
        self.flags = (_lib.FIT_CLOSED_FORM if use_closed_form else 0) | rs[0]._fmt_flag
        self.trace = trace
        self.total = None
        self.steps_done = 0
        n = len(rs)
        npar = 19 if self.light else 9
        nbytes = self.lib.sucre_light_group_bytes(n) if self.light else self.lib.sucre_group_bytes(n)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        assert self.buf.data_ptr() % 256 == 0
        if params0 is None:
            p0 = np.concatenate([np.full(9, 0.1), np.zeros(6), [1.0, 0.0, 0.0, 1.0]])[:npar].astype(np.float32)  # sucre.py:41-46
        else:
            p0 = np.asarray(params0, np.float32).reshape(npar)
        p0c = (C.c_float * npar)(*p0.tolist())
        with torch.cuda.device(self.device):
            if self.light:
                table = (_lib.LightGroupImage * n)(*[_lib.LightGroupImage(r.ws.data_ptr(), r.lws.data_ptr(), r.H, r.W, r.n_views, 0)
                                                     for r in rs])
                _lib.check(self.lib.sucre_light_group_init(C.c_void_p(self.buf.data_ptr()), n, table, p0c, self._sp()))
            else:
                table = (_lib.GroupImage * n)(*[_lib.GroupImage(r.ws.data_ptr(), r.H, r.W, r.n_views, 0) for r in rs])
                _lib.check(self.lib.sucre_group_init(C.c_void_p(self.buf.data_ptr()), n, table, p0c, self._sp()))
        if self.light:
            off = self.lib.sucre_light_group_sums_offset()
            self._sums = self.buf[off:off + 19 * 8].view(torch.float64)
        else:
            off = self.lib.sucre_group_sums_offset()
            self._sums = self.buf[off:off + 96].view(torch.float64)

    def grad_device(self):
        return self.device

    def n_obs(self) -> int:
        return sum(r.n_obs() for r in self.rs)

    def set_n_obs_total(self, n: int) -> None:
        self.total = int(n)

    def _sp(self) -> C.c_void_p:   # a group launch touches every image's workspace
        sp = None
        for r in self.rs:
            sp = r._sp()
        return sp

    def _trace_ptr(self):
        return C.c_void_p(self.trace.data_ptr()) if self.trace is not None else None

    def grad(self, step: int) -> torch.Tensor:
        assert self.total, 'set_n_obs_total() first'
        if int(step) != self.steps_done + 1:
            # the water state is double-buffered by step parity and the pending step is taken by the NEXT launch: a group
            # runs iterations 1, 2, 3, ... once; starting over needs fit_init on the images and a new group
            raise _lib.SucreError(f'HipWaterGroup: iteration {step} asked after {self.steps_done} done -- iterations run in '
                                  f'order, once; build a new group (after fit_init) to fit again')
        with torch.cuda.device(self.device):
            if self.light:   # (the light model's closed-form pass solves J itself: no update_J to start from)
                _lib.check(self.lib.sucre_light_group_iter(C.c_void_p(self.buf.data_ptr()), len(self.rs), int(step), *self.hyper,
                                                           self.flags, self.total, self._trace_ptr(), self._sp()))
                return self._sums
            if self.closed and step == 1:   # start the one-pass closed-form kernel from a solved J (see sucre_fit_run)
                for r in self.rs:
                    r.update_J()
            _lib.check(self.lib.sucre_group_iter(C.c_void_p(self.buf.data_ptr()), len(self.rs), int(step), *self.hyper,
                                                 self.flags, self.total, self._trace_ptr(), self._sp()))
        return self._sums

    def step(self, step: int) -> None:
        self.steps_done = int(step)    # taken in the prologue of the next grad launch, or by finish()
        for r in self.rs:
            r.steps_done = int(step)

    def finish(self) -> None:
        with torch.cuda.device(self.device):
            if self.light:   # the last step, the parameters into every image, and the final update_J in closed-form mode
                _lib.check(self.lib.sucre_light_group_finish(C.c_void_p(self.buf.data_ptr()), len(self.rs), self.steps_done,
                                                             *self.hyper, self.flags, self.total, self._trace_ptr(), self._sp()))
                return
            _lib.check(self.lib.sucre_group_finish(C.c_void_p(self.buf.data_ptr()), len(self.rs), self.steps_done, *self.hyper,
                                                   self.total, self._trace_ptr(), self._sp()))
            if self.closed:
                for r in self.rs:
                    r.update_J()     # the final update_J of sucre.py:156 from the final parameters


_POOL: dict = {}
_STREAMS: dict = {}
_TLS = threading.local()   # .slot: the in-flight slot the calling THREAD is working for (see in_flight_slot); the CLI runs
                           # decode, plan and writer pools next to the main thread: a module global would leak a slot into them


def current_slot() -> int:
    return getattr(_TLS, 'slot', 0)


def current_lane() -> int:
    return getattr(_TLS, 'lane', 0)


@contextlib.contextmanager
def slot_lane(index: int):
    """The ``index``-th of several images that share ONE in-flight slot (a survey of small images whose fits advance in one
    launch per iteration, ``fit_batch``): inside the block ``acquire_restoration`` hands out that image's own workspace; the
    stream stays the slot's."""
    prev, _TLS.lane = current_lane(), int(index)
    try:
        yield
    finally:
        _TLS.lane = prev


def view_capacity(n: int) -> int:   # in steps, so targets whose surviving view counts differ a little share one workspace
    return (n + 7) // 8 * 8 if n <= 256 else (n + 31) // 32 * 32   # (65 views -> 72, not 96: +11 % HBM per slot, not +48 %)


def acquire_restoration(height: int, width: int, n_views: int, device='cuda', light: bool = False,
                        obs_format: str | None = None, float_colour: bool = False, tag: str = '') -> Restoration:
    """Workspace pool: one Restoration per (geometry, device, in-flight slot, tag), reused image after image (the
    1080p x 65-view workspace is ~2 GB; re-allocating it per image would serialise on the allocator) and grown when
    a target needs more views than it holds.  ``tag`` keeps side uses (``Image.match_two_way``) off the workspace a
    matches file is attached to."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if obs_format is None:   # engine knob for the reference-compatible CLI, which has no flag for it
        obs_format = 'f32' if (light or float_colour) else os.environ.get('SUCRE_OBS_FORMAT', 'f32')
    n = int(n_views)
    key = (int(height), int(width), str(dev), bool(light), (current_slot(), current_lane()), obs_format, bool(float_colour), tag)
    have = _POOL.get(key)
    if have is None or have.capacity < n:
        _POOL.pop(key, None)   # release the smaller workspace before allocating the larger one
        del have
        _POOL[key] = Restoration(height, width, view_capacity(n), device=dev, light=light, obs_format=obs_format, float_colour=float_colour)
    return _POOL[key]


_FREE: list = []   # leased workspaces handed back by their owners (lease_restoration / return_restoration)
_FREE_LOCK = threading.Lock()
_FREE_KEEP = 4      # at most this many idle workspaces are kept (a 1080p x 65-view one is ~2 GB)


def lease_restoration(height: int, width: int, n_views: int, device='cuda', light: bool = False,
                      obs_format: str | None = None, float_colour: bool = False) -> Restoration:
    """A workspace for ONE owner (a list-backed ``loader.MatchesData``): taken from the free list when an idle one of the
    same geometry and kind with enough capacity exists, allocated otherwise; nobody else sees it until the owner hands it
    back with ``return_restoration``.  ``obs_format`` None: the SUCRE_OBS_FORMAT knob, as in ``acquire_restoration``."""
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if obs_format is None:
        obs_format = 'f32' if (light or float_colour) else os.environ.get('SUCRE_OBS_FORMAT', 'f32')
    n = int(n_views)
    want = (int(height), int(width), str(dev), bool(light), obs_format, bool(float_colour))
    with _FREE_LOCK:
        for i, r in enumerate(_FREE):
            if (r.H, r.W, str(r.device), r.light, r.obs_format, r.float_colour) == want and r.capacity >= n:
                _FREE.pop(i)
                with torch.cuda.device(dev):   # whatever its last owner had enqueued on it comes first
                    for ev in r.__dict__.pop('_idle_after', []):
                        torch.cuda.current_stream(dev).wait_event(ev)
                return r
    return Restoration(height, width, view_capacity(n), device=dev, light=light, obs_format=obs_format, float_colour=float_colour)


def return_restoration(r: Restoration) -> None:
    """Hands a leased workspace back.  Its last owner's launches may still be queued: one event per stream the workspace
    was ever launched on (``Restoration._sp`` remembers them -- a user stream included; this function may run from a
    ``weakref.finalize`` on any thread, whose current stream says nothing) is left on it for the next owner to wait for."""
    r._keepalive = []
    try:
        with torch.cuda.device(r.device):
            streams = list(r._streams_used.values())
            r._streams_used = {}
            events = []
            for s in streams:
                ev = torch.cuda.Event()
                ev.record(s)
                events.append(ev)
            r.__dict__['_idle_after'] = events
    except Exception:   # interpreter shutdown: the workspace is going away with everything else
        return
    with _FREE_LOCK:
        if len(_FREE) < _FREE_KEEP and all(x is not r for x in _FREE):
            _FREE.append(r)


@contextlib.contextmanager
def in_flight_slot(index: int, device='cuda', wait_for_caller: bool = True):
    """Several images in flight on one GPU.  Code inside the block enqueues on slot ``index``'s own HIP stream and
    ``acquire_restoration`` hands out that slot's own workspace, so image i+1 (slot 1) can be submitted while image
    i (slot 0) is still iterating: the 200 launches of one fit depend on each other, and each ends in a short
    tail where a single workgroup reduces and steps the parameters -- a second image's kernels fill those tails
    (+13 % images/s at 1080p x 65 views, tools/dual_stream_probe.py).  Results of a slot must be read inside a
    block of the same slot (its stream is then the current one, so ``.cpu()`` waits for the right work).
    ``wait_for_caller=False``: the slot's stream does not wait for what the caller's stream holds -- for callers whose
    inputs are complete when they are handed over (``sfm.Image.device_view`` publishes a view only once its upload has
    landed); recording that dependency on the default stream costs the host up to 10 ms per image when other threads
    keep that stream busy with blocking copies (measured in the CLI, tools/cli_timeline.py)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = (str(dev), int(index))
    if key not in _STREAMS:
        _STREAMS[key] = torch.cuda.Stream(dev)
    stream = _STREAMS[key]
    if wait_for_caller:
        stream.wait_stream(torch.cuda.current_stream(dev))   # inputs uploaded / allocations freed on the caller's stream
    prev, _TLS.slot = current_slot(), int(index)
    try:
        with torch.cuda.stream(stream):
            yield stream
    finally:
        _TLS.slot = prev


def release_pool() -> None:
    with _FREE_LOCK:
        _FREE.clear()
    _POOL.clear()
    _STREAMS.clear()
