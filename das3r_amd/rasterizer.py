"""Host-side mirror of the `diff_gaussian_rasterization` Python surface on top of the
MI355X C-ABI library.

Same names, argument meaning, return values and error behaviour as the module DAS3R imports at
/root/reference/gaussian_renderer/__init__.py:14-17 and calls at :62-80,131-140
(upstream:diff_gaussian_rasterization/__init__.py): `GaussianRasterizationSettings` (12-field NamedTuple),
`GaussianRasterizer(nn.Module)` with `forward(...) -> (color[3,H,W], radii[P])` and `markVisible`.

How a call is wired: `_forward` returns a `RasterState` (the record of a finished forward) beside the images, `_backward` and the aux-channel
calls take it; `RasterState` alone fills the library's das3r_raster_saved.  `_RasterizeGaussians` is the one rasterising autograd function,
its per-call options an `_Options` argument.  `_forward_full` / `_backward_impl` / `check_forward` / `count_live_pairs` are the same calls
on plain tuples, for bench.py, the tools and the tests.
"""
import ctypes as C
import threading
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib

MAX_TILES = 1 << 22   # tiles of 16 x 16 pixels from which das3r_raster_forward refuses an image (csrc/render_common.h pack_tiles keeps 22 bits)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def cpu_deep_copy_tuple(input_tuple):
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


_EMPTY = {}


def _empty(device):
    """The 'not provided' placeholder (upstream passes torch.Tensor([])): one cached empty tensor per device."""
    t = _EMPTY.get(device)
    if t is None:
        t = _EMPTY[device] = torch.empty(0, dtype=torch.float32, device=device)
    return t


def _or_empty(device, *tensors):
    e = _empty(device)
    return tuple(e if t is None else t for t in tensors)


def _prep(t, device, name):
    """contiguous fp32 tensor on `device` (empty tensors mean 'not provided', as upstream)."""
    if t is None:
        return _empty(device)
    if t.dtype == torch.float32 and t.device == device and t.is_contiguous():   # the usual case, first
        return t
    if t.numel() == 0:  # 'not provided' placeholders (upstream passes CPU torch.Tensor([])) and P == 0 inputs: keep the shape
        return t.to(device=device, dtype=torch.float32)
    if t.numel() and t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    return t.contiguous()


def _small(t, device, n, name):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.is_contiguous()):
        t = torch.as_tensor(t, dtype=torch.float32, device=device).contiguous()
    if t.numel() != n:
        raise ValueError(f"{name} must have {n} elements")
    return t


def _dense(grad):
    """An upstream gradient as the library reads it: fp32, contiguous (None stays None)."""
    if grad is None:
        return None
    grad = grad.contiguous()
    return grad if grad.dtype == torch.float32 else grad.float()


def _chunks(n):
    """[(first channel, channels)] of the library calls that n aux channels take: DAS3R_AUX_MAX_CHANNELS at a time, one call for none."""
    return [(c0, min(_lib.AUX_MAX_CHANNELS, n - c0)) for c0 in range(0, max(n, 1), _lib.AUX_MAX_CHANNELS)]


def _scratch(nbytes, device, misalign=0, fill=None):
    """-> (tensor to keep alive, address for the library) of a scratch buffer the library writes before it reads.  Tests hand it one that
    is only 4-byte aligned (a C caller may) and fill it first."""
    nbytes, misalign = int(nbytes), int(misalign)
    t = torch.empty(nbytes + misalign, dtype=torch.uint8, device=device)
    if fill is not None:
        t[misalign:][:nbytes // 4 * 4].view(torch.float32).fill_(fill)
    return t, t.data_ptr() + misalign


def _new(device, fill=None):
    """-> z(*shape): an fp32 tensor on `device` that the library writes in full (fill: tests fill it first all the same)"""
    if fill is None:
        return lambda *shape: torch.empty(*shape, dtype=torch.float32, device=device)
    return lambda *shape: torch.full(shape, float(fill), dtype=torch.float32, device=device)


def _grad_set(device, P, M, has_sh, has_cov, chain=None, fill=None):
    """-> ((g_means2D, g_colors, g_opac, g_means3D, g_cov, g_sh, g_scales, g_rot), das3r_raster_grads pointing at them): only the gradients
    the call's inputs have, the others None / NULL.  chain (a _lib.Chain the caller keeps alive): the library goes on through the pose
    pre-transform and the Adam step itself — dL/d(camera-frame means, opacities, scales, rotations) are not produced.  Every tensor is
    written in full by the library (fill: tests fill them first all the same)."""
    z = _new(device, fill)
    g_means2D = z(P, 3)
    g_opac, g_means3D = (None, None) if chain is not None else (z(P, 1), z(P, 3))
    g_sh = z(P, M, 3) if has_sh else None
    g_colors = None if has_sh else z(P, 3)
    g_scales, g_rot = (None, None) if (has_cov or chain is not None) else (z(P, 3), z(P, 4))
    g_cov = z(P, 6) if has_cov else None
    g = _lib.RasterGrads()
    g.dL_dmeans2D, g.dL_dopacities, g.dL_dmeans3D = g_means2D.data_ptr(), _ptr(g_opac), _ptr(g_means3D)
    g.dL_dshs, g.dL_dcolors_precomp = _ptr(g_sh), _ptr(g_colors)
    g.dL_dscales, g.dL_drotations, g.dL_dcov3D = _ptr(g_scales), _ptr(g_rot), _ptr(g_cov)
    if chain is not None:
        g.chain = C.pointer(chain)
    return (g_means2D, g_colors, g_opac, g_means3D, g_cov, g_sh, g_scales, g_rot), g


class _Alloc:
    """Allocator callbacks handed to the library (upstream's resizeFunctional): torch owns the bytes.  One instance per
    device and host thread is kept alive (building ctypes callbacks costs tens of microseconds; threads must not share one:
    a forward on another thread would drop this thread's buffers); `take()` hands the buffers of the call that just finished
    to the caller and forgets them."""

    _local = threading.local()

    @classmethod
    def get(cls, device):
        per_device = getattr(cls._local, "per_device", None)
        if per_device is None:
            per_device = cls._local.per_device = {}
        a = per_device.get(device)
        if a is None:
            a = per_device[device] = cls(device)
        a.bufs = {}
        return a

    def take(self):
        b, self.bufs = self.bufs, {}
        return b

    def __init__(self, device):
        self.device = device
        self.bufs = {}
        self.fns = {k: _lib.ALLOC_FN(self._make(k)) for k in ("geom", "binning", "img")}

    def _make(self, key):
        def fn(_user, nbytes):
            try:
                t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
                self.bufs[key] = t
                return t.data_ptr()
            except Exception:  # noqa: BLE001 - reported by the library as DAS3R_ERR_ALLOC
                return 0
        return fn


def _fill_args(rs, P, M, device, keep):
    a = _lib.RasterArgs()
    a.P, a.sh_degree, a.M = P, int(rs.sh_degree), M
    a.image_width, a.image_height = int(rs.image_width), int(rs.image_height)
    a.tanfovx, a.tanfovy, a.scale_modifier = float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier)
    bg = _small(rs.bg, device, 3, "bg")
    vm = _small(rs.viewmatrix, device, 16, "viewmatrix")
    pm = _small(rs.projmatrix, device, 16, "projmatrix")
    cp = _small(rs.campos, device, 3, "campos")
    keep.extend([bg, vm, pm, cp])
    a.bg, a.viewmatrix, a.projmatrix, a.campos = bg.data_ptr(), vm.data_ptr(), pm.data_ptr(), cp.data_ptr()
    a.prefiltered, a.debug = int(bool(rs.prefiltered)), int(bool(rs.debug))
    return a


def _fill_in(means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp, pre=None):
    i = _lib.RasterIn()
    i.means3D, i.opacities = _ptr(means3D), _ptr(opacities)
    i.shs, i.colors_precomp = _ptr(sh), _ptr(colors_precomp)
    i.scales, i.rotations, i.cov3D_precomp = _ptr(scales), _ptr(rotations), _ptr(cov3Ds_precomp)
    if pre is not None:   # a _lib.PreTransform the caller keeps alive: the kernels take the pose pre-transform on their way in (ABI 14)
        i.pre = C.pointer(pre)
    return i


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
    if _raw_stream is not None and device.index is not None:
        return C.c_void_p(_raw_stream(device.index))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _on_device:
    """`with torch.cuda.device(device)` only when `device` is not already current (the context manager costs ~5 us)."""

    def __init__(self, device):
        self.ctx = None if device.index is None or torch.cuda.current_device() == device.index else torch.cuda.device(device)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


class _Capacity(int):
    """Instance capacity of a forward's binning buffer; also carries the forward's binning self-check ticket
    (das3r_raster_saved.check_word / check_tag) to the backward pass and to `check_forward`."""
    check_word = None
    check_tag = 0
    flags = 0   # das3r_raster_saved.flags of the forward (which compositing kernels its lists call for)


class RasterState:
    """The record of a finished forward, as the backward pass and the aux-channel calls take it (include/das3r_raster.h das3r_raster_saved):
    the three saved buffers, num_rendered and the capacity (a `_Capacity` also carries the forward's self-check ticket and flags; a plain int
    means none), P, W, H and the device.  Valid as long as it is kept, for any number of `composite_features` / `feature_adjoint` /
    `alpha_of` calls, before or after the forward's own backward pass.  `RasterState.of(res, rs)` wraps a `_forward_full` result."""
    __slots__ = ("geom", "binning", "img", "num_rendered", "capacity", "P", "W", "H", "device")

    def __init__(self, geom, binning, img, num_rendered, capacity, P, W, H, device):
        self.geom, self.binning, self.img = geom, binning, img
        self.num_rendered, self.capacity = int(num_rendered), capacity
        self.P, self.W, self.H, self.device = int(P), int(W), int(H), torch.device(device)

    @classmethod
    def of(cls, res, rs):
        """res: what `_forward_full` returned (num_rendered, color, radii, geom, binning, img, capacity, ...); rs: its settings."""
        return cls(res[3], res[4], res[5], res[0], res[6], res[2].shape[0], rs.image_width, rs.image_height, res[1].device)

    @property
    def flags(self):
        return int(getattr(self.capacity, "flags", 0))

    def saved(self, buffers=True):
        """The das3r_raster_saved of this forward: the one place that fills it.  The self-check ticket goes in when the capacity carries
        one (the library examines it before it launches anything); buffers=False: the ticket alone, all das3r_raster_check reads."""
        s = _lib.RasterSaved()
        if getattr(self.capacity, "check_tag", 0):
            s.check_word, s.check_tag = self.capacity.check_word, self.capacity.check_tag
        if buffers:
            s.geom, s.binning, s.img = _ptr(self.geom), _ptr(self.binning), _ptr(self.img)
            s.num_rendered, s.capacity, s.flags = self.num_rendered, int(self.capacity), self.flags
        return s

    def _c_args(self):
        """(the minimal das3r_raster_args — P and the image extents — and the saved struct) of the aux-channel calls"""
        a = _lib.RasterArgs()
        a.P, a.image_width, a.image_height = self.P, self.W, self.H
        return a, self.saved()

    def check(self):
        """Wait for this forward's binning self-check and raise RuntimeError if its image is invalid — for callers that render without a
        backward pass (evaluation); the backward pass does this itself before it launches anything (include/das3r_raster.h:
        das3r_raster_check)."""
        if not getattr(self.capacity, "check_tag", 0):
            return
        with _on_device(self.device):
            rc = _lib.load().das3r_raster_check(C.byref(self.saved(buffers=False)), _stream(self.device))
        _lib.check(rc, "das3r_raster_check")


def _forward(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, exact=False, pre=None, invdepth=False,
             no_backward=False, antialiasing=False):
    """-> (state, color, radii, inverse-depth image or None); the keywords are `_forward_full`'s."""
    lib = _lib.load()
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("das3r_amd rasterizer: tensors must live on a HIP device (torch device 'cuda'); "
                           "there is no CPU path")
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    P = means3D.shape[0]
    H, W = int(rs.image_height), int(rs.image_width)
    if W > 0 and H > 0 and ((W + 15) // 16) * ((H + 15) // 16) >= MAX_TILES:
        # the library's own refusal (csrc/forward.hip validate), raised before the image is allocated: 2^22 tiles are over a billion pixels
        raise RuntimeError(f"das3r_raster_forward failed (status {_lib.ERR_INVALID_ARG}): image of {W} x {H} pixels has 2^22 tiles or more")
    M = 0
    if sh.numel():
        if sh.dim() != 3 or sh.shape[0] != P or sh.shape[2] != 3:
            raise RuntimeError("shs must have dimensions (num_points, M, 3)")
        M = sh.shape[1]
    if P == 0:   # upstream: zero image, background not applied, empty radii
        e = torch.empty(0, dtype=torch.uint8, device=device)
        return (RasterState(e, e, e, 0, 0, 0, W, H, device), torch.zeros(3, H, W, dtype=torch.float32, device=device),
                torch.zeros(0, dtype=torch.int32, device=device), torch.zeros(1, H, W, dtype=torch.float32, device=device) if invdepth else None)
    # every pixel and every radii entry is written by the kernels: no memset needed
    color = torch.empty(3, H, W, dtype=torch.float32, device=device)
    radii = torch.empty(P, dtype=torch.int32, device=device)
    alloc = _Alloc.get(device)
    keep = []
    a = _fill_args(rs, P, M, device, keep)
    a.capacity_hint = -1 if exact else 0   # 0: the library may lay the binning buffer out with headroom (include/das3r_raster.h)
    i = _fill_in(means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp, pre)
    o = _lib.RasterOut()
    o.out_color, o.radii = color.data_ptr(), radii.data_ptr()
    inv = torch.empty(1, H, W, dtype=torch.float32, device=device) if invdepth else None
    o.out_invdepth = _ptr(inv)
    saved = _lib.RasterSaved()   # (the forward's own in / out struct: only the flags go in)
    saved.flags = (_lib.NO_BACKWARD_IN_FLAG if no_backward else 0) | (_lib.ANTIALIAS_FLAG if antialiasing else 0)
    with _on_device(device):
        rc = lib.das3r_raster_forward(C.byref(a), C.byref(i), C.byref(o), alloc.fns["geom"], alloc.fns["binning"],
                                      alloc.fns["img"], None, C.byref(saved), _stream(device))
    _lib.check(rc, "das3r_raster_forward")
    empty = torch.empty(0, dtype=torch.uint8, device=device)
    bufs = alloc.take()
    cap = _Capacity(saved.capacity)
    cap.check_word, cap.check_tag, cap.flags = saved.check_word, int(saved.check_tag), int(saved.flags)
    return RasterState(bufs.get("geom", empty), bufs.get("binning", empty), bufs.get("img", empty), rc, cap, P, W, H, device), color, radii, inv


def _backward(state, rs, grad_out_color, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, _scratch_misalign=0,
              pre=None, chain=None, grad_invdepth=None, focal=False, focal_per_splat=False, _fill=None):
    """The backward of the forward that left `state`; arguments and result as `_backward_impl`'s.  One library call: das3r_raster_backward,
    _backward_depth when an inverse-depth gradient arrives, _backward_focal when the focal sums are wanted."""
    lib = _lib.load()
    device, P = means3D.device, means3D.shape[0]
    M = sh.shape[1] if sh.numel() else 0
    grads, g = _grad_set(device, P, M, sh.numel() > 0, cov3Ds_precomp.numel() > 0, chain)
    z = _new(device)
    if P == 0:
        return grads + (torch.zeros(2, dtype=torch.float32, device=device), z(0, 2) if focal_per_splat else None) if focal else grads
    # per-instance partial sums, written by the render backward and added per Gaussian (no atomics, no memset by the caller)
    depth = grad_invdepth is not None
    nbytes = (lib.das3r_raster_backward_depth_scratch_bytes if depth else lib.das3r_raster_backward_scratch_bytes)(max(int(state.capacity), 1))
    scratch, g.scratch = _scratch(nbytes, device, _scratch_misalign, _fill)
    keep = []
    a = _fill_args(rs, P, M, device, keep)
    i = _fill_in(means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp, pre)
    saved = state.saved()
    dL = _dense(grad_out_color) if grad_out_color is not None else torch.zeros(3, state.H, state.W, dtype=torch.float32, device=device)
    dD = _dense(grad_invdepth)
    # the entry and what it takes besides (args, in, saved, dL_dpix, ..., grads, ..., stream)
    name, before, after, more = "das3r_raster_backward", (), (), ()
    if depth:
        name, before = "das3r_raster_backward_depth", (_ptr(dD),)
    if focal:   # (sums, per_splat and the workspace are written in full by the library; tests fill them first)
        sums, per = z(2), (z(P, 2) if focal_per_splat else None)
        work = torch.empty(int(lib.das3r_raster_focal_workspace_bytes(P)), dtype=torch.uint8, device=device)
        if _fill is not None:
            for t in (sums, per, work.view(torch.float32)):
                if t is not None:
                    t.fill_(_fill)
        name, before, after, more = "das3r_raster_backward_focal", (_ptr(dD),), (C.c_void_p(sums.data_ptr()), _ptr(per), C.c_void_p(work.data_ptr())), (sums, per)
    with _on_device(device):
        rc = getattr(lib, name)(C.byref(a), C.byref(i), C.byref(saved), C.c_void_p(dL.data_ptr()), *before, C.byref(g), *after, _stream(device))
    _lib.check(rc, name)
    return grads + more


# ---- the same calls on plain tuples: what bench.py, the tools and most tests use


def check_forward(capacity, device):
    """Wait for the binning self-check of the forward that returned `capacity` (the 7th element of `_forward_full`'s result) and
    raise RuntimeError if that forward's image is invalid (RasterState.check)."""
    RasterState(None, None, None, 0, capacity, 0, 0, 0, device).check()


def _forward_impl(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
    """-> (num_rendered, color, radii, geom, binning, img), the binning buffer laid out for exactly num_rendered instances
    (inspection helper of the tests and tools: `_lib.layout(P, num_rendered, W, H)` then describes the buffers)."""
    return _forward_full(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, exact=True)[:6]


def _forward_full(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, exact=False, pre=None, invdepth=False,
                  no_backward=False, antialiasing=False):
    """-> (num_rendered, color, radii, geom, binning, img, capacity); capacity >= num_rendered is what the binning buffer
    was laid out for (`_lib.layout(P, capacity, W, H)`), == num_rendered when `exact`.  invdepth: the inverse-depth image [1, H, W]
    (ABI 16, das3r_raster_out.out_invdepth) is appended to the tuple.  no_backward: no backward pass will follow (evaluation) — the
    library leaves out what only the backward reads (das3r_raster_saved.flags bit 3 on the way in).  antialiasing: upstream's 2D mip filter
    (flags bit 4 on the way in; the capacity's `flags` carry it back to `_backward_impl`, which then differentiates it)."""
    st, color, radii, inv = _forward(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, exact=exact, pre=pre,
                                     invdepth=invdepth, no_backward=no_backward, antialiasing=antialiasing)
    out = (st.num_rendered, color, radii, st.geom, st.binning, st.img, st.capacity)
    return out + (inv,) if invdepth else out


def _backward_impl(rs, num_rendered, grad_out_color, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                   geom, binning, img, capacity=None, _scratch_misalign=0, pre=None, chain=None, grad_invdepth=None, focal=False,
                   focal_per_splat=False, _fill=None):
    """-> (g_means2D, g_colors, g_opac, g_means3D, g_cov, g_sh, g_scales, g_rot), None for what the inputs do not have.
    capacity: the forward's (None: num_rendered, no self-check ticket, flags 0).
    grad_invdepth ([1, H, W] or None): also the backward of the forward's inverse-depth image (ABI 16, das3r_raster_backward_depth; the
    forward must have been made with invdepth=True).  grad_out_color may then be None (zero).
    focal: the same backward through das3r_raster_backward_focal — the result gains (sums [2], per_splat [P, 2] or None): dL/d(log-focal
    offsets) of the same loss and, with focal_per_splat, every splat's share of it (include/das3r_raster.h).
    chain (a _lib.Chain the caller keeps alive, with `pre`): see `_grad_set`.
    (_scratch_misalign, _fill: tests hand the library a scratch buffer that is only 4-byte aligned, and fill everything it is said to
    write without reading — the scratch, and with focal sums, per_splat and the workspace — with this value before the call.)"""
    state = RasterState(geom, binning, img, num_rendered, int(num_rendered) if capacity is None else capacity, means3D.shape[0],
                        rs.image_width, rs.image_height, means3D.device)
    return _backward(state, rs, grad_out_color, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                     _scratch_misalign=_scratch_misalign, pre=pre, chain=chain, grad_invdepth=grad_invdepth, focal=focal,
                     focal_per_splat=focal_per_splat, _fill=_fill)


def count_live_pairs(rs, P, M, num_rendered, geom, binning, img, capacity):
    """Measurement aid (include/das3r_raster.h das3r_raster_count_live_pairs): -> (live pairs, (pixel, list position) pairs below the
    pixels' last contributors) of the forward that produced these buffers (`_forward_full`'s results)."""
    device = geom.device
    keep = []
    a = _fill_args(rs, P, M, device, keep)
    saved = RasterState(geom, binning, img, num_rendered, int(capacity), P, rs.image_width, rs.image_height, device).saved()   # (no ticket)
    out = (C.c_uint64 * 2)()
    with _on_device(device):
        rc = _lib.load().das3r_raster_count_live_pairs(C.byref(a), C.byref(saved), out, _stream(device))
    _lib.check(rc, "das3r_raster_count_live_pairs")
    return int(out[0]), int(out[1])


# ---- aux channels over a forward's lists


def _check_state(state):
    if not isinstance(state, RasterState):
        raise TypeError(f"expected a das3r_amd.rasterizer.RasterState, got {type(state).__name__}")


def _needs_device(state):
    if state.device.type != "cuda":
        raise RuntimeError("das3r_amd rasterizer: the state must be that of a forward on a HIP device (torch device 'cuda'); there is no CPU path")


def _check_rows(state, t, name, shape_hint):
    """[P, C] / [C, H, W] fp32, dense, on the state's device — every mismatch is an error here, before the library is called."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor {shape_hint}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")


def _check_features(state, features, name="features"):
    _check_state(state)
    _check_rows(state, features, name, "[P, C]")
    if features.dim() != 2 or features.shape[1] < 1:
        raise ValueError(f"{name} must have dimensions (num_points, C >= 1), got {tuple(features.shape)}")
    if features.shape[0] != state.P:
        raise ValueError(f"{name} has {features.shape[0]} rows, the forward rasterised {state.P} Gaussians")
    if not features.is_contiguous():
        raise ValueError(f"{name} must be contiguous (row-major [P, C]); call .contiguous()")
    if features.device != state.device:
        raise RuntimeError(f"{name} is on {features.device}, the forward ran on {state.device}")


def _aux_forward(state, feat):
    """One das3r_raster_aux_forward call: feat [P, C <= 8] -> [C, H, W]."""
    _needs_device(state)
    lib = _lib.load()
    C_ = feat.shape[1]
    out = torch.empty(C_, state.H, state.W, dtype=torch.float32, device=state.device)   # fully written by the call
    a, saved = state._c_args()
    with _on_device(state.device):
        rc = lib.das3r_raster_aux_forward(C.byref(a), C.byref(saved), C_, _ptr(feat), C.c_void_p(out.data_ptr()), _stream(state.device))
    _lib.check(rc, "das3r_raster_aux_forward")
    return out


def _aux_adjoint(state, grad, out, accumulate):
    """One das3r_raster_aux_adjoint call: grad [C <= 8, H, W] -> out [P, C] (written, or added to)."""
    _needs_device(state)
    lib = _lib.load()
    C_ = grad.shape[0]
    nbytes = int(lib.das3r_raster_aux_scratch_bytes(max(int(state.capacity), 1), C_))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=state.device)   # per-instance rows, written before they are read
    a, saved = state._c_args()
    with _on_device(state.device):
        rc = lib.das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), C_, C.c_void_p(grad.data_ptr()), _ptr(out), int(bool(accumulate)),
                                          C.c_void_p(scratch.data_ptr()), _stream(state.device))
    _lib.check(rc, "das3r_raster_aux_adjoint")
    return out


class _CompositeFeatures(torch.autograd.Function):
    """composite_features with its adjoint: the gradient goes to `features` alone (the geometry is held constant; _AuxWithGeometry is the
    form that differentiates it)."""
    @staticmethod
    def forward(ctx, features, state):
        ctx.state = state
        return _composite(state, features)

    @staticmethod
    def backward(ctx, grad_image):
        return feature_adjoint(ctx.state, grad_image), None


def _composite(state, features):
    parts = [_aux_forward(state, features[:, c0:c0 + n].contiguous()) for c0, n in _chunks(features.shape[1])]
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def composite_features(state, features, geometry=None):
    """features [P, C] fp32 (one row per Gaussian of the forward that left `state`) -> [C, H, W]: per pixel sum_k features[g_k] alpha_k T_k
    over the splats the pixel's colour was blended from — same order, same alpha, same stop; no background term, an empty pixel is 0.
    Nothing of the forward is repeated (no preprocess, emission or sort).  Tensors wider than 8 channels take one library call per 8.
    geometry=None: differentiable with respect to `features` ONLY — alpha and T are the forward's and constant, no gradient reaches
    means, scales, rotations or opacities.  geometry=AuxGeometry(settings, the forward's input tensors): the image is differentiable with
    respect to those tensors as well (das3r_raster_aux_backward: one compositing kernel over the saved lists and the per-Gaussian backward;
    every discrete decision of the forward held fixed), and dL/dmean2D arrives in geometry.means2D.grad.  For a gradient of the COVERAGE use
    alpha_of(state, geometry=) / return_alpha, not a column of ones: the blend of ones differentiates to the same value through a
    cancellation that fp32 loses on pixels with hundreds of faint layers.  One workgroup per tile: on few tiles with ~10 k-entry lists it
    is slower than it could be (docs/ledger.md (ck))."""
    if geometry is not None:
        return _aux_with_geometry(state, features, geometry, False)[0]
    _check_features(state, features)
    if features.requires_grad and torch.is_grad_enabled():
        return _CompositeFeatures.apply(features, state)
    return _composite(state, features.detach())


def feature_adjoint(state, grad_image, out=None, accumulate=False):
    """The adjoint of composite_features: grad_image [C, H, W] -> [P, C] = sum over pixels of alpha T grad_image per Gaussian; with a ones
    image and C = 1, every Gaussian's blending-weight mass in the view (das3r_amd.prune.contribution_scores).  out: a dense [P, C] fp32
    tensor to write into; accumulate: add to `out` instead (needs `out`).  Rows of Gaussians that were not rendered are exactly 0.  No
    floating-point atomics: bit-identical from run to run."""
    _check_state(state)
    _check_rows(state, grad_image, "grad_image", "[C, H, W]")
    if grad_image.dim() != 3 or grad_image.shape[0] < 1 or tuple(grad_image.shape[1:]) != (state.H, state.W):
        raise ValueError(f"grad_image must have dimensions (C >= 1, {state.H}, {state.W}), got {tuple(grad_image.shape)}")
    if grad_image.device != state.device:
        raise RuntimeError(f"grad_image is on {grad_image.device}, the forward ran on {state.device}")
    n = grad_image.shape[0]
    if out is None:
        if accumulate:
            raise ValueError("feature_adjoint(accumulate=True) needs the tensor to add to (out=)")
        out = torch.empty(state.P, n, dtype=torch.float32, device=state.device)
    else:
        _check_features(state, out, "out")
        if out.shape[1] != n:
            raise ValueError(f"out has {out.shape[1]} channels, grad_image {n}")
    grad_image = grad_image.detach().contiguous()
    if n <= _lib.AUX_MAX_CHANNELS:
        return _aux_adjoint(state, grad_image, out, accumulate)
    for c0, c in _chunks(n):   # (a column block of `out` is not dense: each call writes a tensor of its own)
        part = _aux_adjoint(state, grad_image[c0:c0 + c], torch.empty(state.P, c, dtype=torch.float32, device=state.device), False)
        if accumulate:
            out[:, c0:c0 + c] += part
        else:
            out[:, c0:c0 + c] = part
    return out


def alpha_of(state, geometry=None):
    """-> [1, H, W] = 1 - final_T: the coverage of the forward that left `state`, read out of its saved image buffer (the transmittance
    every forward stores for its backward pass; include/das3r_raster.h das3r_raster_get_layout).  Exactly 0 where nothing was blended.
    A view of what is there: no kernel of the library is launched.  geometry=AuxGeometry(...): the same image, differentiable with respect
    to the forward's geometry inputs (composite_features' docstring)."""
    if geometry is not None:
        return _aux_with_geometry(state, None, geometry, True)[1]
    _check_state(state)
    _needs_device(state)
    npix = state.H * state.W
    if state.P == 0 or state.img.numel() == 0:
        return torch.zeros(1, state.H, state.W, dtype=torch.float32, device=state.device)
    L = _lib.layout(state.P, int(state.capacity) if int(state.capacity) > 0 else state.num_rendered, state.W, state.H)
    T = state.img[L["final_T"]:L["final_T"] + 4 * npix].view(torch.float32).reshape(1, state.H, state.W)
    return 1.0 - T


class AuxGeometry:
    """The settings and input tensors of a forward, as `composite_features(state, features, geometry=)` / `alpha_of(state, geometry=)` take
    them to send an aux image's or the coverage image's gradient to the geometry: the GaussianRasterizationSettings the forward ran with and
    the tensors it was given (means2D: the dummy leaf whose .grad receives dL/dmean2D; shs / colors_precomp are not differentiated here — the
    per-Gaussian backward reads the forward's inputs — exactly one of them, and scales + rotations or cov3D_precomp, as for the forward)."""
    __slots__ = ("raster_settings", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")

    def __init__(self, raster_settings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                 cov3D_precomp=None):
        self.raster_settings = raster_settings
        self.means3D, self.means2D, self.opacities = means3D, means2D, opacities
        self.shs, self.colors_precomp, self.scales, self.rotations, self.cov3D_precomp = shs, colors_precomp, scales, rotations, cov3D_precomp


def _given(t):
    return t is not None and t.numel() > 0


def _check_geometry(state, geometry):
    """What the aux backward cannot take is refused here, before the library is reached."""
    _check_state(state)
    if not isinstance(geometry, AuxGeometry):
        raise TypeError(f"geometry must be a das3r_amd.rasterizer.AuxGeometry, got {type(geometry).__name__}")
    _needs_device(state)
    rs = geometry.raster_settings
    if (int(rs.image_width), int(rs.image_height)) != (state.W, state.H):
        raise ValueError(f"geometry.raster_settings is {int(rs.image_width)} x {int(rs.image_height)}, the forward rendered {state.W} x {state.H}")
    for name in ("means3D", "means2D", "opacities"):
        t = getattr(geometry, name)
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != state.P:
            raise ValueError(f"geometry.{name} must be the forward's own tensor ({state.P} rows)")
        if t.device != state.device:
            raise RuntimeError(f"geometry.{name} is on {t.device}, the forward ran on {state.device}")
    if _given(geometry.shs) == _given(geometry.colors_precomp) and state.P > 0:
        raise ValueError("geometry needs exactly one of shs / colors_precomp (the forward's own)")
    if state.P > 0 and (_given(geometry.scales) and _given(geometry.rotations)) == _given(geometry.cov3D_precomp):
        raise ValueError("geometry needs exactly one of the scales + rotations pair / cov3D_precomp (the forward's own)")
    for name in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"):
        t = getattr(geometry, name)
        if _given(t) and t.shape[0] != state.P:
            raise ValueError(f"geometry.{name} has {t.shape[0]} rows, the forward rasterised {state.P} Gaussians")


def _saved_list_backward(name, scratch_bytes, call_args, state, rs, inputs, _scratch_misalign, _fill):
    """One call of a backward over a forward's saved lists that ends in the per-Gaussian backward -> (g_means2D, g_opac, g_means3D, g_cov,
    g_scales, g_rot).  name: the library entry (das3r_raster_aux_backward / das3r_raster_distortion_backward); scratch_bytes: what its
    scratch takes, from its _scratch_bytes function; call_args: what it takes between the saved state and the gradient set; inputs: the
    forward's (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)."""
    means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = inputs
    device, P = state.device, state.P
    M = sh.shape[1] if sh.numel() else 0
    # (the colour gradient is identically zero for these losses; the per-Gaussian backward writes it all the same)
    (g_means2D, _g_colors, g_opac, g_means3D, g_cov, _g_sh, g_scales, g_rot), g = _grad_set(device, P, M, sh.numel() > 0, cov3Ds_precomp.numel() > 0,
                                                                                           fill=_fill)
    if P > 0:
        scratch, g.scratch = _scratch(scratch_bytes, device, _scratch_misalign, _fill)   # everything in it is written before it is read
        keep = []
        a = _fill_args(rs, P, M, device, keep)
        i = _fill_in(means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp)
        saved = state.saved()
        with _on_device(device):
            rc = getattr(_lib.load(), name)(C.byref(a), C.byref(i), C.byref(saved), *call_args, C.byref(g), _stream(device))
        _lib.check(rc, name)
    return g_means2D, g_opac, g_means3D, g_cov, g_scales, g_rot


def _aux_backward_impl(state, rs, features, grad_image, grad_alpha, want_features, means3D, sh, colors_precomp, opacities, scales, rotations,
                       cov3Ds_precomp, _scratch_misalign=0, _fill=None):
    """One das3r_raster_aux_backward call: the backward of <grad_image, composite_features(features)> + <grad_alpha, alpha_of> for the forward
    that left `state` -> (g_means2D, g_opac, g_means3D, g_cov, g_scales, g_rot, g_features or None).  features [P, C <= 8] / grad_image
    [C, H, W] or both None (coverage alone); grad_alpha [1, H, W] or None.  (_fill: tests fill the scratch and every output with it first.)"""
    lib = _lib.load()
    C_ = 0 if features is None else int(features.shape[1])
    g_feat = _new(state.device, _fill)(state.P, C_) if want_features and C_ > 0 else None
    nbytes = lib.das3r_raster_aux_backward_scratch_bytes(max(int(state.capacity), 1), C_) if state.P else 0   # (no Gaussian: no call)
    return _saved_list_backward("das3r_raster_aux_backward", nbytes,
                                (C_, _ptr(features), _ptr(grad_image), _ptr(grad_alpha), _ptr(g_feat)), state, rs,
                                (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), _scratch_misalign, _fill) + (g_feat,)


def _prep_geometry(device, means3D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp):
    """The seven forward inputs the two autograd functions below save for their backward calls, in this order"""
    return [_prep(t, device, n) for t, n in ((means3D, "means3D"), (opacities, "opacities"), (scales, "scales"), (rotations, "rotations"),
                                             (cov3Ds_precomp, "cov3D_precomp"), (sh, "shs"), (colors_precomp, "colors_precomp"))]


class _AuxWithGeometry(torch.autograd.Function):
    """(feature image or None, alpha or None) of a forward's saved lists, differentiable with respect to `features` AND the forward's geometry
    inputs: the backward is ONE das3r_raster_aux_backward call for both upstream gradients (one per 8 channels of a wider tensor), and returns
    dL/dmean2D for the dummy means2D leaf — autograd adds it to the colour loss's there."""
    @staticmethod
    def forward(ctx, features, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp, raster_settings, state,
                want_alpha):
        device = state.device
        tensors = _prep_geometry(device, means3D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp)
        feat = None if features is None else _prep(features.detach(), device, "features")
        ctx.state, ctx.raster_settings, ctx.has_features = state, raster_settings, feat is not None
        ctx.save_for_backward(*tensors, *(() if feat is None else (feat,)))
        ctx.set_materialize_grads(False)
        image = None if feat is None else _composite(state, feat)
        alpha = alpha_of(state) if want_alpha else None
        return image, alpha

    @staticmethod
    def backward(ctx, grad_image, grad_alpha):
        if grad_image is None and grad_alpha is None:
            return (None,) * 12
        saved = ctx.saved_tensors
        means3D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp = saved[:7]
        grad_image, grad_alpha = _dense(grad_image), _dense(grad_alpha)
        feat = saved[7] if ctx.has_features and grad_image is not None else None
        want_feat = feat is not None and ctx.needs_input_grad[0]
        out = None
        # a call per 8 channels, the coverage term with the first; every gradient is linear in the loss terms
        for c0, n in _chunks(0 if feat is None else feat.shape[1]):
            part = _aux_backward_impl(ctx.state, ctx.raster_settings, None if feat is None else feat[:, c0:c0 + n].contiguous(),
                                      None if feat is None else grad_image[c0:c0 + n], grad_alpha if c0 == 0 else None, want_feat,
                                      means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
            out = part if out is None else tuple(None if x is None else (torch.cat((x, y), 1) if k == 6 else x + y)
                                                 for k, (x, y) in enumerate(zip(out, part)))
        g_means2D, g_opac, g_means3D, g_cov, g_scales, g_rot, g_feat = out
        return (g_feat, g_means3D, g_means2D, g_opac, g_scales if scales.numel() else None, g_rot if rotations.numel() else None,
                g_cov if cov3Ds_precomp.numel() else None, None, None, None, None, None)


def _aux_with_geometry(state, features, geometry, want_alpha):
    """-> (feature image or None, alpha or None) through _AuxWithGeometry; the checks of composite_features / _check_geometry first."""
    _check_geometry(state, geometry)
    if features is not None:
        _check_features(state, features)
    elif not want_alpha:
        raise ValueError("nothing to render: neither features nor the coverage image was asked for")
    return _AuxWithGeometry.apply(features, geometry.means3D, geometry.means2D, geometry.opacities,
                                  *_or_empty(state.device, geometry.scales, geometry.rotations, geometry.cov3D_precomp, geometry.shs,
                                             geometry.colors_precomp), geometry.raster_settings, state, bool(want_alpha))


# ---- the ray-distortion regulariser over a forward's lists


def _distortion_forward(state, want_totals, _fill=None):
    """One das3r_raster_distortion_forward call -> (D [1, H, W], the totals plane [H, W] its backward takes, or None)."""
    _needs_device(state)
    lib = _lib.load()
    z = _new(state.device, _fill)   # both fully written by the call
    out = z(1, state.H, state.W)
    totals = z(state.H, state.W) if want_totals else None
    a, saved = state._c_args()
    with _on_device(state.device):
        rc = lib.das3r_raster_distortion_forward(C.byref(a), C.byref(saved), C.c_void_p(out.data_ptr()),
                                                 None if totals is None else C.c_void_p(totals.data_ptr()), _stream(state.device))
    _lib.check(rc, "das3r_raster_distortion_forward")
    return out, totals


def _distortion_backward_impl(state, rs, grad, totals, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                              _scratch_misalign=0, _fill=None):
    """One das3r_raster_distortion_backward call: the backward of <grad, distortion_of> for the forward that left `state` ->
    (g_means2D, g_opac, g_means3D, g_cov, g_scales, g_rot).  grad [1, H, W], totals [H, W]: the forward call's.  (_fill: tests fill the scratch
    and every output with it first.)"""
    lib = _lib.load()
    nbytes = lib.das3r_raster_distortion_backward_scratch_bytes(max(int(state.capacity), 1), state.P) if state.P else 0   # (no Gaussian: no call)
    return _saved_list_backward("das3r_raster_distortion_backward", nbytes,
                                (C.c_void_p(grad.data_ptr()), C.c_void_p(totals.data_ptr())), state, rs,
                                (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), _scratch_misalign, _fill)


class _DistortionWithGeometry(torch.autograd.Function):
    """distortion_of, differentiable with respect to the forward's geometry inputs: the forward is one das3r_raster_distortion_forward call
    (which leaves the totals plane), the backward ONE das3r_raster_distortion_backward call; dL/dmean2D goes to the dummy means2D leaf, where
    autograd adds it to the colour loss's."""
    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp, raster_settings, state):
        device = state.device
        tensors = _prep_geometry(device, means3D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp)
        image, totals = _distortion_forward(state, True)
        ctx.state, ctx.raster_settings = state, raster_settings
        ctx.save_for_backward(*tensors, totals)
        ctx.set_materialize_grads(False)
        return image

    @staticmethod
    def backward(ctx, grad):
        if grad is None:
            return (None,) * 10
        means3D, opacities, scales, rotations, cov3Ds_precomp, sh, colors_precomp, totals = ctx.saved_tensors
        g_means2D, g_opac, g_means3D, g_cov, g_scales, g_rot = _distortion_backward_impl(
            ctx.state, ctx.raster_settings, _dense(grad), totals, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        return (g_means3D, g_means2D, g_opac, g_scales if scales.numel() else None, g_rot if rotations.numel() else None,
                g_cov if cov3Ds_precomp.numel() else None, None, None, None, None)


def distortion_of(state, geometry=None):
    """-> [1, H, W]: the ray-distortion regulariser (Mip-NeRF 360, 2DGS) of the forward that left `state`, per pixel
        D = sum_{j<k} w_j w_k (m_j - m_k) = 1/2 sum_i sum_j w_i w_j |m_i - m_j|,    w_k = alpha_k T_k,  m_k = 1 / z_k,
    over the splats the pixel's colour was blended from — same order (depth, index), same alpha, same stop; z the fp32 view-space depth the
    forward saved; no background term; an empty pixel and a pixel with one contributor are exactly 0 (include/das3r_raster.h
    das3r_raster_distortion_forward).  Nothing of the forward is repeated: one kernel over the saved lists.
    geometry=None: a plain tensor.  geometry=AuxGeometry(settings, the forward's input tensors): differentiable with respect to means3D,
    opacities, scales and rotations or cov3D_precomp, and dL/dmean2D arrives in geometry.means2D.grad (das3r_raster_distortion_backward: one
    compositing kernel, a per-Gaussian fold of dL/d(1/z), the per-Gaussian backward; every discrete decision of the forward held fixed).  No
    floating-point atomics: bit-identical from run to run.  One workgroup per tile: on few tiles with ~10 k-entry lists it is slower than it
    could be (docs/ledger.md (cq))."""
    if geometry is None:
        _check_state(state)
        return _distortion_forward(state, False)[0]
    _check_geometry(state, geometry)
    return _DistortionWithGeometry.apply(geometry.means3D, geometry.means2D, geometry.opacities,
                                         *_or_empty(state.device, geometry.scales, geometry.rotations, geometry.cov3D_precomp, geometry.shs,
                                                    geometry.colors_precomp), geometry.raster_settings, state)


# ---- median depth and surface hits over a forward's lists


def _check_threshold(threshold):
    """-> the threshold as a float inside (0, 1); anything else (NaN included) is refused here, before the library is reached."""
    try:
        tau = float(threshold)
    except (TypeError, ValueError):
        raise TypeError(f"threshold must be a number inside (0, 1), got {type(threshold).__name__}") from None
    if not (0.0 < tau < 1.0):
        raise ValueError(f"threshold must be inside (0, 1) (0.5: the median), got {tau}")
    return tau


def _median_forward(state, tau, want_gaussian, want_position, _fill=None):
    """One das3r_raster_median_forward call -> (depth [1, H, W], hit_gaussian [H, W] int32 or None, hit_position [H, W] int32 or None).  The
    position plane is the library's u32 plane held in an int32 tensor: the empty marker 0xFFFFFFFF reads -1."""
    _needs_device(state)
    lib = _lib.load()
    depth = _new(state.device, _fill)(1, state.H, state.W)   # all three fully written by the call
    plane = lambda want: torch.empty(state.H, state.W, dtype=torch.int32, device=state.device) if want else None
    hit_g, hit_p = plane(want_gaussian), plane(want_position)
    a, saved = state._c_args()
    with _on_device(state.device):
        rc = lib.das3r_raster_median_forward(C.byref(a), C.byref(saved), C.c_float(tau), C.c_void_p(depth.data_ptr()),
                                             None if hit_g is None else C.c_void_p(hit_g.data_ptr()),
                                             None if hit_p is None else C.c_void_p(hit_p.data_ptr()), _stream(state.device))
    _lib.check(rc, "das3r_raster_median_forward")
    return depth, hit_g, hit_p


def _check_hit_position(state, hit_position):
    if not torch.is_tensor(hit_position):
        raise TypeError("hit_position must be the int32 [H, W] plane median_depth_of(return_position=True) returned")
    if hit_position.dtype != torch.int32:
        raise TypeError(f"hit_position must be int32 (got {hit_position.dtype})")
    if tuple(hit_position.shape) != (state.H, state.W):
        raise ValueError(f"hit_position must have dimensions ({state.H}, {state.W}), got {tuple(hit_position.shape)}")
    if hit_position.device != state.device:
        raise RuntimeError(f"hit_position is on {hit_position.device}, the forward ran on {state.device}")


def _median_adjoint(state, grad, hit_position, out, accumulate, _fill=None):
    """One das3r_raster_median_adjoint call: grad [H, W], hit_position [H, W] int32 -> out [P] (written, or added to)."""
    _needs_device(state)
    lib = _lib.load()
    if state.P == 0:
        return out   # no row
    nbytes = int(lib.das3r_raster_median_scratch_bytes(max(int(state.capacity), 1)))
    scratch, address = _scratch(nbytes, state.device, 0, _fill)   # per-instance floats, written before they are read
    a, saved = state._c_args()
    with _on_device(state.device):
        rc = lib.das3r_raster_median_adjoint(C.byref(a), C.byref(saved), C.c_void_p(grad.data_ptr()), C.c_void_p(hit_position.data_ptr()),
                                             C.c_void_p(out.data_ptr()), int(bool(accumulate)), C.c_void_p(address), _stream(state.device))
    _lib.check(rc, "das3r_raster_median_adjoint")
    return out


def median_hit_adjoint(state, grad_image, hit_position, out=None, accumulate=False, _fill=None):
    """The adjoint of median_depth_of with respect to the Gaussians' view-space depths: grad_image [H, W] (or [1, H, W]), hit_position the
    int32 [H, W] plane median_depth_of(return_position=True) returned -> [P], dL_dz[i] = the sum of grad_image over the pixels whose hit is
    Gaussian i; with a ones image, the number of pixels every Gaussian is the visible surface of (das3r_amd.prune.surface_scores).  out: a
    dense [P] fp32 tensor to write into; accumulate: add to `out` instead (needs `out`).  A Gaussian that is nobody's hit gets exactly 0;
    a position at or past its tile's list length (the empty marker -1 among them) contributes nothing.  No floating-point atomics:
    bit-identical from run to run."""
    _check_state(state)
    _check_rows(state, grad_image, "grad_image", "[H, W]")
    if tuple(grad_image.shape) not in ((state.H, state.W), (1, state.H, state.W)):
        raise ValueError(f"grad_image must have dimensions ({state.H}, {state.W}), got {tuple(grad_image.shape)}")
    if grad_image.device != state.device:
        raise RuntimeError(f"grad_image is on {grad_image.device}, the forward ran on {state.device}")
    _check_hit_position(state, hit_position)
    if out is None:
        if accumulate:
            raise ValueError("median_hit_adjoint(accumulate=True) needs the tensor to add to (out=)")
        out = _new(state.device, _fill)(state.P)
    else:
        _check_rows(state, out, "out", "[P]")
        if tuple(out.shape) != (state.P,) or not out.is_contiguous():
            raise ValueError(f"out must be a dense tensor of {state.P} elements, got {tuple(out.shape)}")
        if out.device != state.device:
            raise RuntimeError(f"out is on {out.device}, the forward ran on {state.device}")
    return _median_adjoint(state, grad_image.detach().contiguous(), hit_position.contiguous(), out, accumulate, _fill)


class _MedianWithGeometry(torch.autograd.Function):
    """median_depth_of, differentiable with respect to means3D: the forward is one das3r_raster_median_forward call (which leaves the hit
    positions), the backward ONE das3r_raster_median_adjoint call -> dL_dz [P], handed on as dL_dz[:, None] * viewmatrix[:3, 2][None] — the
    forward's own z = [x y z 1] . viewmatrix[:, 2]; a row-wise product: deterministic."""
    @staticmethod
    def forward(ctx, means3D, raster_settings, state, tau):
        depth, hit_g, hit_p = _median_forward(state, tau, True, True)
        ctx.state = state
        ctx.z_row = raster_settings.viewmatrix.detach().to(device=state.device, dtype=torch.float32).reshape(4, 4)[:3, 2].clone()
        ctx.save_for_backward(hit_p)
        ctx.mark_non_differentiable(hit_g, hit_p)
        ctx.set_materialize_grads(False)
        return depth, hit_g, hit_p

    @staticmethod
    def backward(ctx, grad, _grad_g=None, _grad_p=None):
        if grad is None:
            return None, None, None, None
        (hit_p,) = ctx.saved_tensors
        state = ctx.state
        dz = _median_adjoint(state, _dense(grad), hit_p, torch.empty(state.P, dtype=torch.float32, device=state.device), False)
        return dz[:, None] * ctx.z_row[None], None, None, None


def median_depth_of(state, geometry=None, threshold=0.5, return_hit=False, return_position=False):
    """-> [1, H, W]: the median depth of the forward that left `state` — per pixel the fp32 view-space depth z of the HIT, the entry at
    which the ray's transmittance crosses `threshold`:
        hit = max { k < n : T_k > threshold },    T_0 = 1,  T_{k+1} = T_k (1 - alpha_k),
    over the splats the pixel's colour was blended from — same order (depth, index), same alpha, same stop: the first entry behind which
    T <= threshold, or the last contributor of a ray that never gets that opaque.  0 < threshold < 1; 0.5 is the median, a smaller value a
    deeper quantile.  No background term; an empty pixel is exactly 0 (include/das3r_raster.h das3r_raster_median_forward).  Nothing of the
    forward is repeated: one kernel over the saved lists, which a wave leaves as soon as its pixels are behind their hits.
    return_hit: also the int32 [H, W] plane of the hit's Gaussian index (-1: empty pixel).  return_position: also the int32 [H, W] plane of
    the hit's 0-based position in its tile's list (-1: empty pixel), which median_hit_adjoint takes back.  With either, a tuple in that order.
    geometry=None: plain tensors.  geometry=AuxGeometry(settings, the forward's input tensors): the depth is differentiable with respect to
    geometry.means3D ALONE (das3r_raster_median_adjoint: every discrete decision of the forward and the choice of the hit held fixed, so a
    pixel's gradient moves its hit Gaussian along the view axis); no other input receives a gradient.  No floating-point atomics:
    bit-identical from run to run."""
    tau = _check_threshold(threshold)
    if geometry is None:
        _check_state(state)
        depth, hit_g, hit_p = _median_forward(state, tau, bool(return_hit), bool(return_position))
    else:
        _check_geometry(state, geometry)
        depth, hit_g, hit_p = _MedianWithGeometry.apply(geometry.means3D, geometry.raster_settings, state, tau)
    extra = ((hit_g,) if return_hit else ()) + ((hit_p,) if return_position else ())
    return (depth,) + extra if extra else depth


# ---- the normal-consistency regulariser: per-Gaussian normals, depth normals, the loss image


def _normals_args(rs, P, device, keep):
    """The das3r_raster_args of the per-Gaussian normal calls: P, viewmatrix and campos (and debug)."""
    a = _lib.RasterArgs()
    a.P, a.debug = int(P), int(bool(rs.debug))
    vm = _small(rs.viewmatrix, device, 16, "viewmatrix")
    cp = _small(rs.campos, device, 3, "campos")
    keep.extend([vm, cp])
    a.viewmatrix, a.campos = vm.data_ptr(), cp.data_ptr()
    return a


def _gaussian_normals_forward(rs, rotations, scales, means3D, _fill=None):
    """One das3r_gaussian_normals_forward call -> (normals [P, 3], choice [P] uint8: k | flip << 2)."""
    device, P = rotations.device, rotations.shape[0]
    normals = _new(device, _fill)(P, 3)   # both fully written by the call
    choice = torch.empty(P, dtype=torch.uint8, device=device)
    keep = []
    a = _normals_args(rs, P, device, keep)
    with _on_device(device):
        rc = _lib.load().das3r_gaussian_normals_forward(C.byref(a), _ptr(rotations), _ptr(scales), _ptr(means3D), _ptr(normals), _ptr(choice),
                                                        _stream(device))
    _lib.check(rc, "das3r_gaussian_normals_forward")
    return normals, choice


def _gaussian_normals_backward(rs, rotations, choice, grad, out=None, accumulate=False, _fill=None):
    """One das3r_gaussian_normals_backward call: grad [P, 3] -> dL/drotations [P, 4] (written, or added to `out`)."""
    device, P = rotations.device, rotations.shape[0]
    if out is None:
        out = _new(device, _fill)(P, 4)
    keep = []
    a = _normals_args(rs, P, device, keep)
    with _on_device(device):
        rc = _lib.load().das3r_gaussian_normals_backward(C.byref(a), _ptr(rotations), _ptr(choice), _ptr(grad), _ptr(out), int(bool(accumulate)),
                                                         _stream(device))
    _lib.check(rc, "das3r_gaussian_normals_backward")
    return out


class _GaussianNormals(torch.autograd.Function):
    """gaussian_normals with its backward: the gradient goes to `rotations` alone (the thinnest axis and the flip are the forward's)."""
    @staticmethod
    def forward(ctx, rotations, scales, means3D, raster_settings):
        normals, choice = _gaussian_normals_forward(raster_settings, rotations, scales, means3D)
        ctx.raster_settings = raster_settings
        ctx.save_for_backward(rotations, choice)
        return normals

    @staticmethod
    def backward(ctx, grad):
        rotations, choice = ctx.saved_tensors
        return _gaussian_normals_backward(ctx.raster_settings, rotations, choice, _dense(grad)), None, None, None


def gaussian_normals(raster_settings, rotations, scales, means3D):
    """-> [P, 3]: every Gaussian's normal in view space — the axis of its smallest scale (ties: the lowest index), column k of R(q / |q|),
    turned to face the camera (negated when axis . (mean - campos) > 0; a product of exactly 0 keeps it) and taken into view space by the
    rotation part of raster_settings.viewmatrix (include/das3r_raster.h das3r_gaussian_normals_forward).  Differentiable with respect to
    `rotations` ALONE, through the quaternion's normalisation; which axis and whether it is flipped are held fixed, scales and means receive
    no gradient.  One streaming kernel each way.  The rasterizer takes a raw quaternion as given: for |q| != 1 this is the axis of the
    NORMALISED quaternion, not an eigenvector of the sheared covariance.  A cov3D_precomp caller has no axes: both tensors are required."""
    if not torch.is_tensor(means3D):
        raise TypeError("means3D must be a tensor [P, 3]")
    if means3D.shape[0] > 0 and not (_given(rotations) and _given(scales)):
        raise ValueError("gaussian_normals needs scales and rotations: a cov3D_precomp caller has no axes")
    for t, name, cols in ((rotations, "rotations", 4), (scales, "scales", 3)):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor [P, {cols}]")
    device = means3D.device
    if device.type != "cuda":
        raise RuntimeError("das3r_amd rasterizer: tensors must live on a HIP device (torch device 'cuda'); there is no CPU path")
    P = means3D.shape[0]
    for t, name, cols in ((rotations, "rotations", 4), (scales, "scales", 3), (means3D, "means3D", 3)):
        if t.dim() != 2 or tuple(t.shape) != (P, cols):
            raise ValueError(f"{name} must have dimensions ({P}, {cols}), got {tuple(t.shape)}")
    rotations, scales, means3D = (_prep(t, device, n) for t, n in ((rotations, "rotations"), (scales, "scales"), (means3D, "means3D")))
    if rotations.requires_grad and torch.is_grad_enabled():
        return _GaussianNormals.apply(rotations, scales.detach(), means3D.detach(), raster_settings)
    return _gaussian_normals_forward(raster_settings, rotations.detach(), scales.detach(), means3D.detach())[0]


def _plane(t, H, W, name):
    """[H, W] or [1, H, W] fp32 on a HIP device -> the dense [H, W] tensor the library reads"""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor [H, W] or [1, H, W]")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if tuple(t.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"{name} must have dimensions ({H}, {W}) or (1, {H}, {W}), got {tuple(t.shape)}")
    return t.reshape(H, W).contiguous()


def _image_call(name, rs, *rest):
    H, W = int(rs.image_height), int(rs.image_width)
    device = rest[0].device
    with _on_device(device):
        rc = getattr(_lib.load(), name)(H, W, float(rs.tanfovx), float(rs.tanfovy), *(_ptr(t) for t in rest), _stream(device))
    _lib.check(rc, name)


def _check_image_inputs(depth, rs, normal=None, alpha=None, mask=None):
    """-> (depth, normal, alpha, mask) as dense fp32 [H, W] / [3, H, W] tensors on depth's device; everything else is refused here."""
    H, W = int(rs.image_height), int(rs.image_width)
    if H <= 0 or W <= 0:
        raise ValueError(f"raster_settings describes a {W} x {H} image")
    d = _plane(depth, H, W, "depth")
    n = a = m = None
    if normal is not None:
        if not torch.is_tensor(normal) or normal.dtype != torch.float32 or tuple(normal.shape) != (3, H, W):
            raise ValueError(f"normal must be a float32 tensor of dimensions (3, {H}, {W})")
        n = normal.contiguous()
    if alpha is not None:
        a = _plane(alpha, H, W, "alpha")
    if mask is not None:
        m = _plane(mask.detach() if torch.is_tensor(mask) else mask, H, W, "mask")
    if d.device.type != "cuda":
        raise RuntimeError("das3r_amd rasterizer: tensors must live on a HIP device (torch device 'cuda'); there is no CPU path")
    for t, name in ((n, "normal"), (a, "alpha"), (m, "mask")):
        if t is not None and t.device != d.device:
            raise RuntimeError(f"{name} is on {t.device}, depth on {d.device}")
    return d, n, a, m


def depth_normals(depth, raster_settings):
    """depth [H, W] or [1, H, W] (view-space z) -> [3, H, W]: the unit normal of the depth surface, facing the camera (a fronto-parallel plane
    gives (0, 0, -1)), from central differences of the unprojected points p = z ray, ray through the pixel centres with raster_settings'
    tanfovx / tanfovy (include/das3r_raster.h das3r_normal_consistency_forward).  Exactly 0 on the one-pixel border, where the pixel or one
    of its four neighbours has no finite depth > 0, and where the surface element degenerates.  A plain tensor; normal_consistency is the
    differentiable use of it."""
    d, _, _, _ = _check_image_inputs(depth, raster_settings)
    H, W = d.shape
    out = torch.empty(3, H, W, dtype=torch.float32, device=d.device)   # fully written by the call
    zero = torch.zeros(4, H, W, dtype=torch.float32, device=d.device)   # (the entry takes a blended normal and a coverage: none here)
    _image_call("das3r_normal_consistency_forward", raster_settings, d.detach(), zero[:3], zero[3], None, torch.empty_like(d), out)
    return out


def _normal_consistency_forward(depth, normal, alpha, mask, rs):
    """One das3r_normal_consistency_forward call on dense tensors -> the loss image [H, W]."""
    loss = torch.empty_like(depth)   # fully written by the call
    _image_call("das3r_normal_consistency_forward", rs, depth, normal, alpha, mask, loss, None)
    return loss


class _NormalConsistency(torch.autograd.Function):
    """normal_consistency with its backward: ONE das3r_normal_consistency_backward call for the three gradients."""
    @staticmethod
    def forward(ctx, depth, normal, alpha, mask, raster_settings):
        loss = _normal_consistency_forward(depth, normal, alpha, mask, raster_settings)
        ctx.raster_settings, ctx.has_mask = raster_settings, mask is not None
        ctx.save_for_backward(depth, normal, *(() if mask is None else (mask,)))
        return loss

    @staticmethod
    def backward(ctx, grad):
        depth, normal = ctx.saved_tensors[:2]
        mask = ctx.saved_tensors[2] if ctx.has_mask else None
        g_depth, g_normal, g_alpha = torch.empty_like(depth), torch.empty_like(normal), torch.empty_like(depth)   # each fully written
        _image_call("das3r_normal_consistency_backward", ctx.raster_settings, depth, normal, mask, _dense(grad), g_depth, g_normal, g_alpha)
        return g_depth, g_normal, g_alpha, None, None


def normal_consistency(depth, normal, alpha, raster_settings, mask=None):
    """-> [1, H, W]: the normal-consistency loss image (2DGS's normal term) — per pixel mask * (alpha - normal . N_d), N_d = depth_normals(depth,
    raster_settings).  With normal = sum_k w_k n_k (the Gaussians' normals blended over a forward's lists) and alpha = sum_k w_k (its coverage)
    this is sum_k w_k (1 - n_k . N_d).  depth, alpha: [H, W] or [1, H, W]; normal: [3, H, W]; mask: [H, W] or [1, H, W], a constant, or None
    (ones).  Exactly 0 wherever N_d is (depth_normals), and such a pixel sends exactly 0 to every gradient whatever its depth holds.
    Differentiable with respect to depth, normal and alpha (das3r_normal_consistency_backward: dL/dalpha = g m, dL/dnormal = -g m N_d,
    dL/ddepth gathered from the four neighbours whose stencils read the pixel).  No floating-point atomics: bit-identical from run to run."""
    d, n, a, m = _check_image_inputs(depth, raster_settings, normal, alpha, mask)
    if n is None or a is None:
        raise TypeError("normal_consistency needs the blended normal [3, H, W] and the coverage [H, W]")
    H, W = d.shape
    if torch.is_grad_enabled() and (d.requires_grad or n.requires_grad or a.requires_grad):
        return _NormalConsistency.apply(d, n, a, m, raster_settings).reshape(1, H, W)
    return _normal_consistency_forward(d.detach(), n.detach(), a.detach(), m, raster_settings).reshape(1, H, W)


# ---- the rasterising autograd function and the module


class _Options:
    """What one application of _RasterizeGaussians is asked for besides upstream's nine inputs — invdepth: the inverse-depth image as a third
    output; antialiasing: upstream's 2D mip filter (the settings tuple keeps upstream's twelve fields); no_backward: no backward pass can
    follow (evaluation); want_state: the caller keeps the forward's state beyond the call — and, written by the function's forward, `state`:
    the RasterState it left."""
    __slots__ = ("invdepth", "antialiasing", "no_backward", "want_state", "state")

    def __init__(self, invdepth=False, antialiasing=False, no_backward=False, want_state=False):
        self.invdepth, self.antialiasing, self.no_backward, self.want_state = bool(invdepth), bool(antialiasing), bool(no_backward), bool(want_state)
        self.state = None


def _check_log_focal(log_focal, device):
    if not torch.is_tensor(log_focal) or log_focal.numel() != 2 or log_focal.dtype != torch.float32:
        raise ValueError("log_focal must be a float32 tensor of 2 elements (log-focal offsets in x and y)")
    if log_focal.device != device:
        raise RuntimeError(f"log_focal is on {log_focal.device}, expected {device}")
    return log_focal


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, antialiasing=False,
                        log_focal=None, options=None):
    """-> (color, radii), or (color, radii, invdepth) when options.invdepth.  log_focal ([2] tensor or None): see GaussianRasterizer.forward's
    docstring.  options: an _Options with invdepth / want_state set; antialiasing and no_backward are set here, its `state` by the forward.
    no_backward: under torch.no_grad, or when no input takes a gradient (inside the autograd function's forward grad mode is always off,
    and needs_input_grad ignores it)."""
    if options is None:
        options = _Options()
    if log_focal is not None:
        _check_log_focal(log_focal, means3D.device)
    options.antialiasing = bool(antialiasing)
    options.no_backward = not (torch.is_grad_enabled() and any(
        torch.is_tensor(t) and t.requires_grad for t in (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, log_focal)))
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, options,
                                     log_focal)


class _RasterizeGaussians(torch.autograd.Function):
    """The rasterising function: upstream's nine inputs, then optionally an _Options (None: the defaults — upstream's own nine-argument
    apply) and log_focal ([2] tensor or None: its value is not read, like the dummy means2D — the caller built raster_settings from the same
    field of view; when it takes a gradient the backward is das3r_raster_backward_focal and returns dL/d(log-focal offsets) for it).
    -> (color, radii) or, with options.invdepth, (color, radii, invdepth): a backward that receives no gradient for the inverse depth is the
    das3r_raster_backward call, otherwise das3r_raster_backward_depth takes both."""
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, options=None,
                log_focal=None):
        if options is None:
            options = _Options()
        device = means3D.device
        means3D = _prep(means3D, device, "means3D")
        sh = _prep(sh, device, "shs")
        colors_precomp = _prep(colors_precomp, device, "colors_precomp")
        opacities = _prep(opacities, device, "opacities")
        scales = _prep(scales, device, "scales")
        rotations = _prep(rotations, device, "rotations")
        cov3Ds_precomp = _prep(cov3Ds_precomp, device, "cov3D_precomp")
        args = (raster_settings, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        cpu_args = cpu_deep_copy_tuple(args) if raster_settings.debug else None   # copy them before they can be corrupted
        try:   # (the backward learns of the antialiasing from the forward's flags: the state's capacity)
            state, color, radii, invdepth = _forward(*args, invdepth=options.invdepth, no_backward=options.no_backward,
                                                     antialiasing=options.antialiasing)
        except Exception:
            if cpu_args is not None:
                torch.save(cpu_args, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise
        options.state = state   # (GaussianRasterizer.forward: a render that no backward pass will follow checks itself; the aux-channel calls)
        ctx.raster_settings, ctx.num_rendered, ctx.capacity = raster_settings, state.num_rendered, state.capacity
        ctx.focal_shape = None if log_focal is None else log_focal.shape
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities, state.geom, state.binning,
                              state.img)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)   # no zero-filled 'gradient' for radii on every backward (a fill kernel per step)
        return (color, radii, invdepth) if options.invdepth else (color, radii)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_invdepth=None):
        rs = ctx.raster_settings
        n = len(ctx.needs_input_grad)   # (as many as the inputs actually given: 9, 10 or 11)
        if grad_out_color is None and grad_invdepth is None:   # (grads are not materialised) nothing flows back
            return (None,) * n
        focal = n > 10 and ctx.needs_input_grad[10]
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities, geomBuffer, binningBuffer,
         imgBuffer) = ctx.saved_tensors
        state = RasterState(geomBuffer, binningBuffer, imgBuffer, ctx.num_rendered, ctx.capacity, means3D.shape[0], rs.image_width,
                            rs.image_height, means3D.device)
        inputs = (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        cpu_args = None
        if rs.debug:
            cpu_args = cpu_deep_copy_tuple((rs, ctx.num_rendered, grad_out_color) + inputs + (geomBuffer, binningBuffer, imgBuffer, ctx.capacity))
        try:
            out = _backward(state, rs, grad_out_color, *inputs, grad_invdepth=grad_invdepth, focal=focal)
        except Exception:
            if cpu_args is not None:
                torch.save(cpu_args, "snapshot_bw.dump")
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
            raise
        g_means2D, g_colors, g_opac, g_means3D, g_cov, g_sh, g_scales, g_rot = out[:8]
        g_focal = out[8].reshape(ctx.focal_shape) if focal else None
        return (g_means3D, g_means2D, g_sh if sh.numel() else None, g_colors if colors_precomp.numel() else None, g_opac,
                g_scales if scales.numel() else None, g_rot if rotations.numel() else None,
                g_cov if cov3Ds_precomp.numel() else None, None, None, g_focal)[:n]


# The one hand-over that upstream's fixed `forward` signature forces: GaussianRasterizer.__call__ passes its two extra keywords (log_focal,
# aux_geometry_grad) to GaussianRasterizer.forward through this thread-local, and forward consumes them.  Nothing else in this module reads
# or writes module-level per-call state: options travel as arguments (_Options), results as return values (RasterState).
_last = threading.local()


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings, keep_state=False):
        """keep_state: every forward leaves its `RasterState` in `self.state` (composite_features / feature_adjoint / alpha_of)."""
        super().__init__()
        self.raster_settings = raster_settings
        self.keep_state = bool(keep_state)
        self.state = None

    def __call__(self, *args, log_focal=None, aux_geometry_grad=False, **kwargs):
        """The module call takes two keywords more than forward(): log_focal and aux_geometry_grad (forward's docstring).  None / False:
        nn.Module's call, as it was."""
        if log_focal is None and not aux_geometry_grad:
            return super().__call__(*args, **kwargs)
        _last.log_focal, _last.aux_geometry_grad = log_focal, bool(aux_geometry_grad)
        try:
            return super().__call__(*args, **kwargs)
        finally:
            _last.log_focal, _last.aux_geometry_grad = None, False

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            device = positions.device
            if device.type != "cuda":
                raise RuntimeError("das3r_amd rasterizer: positions must live on a HIP device; there is no CPU path")
            pos = _prep(positions, device, "positions")
            P = pos.shape[0]
            present = torch.zeros(P, dtype=torch.uint8, device=device)
            if P:
                vm = _small(rs.viewmatrix, device, 16, "viewmatrix")
                pm = _small(rs.projmatrix, device, 16, "projmatrix")
                with _on_device(device):
                    rc = _lib.load().das3r_mark_visible(P, _ptr(pos), _ptr(vm), _ptr(pm), _ptr(present), _stream(device))
                _lib.check(rc, "das3r_mark_visible")
            return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, return_invdepth=False, antialiasing=False, features=None, return_alpha=False):
        """-> (color [3, H, W], radii [P]); with return_invdepth, (color, radii, invdepth [1, H, W]) as upstream's newer rasterizer returns:
        per pixel sum_i (1/z_i) alpha_i T_i over the splats the colour is blended from, 0 where nothing is (no background term).  The
        colour and radii are the same bit for bit either way.  The inverse depth is differentiable (back to means3D, scales, rotations,
        opacities and means2D through alpha, and to means3D through 1/z).
        antialiasing: upstream's antialiasing mode (its 2D mip filter) — every splat is blended with its opacity times
        sqrt(max(det(Sigma2D) / det(Sigma2D + 0.3 I), 2.5e-5)), and the backward differentiates that factor too.  Radii are unchanged.
        features ([P, C] fp32) / return_alpha: the extra results come after the others — (color, radii[, invdepth][, feature_image]
        [, alpha]) — feature_image [C, H, W] = composite_features over this forward's lists (differentiable with respect to `features`
        only, unless aux_geometry_grad — below), alpha [1, H, W] = alpha_of.  The colour, the radii and every gradient of a
        colour loss are the same bit for bit; with both at their defaults the call is the one it was.
        log_focal ([2] fp32 tensor; a keyword of the module CALL — rasterizer(..., log_focal=t), see __call__ — so that this method keeps the
        parameters it had): log-focal offsets (s_x, s_y) of the camera, e.g. (-log tan(FoVx / 2), -log tan(FoVy / 2)).  Like the
        dummy means2D its VALUE is not read — raster_settings (tanfov, projmatrix) must have been built from the same field of view.  When
        it requires grad the backward pass returns dL/ds for it (das3r_raster_backward_focal: the rendering with tanfov e^(-s) and the
        clip-x / clip-y columns of projmatrix scaled by e^(s), every discrete decision held fixed), with and without return_invdepth /
        antialiasing; every other gradient is the same bit for bit.  None: the library calls are the ones they were.
        aux_geometry_grad (bool; like log_focal a keyword of the module CALL — rasterizer(..., features=f, aux_geometry_grad=True)): False,
        the default: the library calls are the ones they were, a loss on feature_image reaches `features` alone and alpha
        carries no gradient.  True (needs features and / or return_alpha): feature_image and alpha are differentiable with respect to
        means3D, opacities, scales, rotations / cov3D_precomp as well, and their dL/dmean2D is added to means2D.grad beside the colour
        loss's — one das3r_raster_aux_backward call for both images (a compositing kernel over this forward's saved lists + the per-Gaussian
        backward; no second forward).  The colour, radii and colour-loss gradients are the same bit for bit.  For a coverage / mask loss ask
        for return_alpha; a column of ones in `features` has the same derivative on paper and a poorly conditioned one in fp32."""
        raster_settings = self.raster_settings
        log_focal, _last.log_focal = getattr(_last, "log_focal", None), None   # (handed over by __call__; consumed here)
        aux_geometry_grad, _last.aux_geometry_grad = getattr(_last, "aux_geometry_grad", False), False
        if aux_geometry_grad and features is None and not return_alpha:
            raise ValueError("aux_geometry_grad=True needs features= and / or return_alpha=True: there is no aux image to differentiate")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        # upstream: torch.Tensor([]) placeholders
        shs, colors_precomp, scales, rotations, cov3D_precomp = _or_empty(means3D.device, shs, colors_precomp, scales, rotations, cov3D_precomp)
        want_state = features is not None or return_alpha or self.keep_state
        options = _Options(invdepth=return_invdepth, want_state=want_state)
        out = rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, raster_settings,
                                  antialiasing=antialiasing, options=options, **({} if log_focal is None else {"log_focal": log_focal}))
        state = options.state
        if state is not None and not out[0].requires_grad:
            # evaluation (torch.no_grad, or no input that takes a gradient): no backward pass will examine this forward's binning
            # self-check, so it is examined here, before the image is used (include/das3r_raster.h: das3r_raster_check)
            state.check()
        if want_state:
            self.state = state
            if aux_geometry_grad:
                geometry = AuxGeometry(raster_settings, means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp)
                fimg, alpha = _aux_with_geometry(state, features, geometry, return_alpha)
                return out + (() if features is None else (fimg,)) + ((alpha,) if return_alpha else ())
            if features is not None:
                out = out + (composite_features(state, features),)
            if return_alpha:
                out = out + (alpha_of(state),)
        return out
