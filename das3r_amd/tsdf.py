"""TSDF fusion of rendered depth into a voxel grid, and a triangle mesh out of it (opt-in): the last step of the 2DGS recipe.

The per-view surface depths — rasterizer.median_depth_of over a render's own lists — are fused into ONE truncated signed distance field,
and a mesh with normals and colours is taken from it by marching tetrahedra (no 256-case table; the split of every cube into the six Kuhn
tetrahedra has the same face diagonals in neighbouring cubes, so the surface closes).  include/das3r_raster.h has the rule in full:

    grid      dims = (nx, ny, nz), origin = the corner of voxel (0, 0, 0), edge `voxel`; centres at origin + (i + 1/2, j + 1/2, k + 1/2) voxel;
              dense fp32 tsdf [nz, ny, nx], weight [nz, ny, nx], colour [3, nz, ny, nx]; fresh: tsdf 1, weight 0, colour 0
    per view  camera-space point (skip unless z > near) -> pixel (skip outside) -> d = depth, w = weight (skip unless > 0 and finite) ->
              sdf = d - z (skip below -trunc), ts = min(1, sdf / trunc) -> the running weighted mean of ts and of the colour

Two forms of the integration: csrc/tsdf.hip (one launch per batch of views: the grid is read and written once) for dense fp32 tensors on a
HIP device, and integrate_torch — plain torch on any device, the DEFINITION: it fixes the operation order (sums left to right, where the
quotients are taken, no fused multiply-adds) and the kernel mirrors it operation for operation.  The extraction needs a HIP device."""
import ctypes as C

import torch

from . import _lib


def _views(viewmatrix, tanfovx, tanfovy, V):
    vm = torch.as_tensor(viewmatrix, dtype=torch.float32).reshape(-1, 16)
    if vm.shape[0] != V:
        raise ValueError(f"tsdf: {vm.shape[0]} view matrices for {V} depth images")
    one = lambda t: [float(torch.tensor(float(x), dtype=torch.float32)) for x in (t.reshape(-1).tolist() if torch.is_tensor(t) else
                                                                                  (list(t) if hasattr(t, "__len__") else [t] * V))]
    tx, ty = one(tanfovx), one(tanfovy)
    if len(tx) != V or len(ty) != V:
        raise ValueError("tsdf: tanfovx / tanfovy need one value per view (or one for all)")
    for t in tx + ty:
        if not (t > 0.0) or t == float("inf"):
            raise ValueError(f"tsdf: tanfovx / tanfovy must be finite and > 0, got {t!r}")
    return vm, tx, ty


def _check_scalars(voxel, trunc):
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
    voxel, trunc = f32(voxel), f32(trunc)
    for name, v in (("voxel", voxel), ("trunc", trunc)):
        if not (v > 0.0) or v == float("inf"):
            raise ValueError(f"tsdf: {name} must be finite and > 0, got {v!r}")
    return voxel, trunc


def voxel_centres(dims, origin, voxel, device="cpu"):
    """-> X [nx], Y [ny], Z [nz] fp32: origin + (index + 1/2) * voxel, the product first"""
    o = [float(torch.tensor(float(x), dtype=torch.float32)) for x in origin]
    ax = lambda n, o_: (torch.arange(int(n), dtype=torch.float32, device=device) + 0.5) * float(voxel) + o_
    return ax(dims[0], o[0]), ax(dims[1], o[1]), ax(dims[2], o[2])


@torch.no_grad()
def integrate_torch(tsdf, weight, colour, dims, origin, voxel, depth, viewmatrix, tanfovx, tanfovy, colour_img=None, weight_img=None, trunc=None,
                    near=0.01):
    """The rule in torch ops -> (tsdf, weight, colour) as NEW fp32 tensors on tsdf's device (colour None without a colour grid).
    tsdf, weight [nz, ny, nx], colour [3, nz, ny, nx] or None; depth [V, H, W]; viewmatrix [V, 16] (or [V, 4, 4]) in the rasterizer's layout;
    tanfovx / tanfovy: a number or V numbers; colour_img [V, 3, H, W] iff colour; weight_img [V, H, W] or None."""
    if (colour is None) != (colour_img is None):
        raise ValueError("integrate_torch: a colour image needs a colour grid and a colour grid needs a colour image")
    voxel, trunc = _check_scalars(voxel, trunc)
    dev = tsdf.device
    depth = depth.detach().to(device=dev, dtype=torch.float32)
    V, H, W = depth.shape
    vm, tx, ty = _views(viewmatrix, tanfovx, tanfovy, V)
    m_all = vm.tolist()
    x, y, z = voxel_centres(dims, origin, voxel, dev)
    X, Y, Z = x[None, None, :], y[None, :, None], z[:, None, None]
    T, Wt = tsdf.detach().float().clone(), weight.detach().float().clone()
    Cs = None if colour is None else [colour[c].detach().float().clone() for c in range(3)]
    near = float(torch.tensor(float(near), dtype=torch.float32))
    one = torch.ones((), dtype=torch.float32, device=dev)
    for v in range(V):
        m = m_all[v]
        xc = m[0] * X + m[4] * Y + m[8] * Z + m[12]
        yc = m[1] * X + m[5] * Y + m[9] * Z + m[13]
        zc = m[2] * X + m[6] * Y + m[10] * Z + m[14]
        ok = zc > near
        u = ((xc / zc) / tx[v] + 1.0) * (0.5 * W)
        w_ = ((yc / zc) / ty[v] + 1.0) * (0.5 * H)
        ok = ok & (u >= 0.0) & (u < float(W)) & (w_ >= 0.0) & (w_ < float(H))
        zero = torch.zeros_like(u)
        px = torch.floor(torch.where(ok, u, zero)).to(torch.int64).clamp_(0, W - 1)
        py = torch.floor(torch.where(ok, w_, zero)).to(torch.int64).clamp_(0, H - 1)
        pix = py * W + px
        d = depth[v].reshape(-1)[pix]
        ok = ok & (d > 0.0) & torch.isfinite(d)
        if weight_img is None:
            w = torch.ones_like(d)
        else:
            w = weight_img[v].detach().to(device=dev, dtype=torch.float32).reshape(-1)[pix]
            ok = ok & (w > 0.0) & torch.isfinite(w)
        sdf = d - zc
        ok = ok & ~(sdf < -trunc)
        ts = torch.minimum(one, sdf / trunc)
        Wn = Wt + w
        T = torch.where(ok, (T * Wt + ts * w) / Wn, T)
        if Cs is not None:
            img = colour_img[v].detach().to(device=dev, dtype=torch.float32).reshape(3, -1)
            Cs = [torch.where(ok, (Cs[c] * Wt + img[c][pix] * w) / Wn, Cs[c]) for c in range(3)]
        Wt = torch.where(ok, Wn, Wt)
    return T, Wt, (None if Cs is None else torch.stack(Cs, 0))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _dense(*tensors):
    return all(t is None or (t.device.type == "cuda" and t.dtype == torch.float32 and t.is_contiguous()) for t in tensors)


@torch.no_grad()
def integrate_kernels(tsdf, weight, colour, dims, origin, voxel, depth, viewmatrix, tanfovx, tanfovy, colour_img=None, weight_img=None, trunc=None,
                      near=0.01):
    """das3r_tsdf_integrate: the grid tensors are updated IN PLACE.  Dense fp32 tensors on one HIP device; nothing is read back."""
    lib = _lib.load()
    dev = tsdf.device
    V, H, W = (int(s) for s in depth.shape)
    vm, tx, ty = _views(viewmatrix, tanfovx, tanfovy, V)
    vm = vm.to(dev).contiguous()
    if not _dense(tsdf, weight, colour, depth, colour_img, weight_img):
        raise RuntimeError("das3r_amd.tsdf: the kernel takes dense fp32 tensors on a HIP device (the torch form is tsdf.integrate_torch)")
    nx, ny, nz = (int(d) for d in dims)
    if tuple(tsdf.shape) != (nz, ny, nx) or tuple(weight.shape) != (nz, ny, nx) or (colour is not None and tuple(colour.shape) != (3, nz, ny, nx)):
        raise ValueError("das3r_amd.tsdf: tsdf / weight must be [nz, ny, nx] and colour [3, nz, ny, nx]")
    if (colour_img is not None and tuple(colour_img.shape) != (V, 3, H, W)) or (weight_img is not None and tuple(weight_img.shape) != (V, H, W)):
        raise ValueError("das3r_amd.tsdf: colour_img must be [V, 3, H, W] and weight_img [V, H, W]")
    from .rasterizer import _on_device
    with _on_device(dev):
        rc = lib.das3r_tsdf_integrate((C.c_int32 * 3)(nx, ny, nz), (C.c_float * 3)(*[float(o) for o in origin]), C.c_float(voxel), _ptr(tsdf),
                                      _ptr(weight), _ptr(colour), V, _ptr(vm), (C.c_float * max(V, 1))(*tx), (C.c_float * max(V, 1))(*ty), H, W,
                                      _ptr(depth), _ptr(colour_img), _ptr(weight_img), C.c_float(trunc), C.c_float(near),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "das3r_tsdf_integrate")


class TSDFGrid:
    """A dense TSDF grid.  origin: the corner of voxel (0, 0, 0), world units; voxel: the edge; dims = (nx, ny, nz); colour: keep a colour
    per voxel.  .tsdf / .weight [nz, ny, nx], .colour [3, nz, ny, nx] or None, fp32 on `device`."""

    def __init__(self, origin, voxel, dims, device="cuda", colour=True):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError(f"TSDFGrid: dims must be three sizes >= 1, got {dims!r}")
        if self.dims[0] * self.dims[1] * self.dims[2] > _lib.TSDF_MAX_VOXELS:
            raise ValueError(f"TSDFGrid: {self.dims} is more than 2^28 voxels")
        self.voxel = _check_scalars(voxel, 1.0)[0]
        self.origin = tuple(float(torch.tensor(float(o), dtype=torch.float32)) for o in origin)
        self.device = torch.device(device)
        nx, ny, nz = self.dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=self.device)
        self.colour = torch.zeros(3, nz, ny, nx, dtype=torch.float32, device=self.device) if colour else None
        self.trunc = None   # the last integrate's

    @torch.no_grad()
    def integrate(self, depth, viewmatrix, tanfovx, tanfovy, colour=None, weight=None, trunc=None, near=0.01, use_kernels=None):
        """Fuse V views.  depth [V, H, W] (or [H, W] / [1, H, W] for one): view-space z, 0 where there is nothing; viewmatrix [V, 16] in the
        rasterizer's layout; colour [V, 3, H, W] (required iff the grid has colour); weight [V, H, W] or None; trunc: world units, default
        4 voxels.  use_kernels: None = the HIP kernel for a grid on a HIP device, else torch; False = torch; True = the kernel or an error
        (prune_points' convention)."""
        dev = self.device
        prep = lambda t, nd: None if t is None else t.detach().to(device=dev, dtype=torch.float32).reshape((-1,) + tuple(t.shape[-nd:])).contiguous()
        depth, colour, weight = prep(depth, 2), prep(colour, 3), prep(weight, 2)
        if (colour is None) != (self.colour is None):
            raise ValueError("TSDFGrid.integrate: a colour image is required iff the grid has colour")
        trunc = 4.0 * self.voxel if trunc is None else trunc
        _, trunc = _check_scalars(self.voxel, trunc)
        self.trunc = trunc
        on_hip = dev.type == "cuda"
        if use_kernels and not on_hip:
            raise RuntimeError("TSDFGrid.integrate(use_kernels=True): the grid is not on a HIP device")
        args = (self.dims, self.origin, self.voxel, depth, viewmatrix, tanfovx, tanfovy, colour, weight, trunc, near)
        if on_hip if use_kernels is None else bool(use_kernels):
            integrate_kernels(self.tsdf, self.weight, self.colour, *args)
        else:
            self.tsdf, self.weight, self.colour = integrate_torch(self.tsdf, self.weight, self.colour, *args)
        return self

    @torch.no_grad()
    def extract(self):
        """The mesh -> dict(vertices [Nv, 3], normals [Nv, 3], colours [Nv, 3] or None, faces [Nf, 3] int32, edge_mask [nz, ny, nx] uint8: the
        owned edges of every voxel that carry a vertex, bit = type) as device tensors.  One host read: (Nv, Nf)."""
        return extract_kernels(self.tsdf, self.weight, self.colour, self.dims, self.origin, self.voxel)

    def box(self):
        """-> (lo, hi): the grid's corners in world units"""
        return self.origin, tuple(o + n * self.voxel for o, n in zip(self.origin, self.dims))


@torch.no_grad()
def extract_kernels(tsdf, weight, colour, dims, origin, voxel):
    """das3r_tsdf_extract_count + _emit over given grid tensors (dense fp32 on a HIP device): TSDFGrid.extract's dict."""
    lib = _lib.load()
    if not _dense(tsdf, weight, colour):
        raise RuntimeError("das3r_amd.tsdf: the extraction takes dense fp32 tensors on a HIP device")
    dev = tsdf.device
    nx, ny, nz = (int(d) for d in dims)
    if tuple(tsdf.shape) != (nz, ny, nx) or tuple(weight.shape) != (nz, ny, nx) or (colour is not None and tuple(colour.shape) != (3, nz, ny, nx)):
        raise ValueError("das3r_amd.tsdf: tsdf / weight must be [nz, ny, nx] and colour [3, nz, ny, nx]")
    cdims, corigin = (C.c_int32 * 3)(nx, ny, nz), (C.c_float * 3)(*[float(o) for o in origin])
    nbytes = int(lib.das3r_tsdf_extract_workspace_bytes(cdims))
    if nbytes == 0:
        raise ValueError(f"das3r_amd.tsdf: dims {dims} are refused (each >= 1, at most 2^28 voxels)")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    from .rasterizer import _on_device
    with _on_device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.das3r_tsdf_extract_count(cdims, _ptr(tsdf), _ptr(weight), _ptr(ws), _ptr(totals), stream), "das3r_tsdf_extract_count")
        Nv, Nf = (int(v) for v in totals.tolist())
        vertices = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
        normals = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
        colours = torch.empty(Nv, 3, dtype=torch.float32, device=dev) if colour is not None else None
        faces = torch.empty(Nf, 3, dtype=torch.int32, device=dev)
        if Nv or Nf:
            _lib.check(lib.das3r_tsdf_extract_emit(cdims, corigin, C.c_float(voxel), _ptr(tsdf), _ptr(weight), _ptr(colour), _ptr(ws), Nv, Nf,
                                                   _ptr(vertices), _ptr(normals), _ptr(colours) if Nv else None, _ptr(faces), stream),
                       "das3r_tsdf_extract_emit")
    edge_mask = (ws[:nx * ny * nz] & 0x7F).to(torch.uint8).reshape(nz, ny, nx)
    return dict(vertices=vertices, normals=normals, colours=colours, faces=faces, edge_mask=edge_mask)


@torch.no_grad()
def bounds_from_points(xyz, quantile=0.01):
    """A box from a model's centres -> (lo, hi), two 3-tuples: per axis the `quantile` and 1 - `quantile` order statistics (0: the full
    extent), so that a few far floaters do not decide the grid."""
    p = xyz.detach().reshape(-1, 3).float()
    p = p[torch.isfinite(p).all(dim=1)]
    if p.shape[0] == 0:
        raise ValueError("bounds_from_points: no finite point")
    if not (0.0 <= float(quantile) < 0.5):
        raise ValueError("bounds_from_points: quantile must be in [0, 0.5)")
    n = p.shape[0]
    k = min(int(float(quantile) * n), (n - 1) // 2)
    s = p.sort(dim=0).values
    return tuple(float(v) for v in s[k]), tuple(float(v) for v in s[n - 1 - k])


def grid_for_box(lo, hi, voxel, pad=2):
    """-> (origin, dims): the grid of edge `voxel` that covers the box [lo, hi] with `pad` voxels around it"""
    voxel = float(voxel)
    origin = tuple(float(l) - pad * voxel for l in lo)
    dims = tuple(max(1, int(-(-(float(h) + pad * voxel - o) // voxel))) for h, o in zip(hi, origin))
    return origin, dims


def view_matrix_of(pose7):
    """(qw, qx, qy, qz, tx, ty, tz) world-to-camera -> the 16 floats das3r_tsdf_integrate takes (the rasterizer's layout: the transpose)"""
    from .camera import camera_from_tensor
    return camera_from_tensor(pose7.detach().float()).T.contiguous().reshape(16)


@torch.no_grad()
def fuse_views(model, views, pipe, background, grid, depth="median", min_alpha=0.5, static_weight=False, trunc=None, near=0.01, use_kernels=None):
    """Fuse the model's own renders of `views` into `grid`.  Per view: one no-grad das3r_render that keeps its state; the median depth
    (rasterizer.median_depth_of) or, depth="blended", 1 / the inverse-depth image, from that render's lists; pixels whose coverage
    (rasterizer.alpha_of) is below min_alpha get depth 0; static_weight: the static-confidence map (the per-Gaussian conf_static blended over
    the same lists) is the weight image; then grid.integrate.  views, the pose and the variant: prune.surface_scores'.  -> grid"""
    import math
    from types import SimpleNamespace
    from .rasterizer import alpha_of, composite_features, median_depth_of
    from .render import das3r_render
    if depth not in ("median", "blended"):
        raise ValueError(f'fuse_views: depth must be "median" or "blended", got {depth!r}')
    pipe = pipe or SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    dev = model._xyz.device
    background = background if background is not None else torch.zeros(3, device=dev)
    variant = "render" if hasattr(model, "aggregated_mask") else "test"
    conf = None
    if static_weight:
        conf = model._conf_static.detach().reshape(-1).float()
        if hasattr(model, "aggregated_mask"):
            from .prune import mask_index
            conf = conf[mask_index(model)]
        conf = conf.reshape(-1, 1).contiguous()
    for view in views:
        pose = getattr(view, "pose7", None)
        pose = model.get_RT(view.uid) if pose is None else pose
        pkg = das3r_render(view, model, pipe, background, camera_pose=pose, variant=variant, return_state=True,
                           **({"return_invdepth": True} if depth == "blended" else {}))
        state = pkg["raster_state"]
        if depth == "median":
            z = median_depth_of(state)[0]
        else:
            inv = pkg["invdepth"][0]
            z = torch.where(inv > 0, 1.0 / inv.clamp_min(1e-30), torch.zeros_like(inv))
        z = torch.where(alpha_of(state)[0] >= float(min_alpha), z, torch.zeros_like(z))
        w = composite_features(state, conf)[0] if static_weight else None
        grid.integrate(z[None], view_matrix_of(pose)[None], math.tan(float(view.FoVx) * 0.5), math.tan(float(view.FoVy) * 0.5),
                       colour=pkg["render"].detach().clamp(0.0, 1.0)[None] if grid.colour is not None else None,
                       weight=None if w is None else w[None], trunc=trunc, near=near, use_kernels=use_kernels)
    return grid
