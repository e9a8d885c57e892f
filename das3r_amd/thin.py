"""Voxel thinning (opt-in): one Gaussian per cell of a voxel grid, told how many it stands for.

DAS3R creates one Gaussian per confident pixel of every training frame (SplatModel.create_from_frames), so a static surface seen in F frames
starts as about F coincident Gaussians of opacity 1/F — and the train step is paid per Gaussian.  Pruning (das3r_amd.prune) removes what has
become transparent; this removes the F-fold redundancy itself.  The rule (include/das3r_raster.h das3r_thin_voxels has it in full):

    cell      c_k = floor(xyz_k * inv_edge), one fp32 multiply per axis, inv_edge = fp32(1 / edge)
    placeable the three products finite and every c_k in [-2^20, 2^20); anything else never merges: kept, count 1
    winner    of a cell: the highest score; ties (-0 == +0) to the lower index; NaN loses to every number; no score: the lowest index
    keep      winners and points that are not placeable;  count: the cell's population at its winner, 1 at a point not placeable, 0 at a loser

Two forms, bit-identical: csrc/thin.hip (a hash table, no sort) for dense fp32 tensors on a HIP device, and voxel_keep_torch — plain torch on
any device, what the tests hold the kernels to and what runs off-device.  The surgery on a model is prune_points(also_drop=~keep)."""
import ctypes as C

import torch

from . import _lib

HALF = 1 << 20
OPACITY_MODES = ("coverage", "reference")
COVERAGE_MAX = 0.99


def inv_edge_of(edge):
    """fp32(1 / edge) as a Python float: the ONE value both forms multiply by."""
    edge = float(edge)
    if not (edge > 0.0) or edge == float("inf"):
        raise ValueError(f"thin: the voxel edge must be finite and > 0, got {edge!r}")
    inv = float(torch.tensor(1.0 / edge, dtype=torch.float64).to(torch.float32))
    if not (inv > 0.0) or inv == float("inf"):
        raise ValueError(f"thin: 1 / edge is not a positive finite fp32 number for edge {edge!r}")
    return inv


def _orderable(score):
    """fp32 scores -> int64 in [0, 2^32) with the kernels' total order: NaN (0) < -inf < ... < -0 = +0 < ... < +inf."""
    b = score.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    o = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
    return torch.where(torch.isnan(score), torch.zeros_like(o), o)


@torch.no_grad()
def voxel_keep_torch(xyz, score, inv_edge):
    """The rule in torch ops -> (keep bool [P], count int32 [P]).  xyz [P, 3] fp32, score [P] fp32 or None, inv_edge: inv_edge_of(edge)."""
    xyz = xyz.detach().reshape(-1, 3)
    if xyz.dtype != torch.float32:
        raise TypeError("voxel_keep_torch: xyz must be fp32 (the cell is an fp32 product)")
    dev, P = xyz.device, int(xyz.shape[0])
    keep = torch.ones(P, dtype=torch.bool, device=dev)
    count = torch.ones(P, dtype=torch.int32, device=dev)
    if P == 0:
        return keep, count
    prod = xyz * torch.tensor(float(inv_edge), dtype=torch.float32, device=dev)
    cell = torch.floor(prod)
    placeable = (torch.isfinite(prod) & (cell >= -float(HALF)) & (cell < float(HALF))).all(dim=1)
    idx = torch.nonzero(placeable, as_tuple=False).reshape(-1)
    if idx.numel() == 0:
        return keep, count
    c = cell[idx].to(torch.int64) + HALF
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, inv, pop = torch.unique(key, return_inverse=True, return_counts=True)
    if score is None:
        order = torch.zeros(idx.numel(), dtype=torch.int64, device=dev)
    else:
        s = score.detach().reshape(-1)
        if s.dtype != torch.float32 or s.numel() != P:
            raise TypeError("voxel_keep_torch: score must be fp32 with one entry per point")
        order = _orderable(s[idx])
    top = torch.zeros(pop.numel(), dtype=torch.int64, device=dev).scatter_reduce_(0, inv, order, "amax", include_self=False)
    cand = torch.where(order == top[inv], idx, torch.full_like(idx, P))
    winner = torch.full((pop.numel(),), P, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, cand, "amin", include_self=False)
    won = winner[inv] == idx
    keep[idx] = won
    count[idx] = torch.where(won, pop[inv], torch.zeros_like(pop[inv])).to(torch.int32)
    return keep, count


def _dense(xyz, score):
    return xyz.device.type == "cuda" and xyz.dtype == torch.float32 and xyz.is_contiguous() and \
        (score is None or (score.device == xyz.device and score.dtype == torch.float32 and score.is_contiguous()))


@torch.no_grad()
def voxel_keep_kernels(xyz, score, inv_edge):
    """das3r_thin_voxels -> (keep uint8 [P], count int32 [P], info int32 [2]) as device tensors; nothing is read back."""
    lib = _lib.load()
    dev = xyz.device
    if not _dense(xyz, score):
        raise RuntimeError("das3r_amd.thin: the kernels take dense fp32 tensors on a HIP device (the torch form is thin.voxel_keep_torch)")
    P = int(xyz.shape[0])
    if score is not None and score.numel() != P:
        raise ValueError("das3r_amd.thin: score needs one entry per point")
    keep = torch.empty(P, dtype=torch.uint8, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.das3r_thin_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    from .rasterizer import _on_device
    with _on_device(dev):
        rc = lib.das3r_thin_voxels(P, ptr(xyz), ptr(score), C.c_float(inv_edge), ptr(keep), ptr(count), C.c_void_p(info.data_ptr()), ptr(ws),
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "das3r_thin_voxels")
    return keep, count, info


@torch.no_grad()
def voxel_keep(xyz, score=None, edge=None, use_kernels=None):
    """-> (keep bool [P], count int32 [P], kept: int).  use_kernels: None = the HIP kernels for dense fp32 tensors on a HIP device, else torch;
    False = torch; True = the kernels or an error (prune_points' convention).  One host read: the kept count."""
    if edge is None:
        raise ValueError("voxel_keep: edge (the voxel's side in world units) is required")
    inv = inv_edge_of(edge)
    xyz = xyz.detach().reshape(-1, 3)
    score = None if score is None else score.detach().reshape(-1)
    dense = _dense(xyz, score)
    if use_kernels and not dense:
        raise RuntimeError("voxel_keep(use_kernels=True): dense fp32 tensors on a HIP device only")
    if dense if use_kernels is None else bool(use_kernels):
        keep, count, info = voxel_keep_kernels(xyz, score, inv)
        kept, err = (int(v) for v in info.tolist())
        if err:
            raise RuntimeError("das3r_thin_voxels: the hash table was exhausted (workspace smaller than das3r_thin_workspace_bytes?)")
        return keep.view(torch.bool), count, kept
    keep, count = voxel_keep_torch(xyz, None if score is None else score.float(), inv)
    return keep, count, int(keep.sum().item())


@torch.no_grad()
def pixel_footprint(depths, K, mask=None):
    """The median over masked pixels of depth / fx: the world-space side of a pixel at its own depth, the scale-free unit for the edge
    (DUSt3R scenes have no metric scale).  depths [F, H, W], K [F, 3, 3], mask: anything that reshapes to [F, H, W] (None: every pixel)."""
    d = depths.float()
    fp = d / K.float()[:, 0, 0][:, None, None]
    fp = fp.reshape(-1)
    if mask is not None:
        fp = fp[mask.reshape(-1).to(torch.bool)]
    fp = fp[torch.isfinite(fp) & (fp > 0)]
    if fp.numel() == 0:
        raise ValueError("pixel_footprint: no masked pixel with a positive finite depth")
    return float(fp.median())


def coverage_opacity(count, base, F):
    """The "coverage" opacity of a survivor that stands for `count` Gaussians of opacity 1/F: 1 - (1 - 1/F)^count — what that many stacked
    layers cover — in float64, clamped to <= 0.99, cast to fp32; where count == 1 the entry of `base` (the parent's 1/F tensor) itself."""
    c = count.reshape(base.shape).to(torch.float64)
    cov = (1.0 - torch.pow(torch.tensor(1.0 - 1.0 / float(F), dtype=torch.float64, device=base.device), c)).clamp(max=COVERAGE_MAX)
    return torch.where(count.reshape(base.shape) == 1, base, cov.to(torch.float32))


def default_score(model):
    """The effective opacity the model renders with: sigmoid(_opacity) * conf_static at the Gaussian's pixel (per Gaussian on a loaded model)."""
    from .prune import mask_index
    conf = model._conf_static.detach().reshape(-1)
    if hasattr(model, "aggregated_mask"):
        conf = conf[mask_index(model)]
    return (torch.sigmoid(model._opacity.detach().reshape(-1).float()) * conf.float()).contiguous()


@torch.no_grad()
def thin_model(model, edge, score=None, use_kernels=None):
    """Thin a trained or loaded model through the existing surgery, prune_points(model, min_opacity=0, also_drop=~keep): parameters, Adam
    moments, aggregated_mask, _mask_index and the cached states follow.  score: [P] fp32, default default_score(model).  Opacities and scales
    are NOT touched: a trained model has already learnt them.  -> prune_points' info dict + edge"""
    from .prune import prune_points
    score = default_score(model) if score is None else score
    keep, _, _ = voxel_keep(model._xyz.detach(), score, edge=edge, use_kernels=use_kernels)
    info = prune_points(model, min_opacity=0.0, also_drop=~keep, use_kernels=use_kernels)
    info["edge"] = float(edge)
    return info
