"""Pruning of transparent Gaussians (opt-in) — the one density-control step DAS3R's model admits.

The reference carries the operation and never calls it: prune_points / _prune_optimizer / densify_and_prune
(/root/reference/scene/gaussian_model.py:436-468, 552-566; call sites commented out, train_gui.py:612-623).  Clone and split would break
`conf_static.reshape(-1, 1)[aggregated_mask]`, which needs exactly one Gaussian per True pixel; pruning keeps that mapping intact by
clearing mask bits.  A Gaussian is dropped iff

    eff = sigmoid(_opacity) * conf_static[its pixel] < min_opacity              (NaN compares false: kept, as get_opacity < min_opacity)
 or max_world_scale > 0 and max_k exp(_scaling_k) > max_world_scale             (the reference's big_points_ws, the limit in absolute units)
 or also_drop[i]                                                                (a caller's mask)

and at min_opacity <= 1/255 nothing that is left changes: such a Gaussian is binned with an empty rectangle and gets no gradient.

Two forms of the same surgery: on a HIP device with dense fp32 tensors, das3r_prune_select + das3r_prune_compact (csrc/prune.hip: one
decision pass, one pass over up to sixteen tensors, one host synchronise per event to size the new tensors); anywhere else plain torch
(`t[keep]`), which is also what the tests hold the kernels to."""
import ctypes as C
import warnings

import torch
from torch import nn

from . import _lib

PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
NEVER_BLENDED = 1.0 / 255.0   # below this opacity the compositing kernels skip a Gaussian at every pixel (alpha <= opacity)
_CACHES = ("_fast_state", "_das3r_eval")   # fast_step._State, offline._EvalState: P-sized buffers and raw pointers


def mask_index(model):
    """The flat pixel index of every Gaussian (nonzero of aggregated_mask), as the fused render paths cache it on the model."""
    idx = getattr(model, "_mask_index", None)
    if idx is None:
        idx = model._mask_index = torch.nonzero(model.aggregated_mask.reshape(-1), as_tuple=False).reshape(-1).contiguous()
    return idx


def keep_mask(opacity_raw, conf_flat, index=None, min_opacity=0.005, scaling=None, max_world_scale=0.0, also_drop=None):
    """The decision in torch ops -> bool [P], True = kept.  index: int64 [P] into conf_flat, None = identity."""
    conf = conf_flat.reshape(-1)
    conf = conf if index is None else conf[index]
    eff = torch.sigmoid(opacity_raw.reshape(-1).float()) * conf.float()
    drop = eff < torch.tensor(float(min_opacity), dtype=torch.float32, device=eff.device)
    if scaling is not None and max_world_scale > 0:
        drop = drop | (torch.exp(scaling.float()).max(dim=1).values > torch.tensor(float(max_world_scale), dtype=torch.float32, device=eff.device))
    if also_drop is not None:
        drop = drop | also_drop.reshape(-1).to(torch.bool)
    return ~drop


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _on(dev):
    from .rasterizer import _on_device
    return _on_device(dev)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def select(opacity_raw, conf_flat, index=None, min_opacity=0.005, scaling=None, max_world_scale=0.0, also_drop=None):
    """das3r_prune_select -> (dst_index int32 [P]: new row or -1, count: device int32 tensor whose word 0 is the number of kept rows).
    Dense device tensors: opacity_raw / conf_flat / scaling fp32, index int64, also_drop uint8 (or bool).  Nothing is read back."""
    lib = _lib.load()
    dev = opacity_raw.device
    if dev.type != "cuda":
        raise RuntimeError("das3r_amd.prune.select: tensors must live on a HIP device (the torch form is prune.keep_mask)")
    P = int(opacity_raw.shape[0])
    if also_drop is not None:
        also_drop = also_drop.reshape(-1)
        also_drop = also_drop.view(torch.uint8) if also_drop.dtype == torch.bool else also_drop
    for name, t, dt in (("opacity_raw", opacity_raw, torch.float32), ("conf_flat", conf_flat, torch.float32), ("index", index, torch.int64),
                        ("scaling", scaling, torch.float32), ("also_drop", also_drop, torch.uint8)):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != dev):
            raise RuntimeError(f"das3r_amd.prune.select: {name} must be a dense {dt} tensor on {dev}")
    if (index is not None and index.numel() != P) or (scaling is not None and tuple(scaling.shape) != (P, 3)) or (also_drop is not None and also_drop.numel() != P):
        raise ValueError("das3r_amd.prune.select: index / also_drop need P entries, scaling [P, 3]")
    if index is None and conf_flat.numel() < P:
        raise ValueError("das3r_amd.prune.select: conf_flat is shorter than P and there is no index")
    dst = torch.empty(P, dtype=torch.int32, device=dev)
    count = torch.empty(_lib.prune_count_words(P), dtype=torch.int32, device=dev)
    with _on(dev):
        rc = lib.das3r_prune_select(P, _ptr(opacity_raw), _ptr(conf_flat), _ptr(index), C.c_float(min_opacity), _ptr(scaling),
                                    C.c_float(max_world_scale), _ptr(also_drop), _ptr(dst), _ptr(count), _stream(dev))
    _lib.check(rc, "das3r_prune_select")
    return dst, count


def compact(dst_index, kept, tensors):
    """das3r_prune_compact -> [t[dst_index >= 0] for t in tensors] as new dense tensors, sixteen tensors per launch.  Every tensor is
    contiguous, on dst_index's device, with dst_index.numel() rows of a multiple of 4 bytes."""
    lib = _lib.load()
    dev = dst_index.device
    P, kept = int(dst_index.shape[0]), int(kept)
    out, jobs = [], []
    for t in tensors:
        if t.device != dev or not t.is_contiguous() or t.dim() < 1 or t.shape[0] != P:
            raise RuntimeError("das3r_amd.prune.compact: dense tensors with P rows on the index's device only")
        new = torch.empty((kept,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        row_bytes = (t.numel() // P) * t.element_size() if P else 0
        if row_bytes % 4:
            raise RuntimeError("das3r_amd.prune.compact: rows must be a multiple of 4 bytes")
        out.append(new)
        if row_bytes and kept and P:
            jobs.append((t, new, row_bytes))
    with _on(dev):
        for i in range(0, len(jobs), 16):
            chunk = jobs[i:i + 16]
            arr = (_lib.PruneTensor * len(chunk))()
            for k, (t, new, rb) in enumerate(chunk):
                arr[k].src, arr[k].dst, arr[k].row_bytes = t.data_ptr(), new.data_ptr(), rb
            _lib.check(lib.das3r_prune_compact(P, kept, _ptr(dst_index), len(chunk), arr, _stream(dev)), "das3r_prune_compact")
    return out


def _optimizers(model):
    return [o for o in (getattr(model, "optimizer", None),) if o is not None]


def _state_of(optimizer, p):
    return optimizer.state.get(p)   # (.get: torch's state is a defaultdict, a lookup must not create an entry)


@torch.no_grad()
def prune_points(model, min_opacity=0.005, max_world_scale=0.0, also_drop=None, use_kernels=None):
    """Drop the Gaussians the criteria above select and replace, consistently: the six per-Gaussian parameters (new nn.Parameters the
    optimizer's param_groups then point at), their Adam moments in torch.optim.Adam and in FusedAdam (compact SH moments in their compact
    shape, step counts kept), aggregated_mask (the dropped Gaussians' pixels cleared), the cached _mask_index (compacted, not recomputed),
    and every cache that holds a P-sized buffer or a pointer.  conf_static, the poses and the camera optimizer are per pixel / per frame
    and stay — except on a LOADED model (offline.load_trained_model: no aggregated_mask, one conf_static value per Gaussian), whose
    conf_static column is a seventh per-Gaussian tensor.
    use_kernels: None = the HIP kernels where the model qualifies (HIP device, dense fp32), else torch; False = torch; True = kernels or an
    error.  An event that would keep nothing is skipped with a warning.  -> dict(before, after, dropped, path)"""
    P = int(model._xyz.shape[0])
    info = dict(before=P, after=P, dropped=0, path="none")
    if P == 0:
        return info
    loaded = not hasattr(model, "aggregated_mask")
    conf_flat = model._conf_static.detach().reshape(-1)
    if loaded and conf_flat.numel() != P:
        raise RuntimeError("prune_points: a model without aggregated_mask needs one conf_static value per Gaussian")
    index = None if loaded else mask_index(model)
    dev = model._xyz.device
    if also_drop is not None:
        also_drop = torch.as_tensor(also_drop).to(dev).reshape(-1)
        if also_drop.numel() != P:
            raise ValueError("prune_points: also_drop needs one entry per Gaussian")
    # ---- everything with P rows: (tensor, where its compacted form goes)
    new_params, extra, entries = {}, {}, []
    for name in PARAMS:
        entries.append((getattr(model, name).detach(), new_params, name))
    states = []   # (optimizer, parameter name, state dict)
    for o in _optimizers(model):
        for name in PARAMS:
            st = _state_of(o, getattr(model, name))
            if st is not None:
                states.append((o, name, st))
                for k, v in st.items():
                    if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == P:
                        entries.append((v, st, k))
    if index is not None:
        entries.append((index, extra, "index"))
    else:
        entries.append((model._conf_static.detach(), extra, "conf"))
    dense = dev.type == "cuda" and all(t.device == dev and t.is_contiguous() and (t.dtype == torch.float32 or t is index) for t, _, _ in entries) \
        and conf_flat.is_contiguous() and conf_flat.dtype == torch.float32
    if use_kernels and not dense:
        raise RuntimeError("prune_points(use_kernels=True): dense fp32 tensors on a HIP device only")
    kernels = dense if use_kernels is None else bool(use_kernels)
    # ---- the decision, and the one host read of the event
    scaling = model._scaling.detach() if max_world_scale > 0 else None
    if kernels:
        dst, count = select(model._opacity.detach(), conf_flat, index, min_opacity, scaling, max_world_scale, also_drop)
        kept = int(count[0].item())
    else:
        keep = keep_mask(model._opacity.detach(), conf_flat, index, min_opacity, scaling, max_world_scale, also_drop)
        kept = int(keep.sum().item())
    info["path"] = "kernels" if kernels else "torch"
    if kept == 0:
        warnings.warn(f"prune_points: the event would drop all {P} Gaussians (min_opacity {min_opacity:g}); skipped")
        return info
    if kept == P:
        return info
    tensors = [t for t, _, _ in entries]
    moved = compact(dst, kept, tensors) if kernels else [t[keep].contiguous() for t in tensors]
    for (_, where, key), new in zip(entries, moved):
        where[key] = new
    # ---- parameters: new leaves, the optimizers' groups and state re-keyed to them (scene/gaussian_model.py _prune_optimizer)
    for name in PARAMS:
        old = getattr(model, name)
        new = nn.Parameter(new_params[name], requires_grad=old.requires_grad) if isinstance(old, nn.Parameter) else new_params[name]
        for o in _optimizers(model):
            for g in o.param_groups:
                g["params"] = [new if q is old else q for q in g["params"]]
            if old in o.state:
                o.state[new] = o.state.pop(old)
        setattr(model, name, new)
    # ---- the pixel <-> Gaussian mapping
    if index is not None:
        mask = torch.zeros_like(model.aggregated_mask, memory_format=torch.contiguous_format)
        mask.view(-1)[extra["index"]] = True
        model.aggregated_mask = mask
        model._mask_index = extra["index"]
    else:
        old = model._conf_static
        model._conf_static = nn.Parameter(extra["conf"], requires_grad=old.requires_grad) if isinstance(old, nn.Parameter) else extra["conf"]
    for k in _CACHES:   # buffers sized by the old P, pointers into the old tensors (the packed-SH mirror hangs on the old parameters and goes with them)
        model.__dict__.pop(k, None)
    info.update(after=kept, dropped=P - kept)
    return info


@torch.no_grad()
def contribution_scores(model, views, pipe=None, background=None):
    """-> [P] fp32: every Gaussian's blending-weight mass over `views`, sum_views sum_pixels alpha_i T_i — how much of the rendered images
    the Gaussian actually makes up (a Gaussian hidden behind others, or off every screen, scores 0 whatever its opacity: not what the opacity
    threshold above measures).  Per view: one no-grad forward and one adjoint of a ones image over that forward's lists
    (rasterizer.feature_adjoint: sum_pixels alpha T per Gaussian, no backward pass), accumulated in place after the first view.  No
    floating-point atomics: the scores are bit-identical from run to run.
    views: cameras; the pose is the view's own `.pose7` when it carries one, else the model's training pose of `view.uid`.  A training
    model is rendered as in training (opacity x conf_static at the Gaussian's pixel), a loaded one as the offline renderer does
    (variant "test").  The hand-off to the pruning event:

        scores = contribution_scores(model, cameras, pipe, background)
        prune_points(model, also_drop=scores < tau)        # tau: the caller's threshold, in units of pixels"""
    from types import SimpleNamespace
    from .rasterizer import feature_adjoint
    from .render import das3r_render
    pipe = pipe or SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    dev = model._xyz.device
    background = background if background is not None else torch.zeros(3, device=dev)
    variant = "render" if hasattr(model, "aggregated_mask") else "test"
    scores = torch.zeros(int(model._xyz.shape[0]), 1, dtype=torch.float32, device=dev)
    ones = {}
    for n, view in enumerate(views):
        pose = getattr(view, "pose7", None)
        pose = model.get_RT(view.uid) if pose is None else pose
        state = das3r_render(view, model, pipe, background, camera_pose=pose, variant=variant, return_state=True)["raster_state"]
        g = ones.get((state.H, state.W))
        if g is None:
            g = ones[(state.H, state.W)] = torch.ones(1, state.H, state.W, dtype=torch.float32, device=dev)
        feature_adjoint(state, g, out=scores, accumulate=n > 0)
    return scores.reshape(-1)


@torch.no_grad()
def surface_scores(model, views, pipe=None, background=None, threshold=0.5):
    """-> [P] fp32: the number of pixels over `views` at which each Gaussian is the HIT — the entry at which the ray's transmittance
    crosses `threshold` (0.5: the median; rasterizer.median_depth_of), i.e. how often the Gaussian is the visible surface.  What
    contribution_scores does not say: a Gaussian may carry blending-weight mass on many rays and be the surface of none of them (a faint
    floater in front, a near-copy behind the one that is hit).  Per view: one no-grad forward, one median kernel over that forward's lists
    and the hit adjoint of a ones image (rasterizer.median_hit_adjoint), accumulated in place after the first view.  The counts are integers
    in fp32, summing to the covered pixels of all views; no floating-point atomics: bit-identical from run to run.
    views, the pose and the variant: contribution_scores'.  The hand-off to the pruning event:

        scores = surface_scores(model, cameras, pipe, background)
        prune_points(model, also_drop=scores == 0)         # never the surface of any pixel of any view"""
    from types import SimpleNamespace
    from .rasterizer import _check_threshold, median_depth_of, median_hit_adjoint
    from .render import das3r_render
    threshold = _check_threshold(threshold)
    pipe = pipe or SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    dev = model._xyz.device
    background = background if background is not None else torch.zeros(3, device=dev)
    variant = "render" if hasattr(model, "aggregated_mask") else "test"
    scores = torch.zeros(int(model._xyz.shape[0]), dtype=torch.float32, device=dev)
    ones = {}
    for n, view in enumerate(views):
        pose = getattr(view, "pose7", None)
        pose = model.get_RT(view.uid) if pose is None else pose
        state = das3r_render(view, model, pipe, background, camera_pose=pose, variant=variant, return_state=True)["raster_state"]
        g = ones.get((state.H, state.W))
        if g is None:
            g = ones[(state.H, state.W)] = torch.ones(state.H, state.W, dtype=torch.float32, device=dev)
        _, position = median_depth_of(state, threshold=threshold, return_position=True)
        median_hit_adjoint(state, g, position, out=scores, accumulate=n > 0)
    return scores


def write_pruned_ply(path, model):
    """A loaded, pruned model back into the reference's PLY layout (io_formats.save_gaussians_ply)."""
    from .io_formats import save_gaussians_ply
    save_gaussians_ply(path, model._xyz, model._features_dc, model._features_rest, model._opacity, model._scaling, model._rotation, model._conf_static)
