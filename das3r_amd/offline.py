"""Offline render of a trained sequence — the counterpart of /root/reference/render.py:72-123 (`render_set` / `render_sets`):
load <model_path>/point_cloud/iteration_N/point_cloud.ply, render every training camera, write
<model_path>/interp/ours_N/renders/%05d.png, and turn <model_path>/pose/pose_N.npy into pose/pose_interpolated.npy
(render.py:32-52 `save_interpolate_pose`, minus the two matplotlib trajectory plots, which are figures, not data).

    python -m das3r_amd.offline --model-path OUT/market_2 --source-path DATA/market_2 [--iteration -1] [--optimised-poses]

What is rendered.  The reference calls `render()` on a model it has just loaded from the PLY — which reads `pc.aggregated_mask`, an
attribute only `create_from_cameras` sets: as written, its offline renderer stops with an AttributeError.  The renderer that works
on a loaded PLY is the one the reference's own evaluation uses, `render_test` (gaussian_renderer/__init__.py:152-277: opacity x the
per-Gaussian `conf_static` as stored — exactly the two columns `load_ply` reads back, scene/gaussian_model.py:371-418); that is what
runs here (das3r_amd.render variant="test"), under torch.no_grad like the reference.  Poses: the reference renders each view from
the pose its camera was LOADED with (sparse/0/images.txt: `view.world_view_transform`), not from the optimised pose it saved;
`optimised_poses=True` (CLI --optimised-poses) takes pose/pose_N.npy instead, which is what one wants to look at.

Eval-mode throughput: `forward_throughput` times the same no-grad forward (the path that waits for the binning self-check inside
every call: rasterizer.py) and is what bench.py reports as `eval_forward`."""
import argparse
import os
import re
import time
from types import SimpleNamespace

import numpy as np
import torch

from .model import SplatModel
from .render import das3r_render


def tensor_from_camera(RT, device="cuda"):
    """utils/pose_utils.py:183-215 get_tensor_from_camera: 4x4 world-to-camera -> (qw, qx, qy, qz, tx, ty, tz), the quaternion by
    rotation2quad (io_formats.matrix_to_quat_wxyz, pinned by the reference's own outputs in tests/golden)."""
    from .io_formats import matrix_to_quat_wxyz
    m = RT.detach().cpu().numpy() if torch.is_tensor(RT) else np.asarray(RT)
    return torch.from_numpy(np.concatenate([matrix_to_quat_wxyz(m[:3, :3]), m[:3, 3]]).astype(np.float32)).to(device)


def save_image(chw, path):
    """torchvision.utils.save_image for one image: x -> clamp(255 x + 0.5, 0, 255) -> uint8 -> PNG (render.py:84-86 writes with it)."""
    from PIL import Image
    arr = chw.detach().float().mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(arr).save(path, format="PNG")
    return arr


def search_for_max_iteration(folder):
    """utils/system_utils.py searchForMaxIteration: the largest N among <folder>/iteration_N."""
    its = [int(m.group(1)) for m in (re.fullmatch(r"iteration_(\d+)", f) for f in os.listdir(folder)) if m]
    if not its:
        raise FileNotFoundError(f"no iteration_* under {folder}")
    return max(its)


def load_trained_model(model_path, iteration=-1, sh_degree=3, device="cuda"):
    """GaussianModel.load_ply (scene/gaussian_model.py:371-418) into a SplatModel: `opacity_ori` as the opacity parameter, the
    per-Gaussian `conf_static` column [P, 1], active degree = maximum degree.  -> (model, iteration)"""
    from .io_formats import load_gaussians_ply
    if iteration == -1:
        iteration = search_for_max_iteration(os.path.join(model_path, "point_cloud"))
    g = load_gaussians_ply(os.path.join(model_path, "point_cloud", f"iteration_{iteration}", "point_cloud.ply"), max_sh_degree=sh_degree)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=torch.float32)
    m = SplatModel(sh_degree)
    m._xyz, m._features_dc, m._features_rest = t(g["xyz"]), t(g["features_dc"]), t(g["features_rest"])
    m._opacity, m._conf_static, m._scaling, m._rotation = t(g["opacity"]), t(g["conf_static"]), t(g["scaling"]), t(g["rotation"])
    m.active_sh_degree = sh_degree
    return m, iteration


def save_interpolate_pose(model_path, iteration):
    """render.py:32-52 with its interpolation commented out, as it is there: pose_N.npy ([N, 4, 4] world-to-camera) -> 4x4 matrices
    rebuilt from the rotation and translation blocks -> pose/pose_interpolated.npy.  -> the array, or None without a pose file."""
    src = os.path.join(model_path, "pose", f"pose_{iteration}.npy")
    if not os.path.exists(src):
        return None
    org = np.load(src)
    out = np.stack([np.block([[p[:3, :3], p[:3, 3:4]], [np.zeros((1, 3)), np.ones((1, 1))]]) for p in org], 0)
    np.save(os.path.join(model_path, "pose", "pose_interpolated.npy"), out)
    return out


def sequence_cameras(seq, device="cuda"):
    """Every frame of a sequence dict (io_formats.load_sequence / train.consistent_sequence) as a camera with the pose it was loaded
    with: what Scene(..., shuffle=False).getTrainCameras() is for render.py, which runs with args.eval = False (no held-out split)."""
    from .train import make_camera
    K = seq["K"]
    cams = []
    for i in range(seq["images"].shape[0]):
        c = make_camera(i, seq["images"][i].to(device), float(K[i, 0, 0]), seq["W"], seq["H"], device, focal_y=float(K[i, 1, 1]),
                        camera_center=seq["cam2world"][i][:3, 3])
        c.pose7 = seq["w2c_pose7"][i].to(device=device, dtype=torch.float32)
        cams.append(c)
    return cams


def apply_fov(views, fovx, fovy):
    """Give every camera the field of view (radians) of a job that trained it — <model_path>/fov.json — and the projection built from it
    (train.make_camera's matrix at those values).  In place; -> views."""
    from .camera import projection_matrix
    for v in views:
        dev = v.projection_matrix.device
        v.FoVx, v.FoVy = float(fovx), float(fovy)
        v.projection_matrix = projection_matrix(0.01, 100.0, float(fovx), float(fovy)).transpose(0, 1).to(dev)
    return views


PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


class _EvalState:
    """What a model's fused no-grad renders share: the pose matrices' buffer and the packed [P, (D + 1)^2, 3] SH tensor the rasterizer reads
    (get_features is a torch.cat of 190 bytes per Gaussian — rebuilt only when a parameter was written since)."""

    def __init__(self, model):
        dev = model._xyz.device
        self.mats = torch.empty(28, device=dev)
        self.e = torch.empty(0, device=dev)
        self.shs, self.versions = None, None

    def packed_sh(self, model):
        v = (model._features_dc._version, model._features_rest._version, model._features_dc.data_ptr(), model._features_rest.data_ptr())
        if self.shs is None or v != self.versions:
            self.shs, self.versions = model.get_features.detach().contiguous(), v
        return self.shs


@torch.no_grad()
def render_view_fused(model, view, pose7, background, pipe=PIPE, invdepth=False, features=None, alpha=False, return_state=False, distortion=False,
                      median_depth=False, normals=False):
    """render_test of one view (gaussian_renderer/__init__.py:152-277) with the pose pre-transform INSIDE the rasterizer's per-Gaussian
    kernel (include/das3r_raster.h das3r_raster_in.pre, as the direct training iteration uses it): R xyz + t, quaternion product, exp,
    sigmoid x the per-Gaussian conf_static column — the dozen PyTorch kernels of the reference's glue (a boolean-mask gather of every
    tensor among them: 190 bytes of SH per Gaussian copied per view) are not launched and the camera-frame tensors never exist.
    Same arithmetic up to the rounding of the pre-transform (tests: within the parity bars of the glue form).  -> (image, radii), or with
    invdepth (image, radii, inverse-depth image [1, H, W]: include/das3r_raster.h das3r_raster_out.out_invdepth).  features ([P, C] fp32) /
    alpha: appended after those, in this order — the [C, H, W] image of the channels blended over this forward's lists
    (rasterizer.composite_features) and the [1, H, W] coverage (rasterizer.alpha_of); distortion: then the [1, H, W] ray-distortion image
    (rasterizer.distortion_of); median_depth: then the [1, H, W] median depth (rasterizer.median_depth_of: the view-space depth of the Gaussian
    at which the ray's transmittance crosses one half); normals: then the [3, H, W] view-space normal image — the Gaussians' normals
    (rasterizer.gaussian_normals of the camera-frame rotations and means, which this one option forms in torch ops) blended over the same lists —
    and the [3, H, W] normal of the median-depth image (rasterizer.depth_normals); return_state: last, the forward's RasterState."""
    import ctypes as C
    from . import _lib
    from .rasterizer import _forward, _on_device, _stream, alpha_of, composite_features, distortion_of, median_depth_of
    from .render import _settings
    st = model.__dict__.get("_das3r_eval")
    if st is None:
        st = model.__dict__["_das3r_eval"] = _EvalState(model)
    dev = model._xyz.device
    lib = _lib.load()
    pose7 = pose7.detach().to(device=dev, dtype=torch.float32).contiguous()
    conf = model._conf_static.detach().reshape(-1)
    if conf.shape[0] != model._xyz.shape[0]:
        raise RuntimeError("render_view_fused renders a LOADED model (one conf_static value per Gaussian: load_trained_model)")
    with _on_device(dev):
        _lib.check(lib.das3r_pose_matrices(C.c_void_p(pose7.data_ptr()), C.c_void_p(st.mats.data_ptr()), _stream(dev)), "das3r_pose_matrices")
    pre = _lib.PreTransform()
    xyz, rot, sc, op = model._xyz.detach(), model._rotation.detach(), model._scaling.detach(), model._opacity.detach()
    pre.xyz, pre.rot, pre.scaling, pre.opacity_raw = xyz.data_ptr(), rot.data_ptr(), sc.data_ptr(), op.data_ptr()
    pre.conf_flat, pre.mask_index = conf.data_ptr(), None
    pre.R, pre.t, pre.Lq = st.mats.data_ptr(), st.mats.data_ptr() + 36, st.mats.data_ptr() + 48
    rs = _settings(view, model, pipe, background, 1.0, dev)
    state, image, radii, inv = _forward(rs, xyz, st.packed_sh(model), st.e, op, sc, rot, st.e, pre=pre, invdepth=invdepth, no_backward=True,
                                        antialiasing=bool(getattr(pipe, "antialiasing", False)))
    state.check()   # (no backward pass will examine this forward's binning self-check)
    out = (image, radii, inv) if invdepth else (image, radii)
    if features is not None:
        out = out + (composite_features(state, features),)
    if alpha:
        out = out + (alpha_of(state),)
    if distortion:
        out = out + (distortion_of(state),)
    if median_depth:
        out = out + (median_depth_of(state),)
    if normals:
        from .camera import camera_from_tensor, quat_multiply
        from .rasterizer import depth_normals, gaussian_normals
        w2c = camera_from_tensor(pose7)
        per_gaussian = gaussian_normals(rs, quat_multiply(pose7[:4], rot).contiguous(), model.get_scaling.detach().contiguous(),
                                        (xyz @ w2c[:3, :3].T + w2c[:3, 3]).contiguous())
        out = out + (composite_features(state, per_gaussian), depth_normals(median_depth_of(state), rs))
    if return_state:
        out = out + (state,)
    return out


def invdepth_median_rel_error(invdepth, depth):
    """Diagnostic of --depth: median over the pixels with invdepth > 0 of |1/invdepth - depth| / depth, the rendered inverse depth against
    a sequence's depth map (depth_maps/frame_%04d.npy, [H, W]).  NaN when no pixel is covered."""
    inv = torch.as_tensor(invdepth).detach().reshape(-1).float().cpu()
    d = torch.as_tensor(depth).detach().reshape(-1).float().cpu()
    sel = (inv > 0) & (d > 0)
    if not bool(sel.any()):
        return float("nan")
    return float(((1.0 / inv[sel] - d[sel]).abs() / d[sel]).median())


def median_depth_median_rel_error(median_depth, depth):
    """Diagnostic of --median-depth, the one --depth prints on the other depth image: median over the pixels with median_depth > 0 of
    |median_depth - depth| / depth against a sequence's depth map.  NaN when no pixel is covered."""
    z = torch.as_tensor(median_depth).detach().reshape(-1).float().cpu()
    d = torch.as_tensor(depth).detach().reshape(-1).float().cpu()
    sel = (z > 0) & (d > 0)
    if not bool(sel.any()):
        return float("nan")
    return float(((z[sel] - d[sel]).abs() / d[sel]).median())


@torch.no_grad()
def render_set(model_path, name, iteration, views, model, pipe=PIPE, background=None, poses=None, write=True, fused=False, invdepth=None,
               exposures=None, static_map=None, alpha=None, distortion=None, median_depth=None, normals=None):
    """render.py:72-86.  views: cameras carrying .pose7 (qw, qx, qy, qz, tx, ty, tz world-to-camera); poses: optional [N, 4, 4]
    world-to-camera matrices that override them.  fused: render_view_fused instead of the reference's PyTorch glue in front of the
    rasterizer (opt-in, like every fused form).  invdepth: a list that receives every view's inverse-depth image [1, H, W] (written as
    invdepth/%05d.npy next to renders/ when `write`); None: colour only.  exposures: per view a [3, 4] exposure matrix (applied to the
    render: das3r_amd.losses.apply_exposure) or None.  static_map / alpha: lists that receive every view's static-confidence map — the
    loaded model's per-Gaussian conf_static column blended over the view's own lists, [1, H, W] — and its coverage map [1, H, W]
    (written as static/%05d.npy and alpha/%05d.npy beside invdepth/, in the same format, when `write`); None: not computed.
    distortion: a list that receives every view's ray-distortion image [1, H, W] from the render's own lists (rasterizer.distortion_of;
    written as distortion/%05d.npy, as alpha is); None: not computed.
    median_depth: a list that receives every view's median-depth image [1, H, W] from the render's own lists (rasterizer.median_depth_of;
    written as median_depth/%05d.npy, as alpha is); None: not computed.
    normals: a list that receives every view's (normal image, depth-normal image) pair, both [3, H, W] in view space — the Gaussians' normals
    blended over the render's own lists and the normal of its median-depth image (rasterizer.gaussian_normals / depth_normals; written as
    normals/%05d.npy and depth_normals/%05d.npy beside alpha/); None: not computed.
    -> list of the rendered [3, H, W] tensors (on the device)."""
    dev = model.get_xyz.device
    background = background if background is not None else torch.zeros(3, device=dev)
    base = os.path.join(model_path, name, f"ours_{iteration}")
    render_path = os.path.join(base, "renders")
    want, want_static, want_alpha, want_dist = invdepth is not None, static_map is not None, alpha is not None, distortion is not None
    want_median, want_normals = median_depth is not None, normals is not None
    conf = None
    if want_static:
        conf = model._conf_static.detach().reshape(-1, 1).float().contiguous()
        if conf.shape[0] != model.get_xyz.shape[0]:
            raise RuntimeError("render_set(static_map=...) renders a LOADED model (one conf_static value per Gaussian: load_trained_model)")
    out = []
    for idx, view in enumerate(views):
        pose = view.pose7 if poses is None else tensor_from_camera(poses[idx], dev)
        smap = amap = dmap = zmap = nmap = dnmap = None
        if fused:
            res = render_view_fused(model, view, pose, background, pipe, invdepth=want, features=conf, alpha=want_alpha,
                                    **({"distortion": True} if want_dist else {}), **({"median_depth": True} if want_median else {}),
                                    **({"normals": True} if want_normals else {}))
            img, inv = res[0], (res[2] if want else None)
            nxt = 3 if want else 2
            if want_static:
                smap, nxt = res[nxt], nxt + 1
            if want_alpha:
                amap, nxt = res[nxt], nxt + 1
            if want_dist:
                dmap, nxt = res[nxt], nxt + 1
            if want_median:
                zmap, nxt = res[nxt], nxt + 1
            if want_normals:
                nmap, dnmap = res[nxt], res[nxt + 1]
        else:
            pkg = das3r_render(view, model, pipe, background, camera_pose=pose, variant="test", return_invdepth=want, features=conf,
                               return_alpha=want_alpha, **({"return_state": True} if want_dist or want_median or want_normals else {}),
                               **({"return_normals": True} if want_normals else {}))
            img, inv, smap, amap = pkg["render"], pkg.get("invdepth"), pkg.get("features"), pkg.get("alpha")
            if want_dist:
                from .rasterizer import distortion_of
                dmap = distortion_of(pkg["raster_state"])
            if want_median:
                from .rasterizer import median_depth_of
                zmap = median_depth_of(pkg["raster_state"])
            if want_normals:
                from .rasterizer import depth_normals, median_depth_of
                from .render import _settings
                nmap = pkg["normals"]
                dnmap = depth_normals(median_depth_of(pkg["raster_state"]) if zmap is None else zmap, _settings(view, model, pipe, background, 1.0, dev))
        if exposures is not None and exposures[idx] is not None:
            from .losses import apply_exposure
            img = apply_exposure(img, torch.as_tensor(exposures[idx], dtype=img.dtype, device=img.device))
        out.append(img)
        if want:
            invdepth.append(inv)
        if want_static:
            static_map.append(smap)
        if want_alpha:
            alpha.append(amap)
        if want_dist:
            distortion.append(dmap)
        if want_median:
            median_depth.append(zmap)
        if want_normals:
            normals.append((nmap, dnmap))
        if write:
            save_image(img, os.path.join(render_path, f"{idx:05d}.png"))
            for sub, m in (("invdepth", inv if want else None), ("static", smap), ("alpha", amap), ("distortion", dmap),
                           ("median_depth", zmap)):
                if m is not None:
                    os.makedirs(os.path.join(base, sub), exist_ok=True)
                    np.save(os.path.join(base, sub, f"{idx:05d}.npy"), m[0].detach().cpu().numpy())
            for sub, m in (("normals", nmap), ("depth_normals", dnmap)):   # (three channels: the whole [3, H, W] tensor)
                if m is not None:
                    os.makedirs(os.path.join(base, sub), exist_ok=True)
                    np.save(os.path.join(base, sub, f"{idx:05d}.npy"), m.detach().cpu().numpy())
    return out


def render_sets(model_path, seq, iteration=-1, sh_degree=3, white_background=False, optimised_poses=False, device="cuda", write=True, fused=False,
                depth=False, pipe=PIPE, prune_min_opacity=0.0, write_pruned_ply=False, exposure="none", static_map=False, alpha=False, thin_edge=None, thin_relative=None,
                camera_fov=False, distortion=False, median_depth=False, normals=False, tsdf=False, tsdf_voxel=None, tsdf_relative=None, tsdf_trunc=4.0,
                tsdf_depth="median", tsdf_min_alpha=0.5, tsdf_static_weight=False, tsdf_min_faces=0, tsdf_keep_largest=0):
    """render.py:89-123: load the trained model, write pose_interpolated.npy, render the "interp" set.  seq: the sequence the model was
    trained on (its cameras).  depth: also the inverse-depth images (invdepth/%05d.npy) and, per view, the median relative error of
    1 / invdepth against the sequence's depth map (printed: a diagnostic).  pipe: PIPE, or pipe_from_args' (pipe.antialiasing: a model
    trained with antialiasing is rendered with it).  prune_min_opacity > 0: the loaded model is compacted first (das3r_amd.prune.prune_points:
    the Gaussians with sigmoid(opacity) * conf_static below it go; at or below 1/255 the renders do not change); write_pruned_ply: the
    compacted model is saved as point_cloud/iteration_N/point_cloud_pruned.ply.  exposure: "none" (the default: today's output) or "train" —
    <model_path>/exposure.json (a job that trained with per-frame exposure compensation writes it) is loaded and every view whose frame
    name it holds, i.e. every training view, is written compensated; the others stay raw.  static_map / alpha: also every view's
    static-confidence map and coverage map (render_set: static/%05d.npy, alpha/%05d.npy); distortion: and its ray-distortion image
    (distortion/%05d.npy, from the render's own lists); median_depth: and its median-depth image (median_depth/%05d.npy, from the same
    lists) with, per view, the diagnostic `depth` prints — the median relative error against the sequence's depth map — so that the blended
    and the median depth can be compared on one sequence.  normals: and its view-space normal image and the normal of its median-depth image
    (normals/%05d.npy, depth_normals/%05d.npy, [3, H, W], beside alpha/).  thin_edge (world units) / thin_relative (multiples of
    the pixel footprint of `seq`'s depth maps and intrinsics: das3r_amd.thin.pixel_footprint over its confident pixels), at most one: the loaded
    model is thinned to one Gaussian per voxel first (das3r_amd.thin.thin_model, after prune_min_opacity's event when both are given);
    write_pruned_ply then saves the thinned model.  A model directory that holds fov.json (a job that trained its field of view: farm
    --fov-lr) is rendered with that field of view; camera_fov: ignore the file and keep the cameras' own.  Without the file: today's output.
    tsdf: after the renders, the views' surface depths are fused into one TSDF grid and a mesh is taken from it (fuse_and_mesh below:
    tsdf/mesh.ply and tsdf/tsdf.npz beside renders/); tsdf_voxel (world units) / tsdf_relative (pixel footprints, as thin_relative; default 2),
    tsdf_trunc (voxels), tsdf_depth ("median" | "blended"), tsdf_min_alpha, tsdf_static_weight: das3r_amd.tsdf.fuse_views'.
    tsdf_min_faces / tsdf_keep_largest: with either above 0 the mesh is cleaned before it is written (das3r_amd.mesh.filter_components: the
    connected pieces with fewer faces than the keep rule's threshold go, with their vertices) and tsdf/components.json records the pieces.
    -> (iteration, list of rendered images)"""
    if exposure not in ("none", "train"):
        raise ValueError(f'render_sets: exposure must be "none" or "train", got {exposure!r}')
    if thin_edge is not None and thin_relative is not None:
        raise ValueError("render_sets: give thin_edge (world units) or thin_relative (pixel footprints), not both")
    model, iteration = load_trained_model(model_path, iteration, sh_degree, device)
    if prune_min_opacity > 0:
        from .prune import prune_points
        info = prune_points(model, min_opacity=prune_min_opacity)
        print(f"pruned {info['dropped']} of {info['before']} Gaussians below opacity {prune_min_opacity:g}")
    if thin_edge is not None or thin_relative is not None:
        from .thin import pixel_footprint, thin_model
        edge = thin_edge
        if edge is None:
            if seq.get("depths") is None:
                raise ValueError("render_sets(thin_relative=...): the sequence has no depth maps to take the pixel footprint from; give thin_edge")
            confs = seq.get("confs")
            edge = float(thin_relative) * pixel_footprint(seq["depths"], seq["K"], None if confs is None else confs > 0.0)
        info = thin_model(model, edge)
        print(f"thinned {info['dropped']} of {info['before']} Gaussians to one per voxel of edge {info['edge']:g}")
    if write_pruned_ply and (prune_min_opacity > 0 or thin_edge is not None or thin_relative is not None):
        from .prune import write_pruned_ply as save_pruned
        save_pruned(os.path.join(model_path, "point_cloud", f"iteration_{iteration}", "point_cloud_pruned.ply"), model)
    inter = save_interpolate_pose(model_path, iteration)
    bg = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    views = sequence_cameras(seq, device)
    fov_path = os.path.join(model_path, "fov.json")
    if not camera_fov and os.path.exists(fov_path):
        from .io_formats import read_fov_json
        fov = read_fov_json(fov_path)
        apply_fov(views, fov["FoVx"], fov["FoVy"])
        print(f"rendering with the trained field of view of {fov_path}: focal {fov['focal_x']:.3f} x {fov['focal_y']:.3f} px")
    frames = list(range(len(views)))   # (the sequence frame of each view: its depth map)
    poses = None
    if optimised_poses:
        if inter is None:
            raise FileNotFoundError(f"--optimised-poses: no pose/pose_{iteration}.npy under {model_path}")
        if len(inter) != len(views):   # (a job trained with the held-out split saved the training views' poses only)
            from .train import split_sequence
            tr, _ = split_sequence(seq)
            if len(inter) != len(tr):
                raise ValueError(f"pose_{iteration}.npy holds {len(inter)} poses, the sequence {len(views)} frames ({len(tr)} training frames)")
            views = [views[i] for i in tr]
            frames = list(tr)
        poses = inter
    inv = [] if depth else None
    med = [] if median_depth else None
    exposures = None
    if exposure == "train":
        from .io_formats import read_exposure_json, sequence_frame_names
        path = os.path.join(model_path, "exposure.json")
        if not os.path.exists(path):
            raise FileNotFoundError(f'exposure="train": no exposure.json under {model_path} (the job trained without exposure compensation)')
        table, names = read_exposure_json(path), sequence_frame_names(seq)
        exposures = [table.get(names[f]) for f in frames]
    imgs = render_set(model_path, "interp", iteration, views, model, pipe, bg, poses=poses, write=write, fused=fused, invdepth=inv,
                      exposures=exposures, static_map=[] if static_map else None, alpha=[] if alpha else None,
                      **({"distortion": []} if distortion else {}), **({"median_depth": med} if median_depth else {}),
                      **({"normals": []} if normals else {}))
    if tsdf:
        fuse_and_mesh(os.path.join(model_path, "interp", f"ours_{iteration}", "tsdf"), model, views, seq, pipe, bg, poses=poses, voxel=tsdf_voxel,
                      relative=tsdf_relative, trunc_voxels=tsdf_trunc, depth=tsdf_depth, min_alpha=tsdf_min_alpha, static_weight=tsdf_static_weight,
                      write=write, **({"min_faces": tsdf_min_faces, "keep_largest": tsdf_keep_largest} if (tsdf_min_faces or tsdf_keep_largest) else {}))
    if depth and seq.get("depths") is not None:
        for idx, (f, d) in enumerate(zip(frames, inv)):
            print(f"view {idx:05d} (frame {f}): median |1/invdepth - depth| / depth = {invdepth_median_rel_error(d, seq['depths'][f]):.4f}")
    if median_depth and seq.get("depths") is not None:
        for idx, (f, z) in enumerate(zip(frames, med)):
            print(f"view {idx:05d} (frame {f}): median |median_depth - depth| / depth = {median_depth_median_rel_error(z, seq['depths'][f]):.4f}")
    return iteration, imgs


@torch.no_grad()
def fuse_and_mesh(out_dir, model, views, seq, pipe=PIPE, background=None, poses=None, voxel=None, relative=None, trunc_voxels=4.0, depth="median",
                  min_alpha=0.5, static_weight=False, write=True, quantile=0.01, min_faces=0, keep_largest=0):
    """--tsdf: fuse the loaded model's own renders of `views` into a TSDF grid over the box of its centres (das3r_amd.tsdf.bounds_from_points)
    and take the mesh.  voxel: the edge in world units; relative: in multiples of the pixel footprint of `seq` (das3r_amd.thin.pixel_footprint,
    as --thin-relative computes it; default 2 when neither is given), raised with a printed note while the box would exceed 2^28 voxels.
    poses: [N, 4, 4] world-to-camera matrices that override the views' own.  Writes <out_dir>/mesh.ply (vertices, normals, colours, faces)
    and <out_dir>/tsdf.npz (tsdf, weight, colour, origin, voxel, trunc) when `write`.  min_faces / keep_largest (both 0: off, the mesh is the
    extraction's as it is): the mesh is cleaned first (das3r_amd.mesh.filter_components) and <out_dir>/components.json holds the descending
    face counts of its pieces, the threshold, and the kept and dropped counts.  -> (grid, mesh dict)"""
    import copy
    from . import _lib
    from .io_formats import save_mesh_ply
    from .tsdf import TSDFGrid, bounds_from_points, fuse_views, grid_for_box
    if voxel is not None and relative is not None:
        raise ValueError("fuse_and_mesh: give voxel (world units) or relative (pixel footprints), not both")
    dev = model.get_xyz.device
    edge = voxel
    if edge is None:
        from .thin import pixel_footprint
        if seq.get("depths") is None:
            raise ValueError("--tsdf-relative: the sequence has no depth maps to take the pixel footprint from; give --tsdf-voxel")
        confs = seq.get("confs")
        edge = float(2.0 if relative is None else relative) * pixel_footprint(seq["depths"], seq["K"], None if confs is None else confs > 0.0)
    lo, hi = bounds_from_points(model.get_xyz, quantile)
    origin, dims = grid_for_box(lo, hi, edge)
    while dims[0] * dims[1] * dims[2] > _lib.TSDF_MAX_VOXELS:
        edge *= 1.25
        origin, dims = grid_for_box(lo, hi, edge)
        print(f"tsdf: the box would exceed 2^28 voxels; voxel edge raised to {edge:g}")
    if poses is not None:
        moved = []
        for idx, v in enumerate(views):
            v = copy.copy(v)
            v.pose7 = tensor_from_camera(poses[idx], dev)
            moved.append(v)
        views = moved
    grid = TSDFGrid(origin, edge, dims, device=dev, colour=True)
    fuse_views(model, views, pipe, background, grid, depth=depth, min_alpha=min_alpha, static_weight=static_weight, trunc=float(trunc_voxels) * grid.voxel)
    mesh = grid.extract()
    print(f"tsdf: {len(views)} views fused into {dims[0]} x {dims[1]} x {dims[2]} voxels of edge {grid.voxel:g}; mesh: {mesh['vertices'].shape[0]} vertices, "
          f"{mesh['faces'].shape[0]} triangles")
    report = None
    if min_faces or keep_largest:
        from .mesh import filter_components
        mesh, report = filter_components(mesh, min_faces=min_faces, keep_largest=keep_largest)
        print(f"tsdf: mesh clean-up (min faces {int(min_faces)}, keep largest {int(keep_largest)}: threshold {report['threshold']}): "
              f"{report['components']} pieces -> {report['kept_components']}, {report['vertices_before']} vertices -> {report['vertices_after']}, "
              f"{report['faces_before']} triangles -> {report['faces_after']}")
    if write:
        os.makedirs(out_dir, exist_ok=True)
        if report is not None:
            from .mesh import write_components_json
            write_components_json(os.path.join(out_dir, "components.json"), report)
        save_mesh_ply(os.path.join(out_dir, "mesh.ply"), mesh["vertices"], mesh["faces"], normals=mesh["normals"], colours=mesh["colours"])
        np.savez_compressed(os.path.join(out_dir, "tsdf.npz"), tsdf=grid.tsdf.cpu().numpy(), weight=grid.weight.cpu().numpy(),
                            colour=grid.colour.cpu().numpy(), origin=np.asarray(grid.origin, np.float32), voxel=np.float32(grid.voxel),
                            trunc=np.float32(grid.trunc if grid.trunc is not None else float(trunc_voxels) * grid.voxel))
    return grid, mesh


@torch.no_grad()
def forward_throughput(model, views, repeats=3, background=None, fused=False):
    """Eval-mode (torch.no_grad) forward alone: views per second and ms per view over `repeats` passes of all views, after one
    warm-up pass.  In this mode the rasterizer examines every forward's binning self-check before it returns (there is no backward
    to do it), so the figure contains that wait — the path render.py and every held-out report take."""
    dev = model.get_xyz.device
    background = background if background is not None else torch.zeros(3, device=dev)
    run = ((lambda: [render_view_fused(model, v, v.pose7, background)[0] for v in views]) if fused
           else (lambda: [das3r_render(v, model, PIPE, background, camera_pose=v.pose7, variant="test")["render"] for v in views]))
    run()
    torch.cuda.current_stream(dev).synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        run()
    torch.cuda.current_stream(dev).synchronize()
    dt = (time.perf_counter() - t0) / (repeats * len(views))
    return dict(ms_per_view=dt * 1e3, views_per_s=1.0 / dt, views=len(views), splats=int(model.get_xyz.shape[0]))


def pipe_from_args(args):
    """The `pipe` a command line renders with: PIPE, and pipe.antialiasing from --antialiasing."""
    return SimpleNamespace(**vars(PIPE), antialiasing=bool(getattr(args, "antialiasing", False)))


def _count(text):
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError(f"{text!r} is negative")
    return n


def parser():
    ap = argparse.ArgumentParser(description="Testing script parameters (render.py)")
    ap.add_argument("--model-path", "-m", "--model_path", dest="model_path", required=True)
    ap.add_argument("--source-path", "-s", "--source_path", dest="source_path", required=True, help="the preprocessed sequence directory the model was trained on")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--sh-degree", "--sh_degree", dest="sh_degree", type=int, default=3)
    ap.add_argument("--white-background", "--white_background", dest="white_background", action="store_true")
    ap.add_argument("--optimised-poses", action="store_true", help="render from pose/pose_N.npy instead of the poses the cameras were loaded with")
    ap.add_argument("--dataset", default="sintel", choices=("sintel", "davis"))
    ap.add_argument("--fused", action="store_true", help="the pose pre-transform inside the rasterizer's kernels instead of the reference's PyTorch glue (render_view_fused)")
    ap.add_argument("--depth", action="store_true", help="also write the inverse-depth images (invdepth/%%05d.npy next to renders/) and print each view's "
                                                         "median relative error of 1/invdepth against the sequence's depth_maps")
    ap.add_argument("--antialiasing", action="store_true", help="the rasterizer's antialiasing mode (upstream's 2D mip filter), fused or not: "
                                                                "render a model trained with it (farm --antialiasing) this way")
    ap.add_argument("--prune-min-opacity", type=float, default=0.0, help="compact the loaded model before rendering: drop the Gaussians with "
                    "sigmoid(opacity) * conf_static below this (0: off; at or below 1/255 = 0.0039 the renders do not change)")
    thin = ap.add_mutually_exclusive_group()
    thin.add_argument("--thin-edge", type=float, default=None, help="thin the loaded model to one Gaussian per voxel of this edge (world units) before "
                      "rendering: the highest sigmoid(opacity) * conf_static of a voxel stays (after --prune-min-opacity's event when both are given)")
    thin.add_argument("--thin-relative", type=float, default=None, help="the same with the edge in multiples of the pixel footprint (median depth / focal) "
                      "of the sequence given with -s")
    ap.add_argument("--write-pruned-ply", action="store_true", help="with --prune-min-opacity, --thin-edge or --thin-relative: save the compacted model as "
                    "point_cloud/iteration_N/point_cloud_pruned.ply")
    ap.add_argument("--exposure", default="none", choices=("none", "train"), help='"train": write the training views compensated with the matrices '
                    "of <model-path>/exposure.json (a job trained with --exposure-lr-init / --exposure-lr-final); none: the raw renders")
    ap.add_argument("--camera-fov", action="store_true", help="keep the cameras' own field of view even when <model-path>/fov.json (a job trained with "
                    "farm --fov-lr) holds a trained one")
    ap.add_argument("--static-map", action="store_true", help="also write every view's static-confidence map (static/%%05d.npy next to renders/): the "
                    "model's per-Gaussian conf_static blended over the view's own lists, at any view, without a second forward")
    ap.add_argument("--alpha", action="store_true", help="also write every view's coverage map 1 - T (alpha/%%05d.npy next to renders/)")
    ap.add_argument("--distortion", action="store_true", help="also write every view's ray-distortion image, sum_{j<k} w_j w_k (1/z_j - 1/z_k) per pixel "
                    "over the render's own lists (distortion/%%05d.npy next to renders/)")
    ap.add_argument("--median-depth", action="store_true", help="also write every view's median depth — the view-space depth of the Gaussian at which the "
                    "ray's transmittance crosses one half, from the render's own lists (median_depth/%%05d.npy next to renders/) — and print, per view, "
                    "its median relative error against the sequence's depth map (what --depth prints for the blended depth)")
    ap.add_argument("--normals", action="store_true", help="also write every view's normal image — the Gaussians' thinnest axes, facing the camera, blended "
                    "over the render's own lists (normals/%%05d.npy beside alpha/) — and the normal of its median-depth image (depth_normals/%%05d.npy), "
                    "both [3, H, W] in view space")
    ap.add_argument("--tsdf", action="store_true", help="after the renders, fuse every view's surface depth into one TSDF grid and write the mesh taken "
                    "from it — tsdf/mesh.ply (vertices, normals, colours, triangles) and tsdf/tsdf.npz (the grid) beside renders/")
    edge = ap.add_mutually_exclusive_group()
    edge.add_argument("--tsdf-voxel", type=float, default=None, help="with --tsdf: the voxel edge in world units")
    edge.add_argument("--tsdf-relative", type=float, default=None, help="with --tsdf: the voxel edge in multiples of the pixel footprint of the sequence "
                      "given with -s, as --thin-relative (default 2; raised with a note if the model's box would exceed 2^28 voxels)")
    ap.add_argument("--tsdf-trunc", type=float, default=4.0, help="with --tsdf: the truncation distance in voxels")
    ap.add_argument("--tsdf-depth", default="median", choices=("median", "blended"), help="with --tsdf: the depth that is fused — the median depth of "
                    "the render's lists, or 1 / its blended inverse depth")
    ap.add_argument("--tsdf-min-alpha", type=float, default=0.5, help="with --tsdf: pixels whose coverage is below this are not fused")
    ap.add_argument("--tsdf-static-weight", action="store_true", help="with --tsdf: weigh every pixel by the static-confidence map of its view")
    ap.add_argument("--tsdf-min-faces", type=_count, default=0, help="with --tsdf: before the mesh is written, drop its connected pieces with fewer "
                    "triangles than this, and their vertices (0: off); tsdf/components.json records the pieces")
    ap.add_argument("--tsdf-keep-largest", type=_count, default=0, help="with --tsdf: keep the K pieces with the most triangles (ties with the K-th "
                    "stay too; 0: off); combines with --tsdf-min-faces: a piece must pass both")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    from .io_formats import load_sequence
    print("Rendering " + args.model_path)
    seq = load_sequence(args.source_path, device="cuda", dataset=args.dataset)
    it, imgs = render_sets(args.model_path, seq, args.iteration, args.sh_degree, args.white_background, args.optimised_poses, fused=args.fused,
                           depth=args.depth, pipe=pipe_from_args(args), prune_min_opacity=args.prune_min_opacity, write_pruned_ply=args.write_pruned_ply,
                           exposure=args.exposure, static_map=args.static_map, alpha=args.alpha, **({"camera_fov": True} if args.camera_fov else {}),
                           **({"distortion": True} if args.distortion else {}), **({"median_depth": True} if args.median_depth else {}),
                           **({"normals": True} if args.normals else {}),
                           **({"tsdf": True, "tsdf_voxel": args.tsdf_voxel, "tsdf_relative": args.tsdf_relative, "tsdf_trunc": args.tsdf_trunc,
                               "tsdf_depth": args.tsdf_depth, "tsdf_min_alpha": args.tsdf_min_alpha, "tsdf_static_weight": args.tsdf_static_weight}
                              if args.tsdf else {}),
                           **({"tsdf_min_faces": args.tsdf_min_faces, "tsdf_keep_largest": args.tsdf_keep_largest}
                              if (args.tsdf and (args.tsdf_min_faces or args.tsdf_keep_largest)) else {}),
                           **({"thin_edge": args.thin_edge, "thin_relative": args.thin_relative}
                              if (args.thin_edge is not None or args.thin_relative is not None) else {}))
    print(f"wrote {len(imgs)} images to {os.path.join(args.model_path, 'interp', f'ours_{it}', 'renders')}")


if __name__ == "__main__":
    main()
