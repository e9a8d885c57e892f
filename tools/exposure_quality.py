#!/usr/bin/env python3
"""Does per-frame exposure compensation do its job?  A self-consistent synthetic sequence (das3r_amd.train.consistent_sequence) whose
training frames flicker (train.apply_flicker: per-frame, per-channel gain in [0.7, 0.95] and bias in [0, 0.05]) is trained twice from
one seed, with the feature (learning rates 0.01 -> 0.001, upstream's) and without, the same number of iterations.

    python tools/exposure_quality.py [--seeds 0 1 2] [--iterations 600] [--json profiles/exposure_quality.json]

Per seed: the median training-view PSNR of the (compensated) render against the flickered frames, static region; how close the learned
per-channel log-gains (diagonal of E_f, centred over the frames: nothing pins the global colour scale) are to the applied ones, as a mean
absolute difference, beside the same measure for all-zero log-gains; the held-out static-region PSNR under both held-out policies
(reported only: the global scale decides its sign).  tests/test_gpu_exposure.py asserts the two orderings with this very function."""
import argparse
import copy
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ITERATIONS = 600   # (the depth term's end-to-end test trains 300; an exposure row gets a gradient once per epoch of 11 views)
SHAPE = dict(frames=12, W=128, H=48, focal=150.0, n_splats=3000)
PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def centred_log_gains(E):
    """[n, 3] log of the diagonal of every view's matrix, minus its mean over the views."""
    d = torch.stack([E[:, c, c] for c in range(3)], 1).double().clamp_min(1e-6).log()
    return d - d.mean(0, keepdim=True)


@torch.no_grad()
def train_view_psnrs(model, cams, masks):
    """PSNR of every training view's render — compensated with its own matrix when the model has them — against its (flickered) frame,
    over the static region."""
    from das3r_amd.losses import apply_exposure, psnr
    from das3r_amd.render import das3r_render
    from das3r_amd.train import resize_mask_nearest
    bg = torch.zeros(3, device=model.get_xyz.device)
    out = []
    for c in cams:
        img = das3r_render(c, model, PIPE, bg, camera_pose=model.get_RT(c.uid))["render"]
        if model._exposure is not None:
            img = apply_exposure(img, model._exposure.detach()[c.uid])
        static = 1 - resize_mask_nearest(torch.from_numpy(masks[c.frame_index]).to(img.device), img.shape[1], img.shape[2])
        out.append(float(psnr(img.clamp(0, 1) * static, c.original_image * static).mean()))
    return out


def measure(seed, iterations=ITERATIONS, device="cuda"):
    from das3r_amd import _lib
    from das3r_amd.model import OptimParams
    from das3r_amd.train import apply_flicker, build_from_sequence, consistent_sequence, psnr_report, train
    seq = consistent_sequence(seed=seed, device=device, **SHAPE)
    applied = apply_flicker(seq, seed)
    masks = seq["gt_dynamic_masks"]
    row = dict(seed=seed, iterations=iterations, shape=SHAPE)
    for name, (e0, e1) in (("with", (0.01, 0.001)), ("without", (0.0, 0.0))):
        model, cams, test = build_from_sequence(copy.deepcopy(seq), heldout=True)
        opt = OptimParams(iterations=iterations, exposure_lr_init=e0, exposure_lr_final=e1)
        model.training_setup(opt, fused=True)
        _lib.forget_shapes()
        dyn = {c.uid: torch.from_numpy(masks[c.frame_index]).to(device) for c in test}
        train(model, cams, opt, iterations, pipe=PIPE, seed=seed, fused=True, test_cameras=test, gt_dynamic_masks=dyn)
        ps = train_view_psnrs(model, cams, masks)
        res = dict(median_train_psnr=float(torch.tensor(ps).median()), train_psnrs=[round(p, 3) for p in ps])
        for policy in ("identity", "nearest"):
            res[f"heldout_psnr_{policy}"] = psnr_report(model, test, dynamic_masks=dyn, pipe=PIPE, test_poses=True, exposure=policy)["psnr"]
        if model._exposure is not None:
            want = centred_log_gains(applied[torch.tensor(model.exposure_frames, device=applied.device)])
            got = centred_log_gains(model._exposure.detach())
            res["log_gain_mad"] = float((got - want).abs().mean())
            res["log_gain_mad_of_identity"] = float(want.abs().mean())
        row[name] = res
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--iterations", type=int, default=ITERATIONS)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    rows = []
    for s in args.seeds:
        rows.append(measure(s, args.iterations))
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
