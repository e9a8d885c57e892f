#!/usr/bin/env python3
"""train-step ms of the DAS3R hot loop (render + masked L1/SSIM loss + backward + two Adam steps), on a synthetic sequence
with the shape real DAS3R training has: every pixel of every frame is one Gaussian, frames 512x208.

    python tools/train_bench.py [--frames 20 --W 512 --H 208 --iters 50] [--fused-adam] [--breakdown]
Prints one JSON line: {"train_step_ms": ..., "splats": P, "iters_per_s": ..., "breakdown_ms": {...}}.

    python tools/train_bench.py --frames 22 --fused-adam --fused-pre --dynamic-fraction 0.25 --prune-min-opacity 0.005
what a job gains from pruning (das3r_amd.prune): a rectangle of that share of every frame is dynamic (dyna_avg = 1: those Gaussians are
rendered at opacity 0 from iteration 1), and the step is timed on the warmed-up model and on a copy of it after one prune event, the two
alternating for --rounds rounds — "prune": {"before_ms": [...], "after_ms": [...], "splats_after": ...} in the JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--W", type=int, default=512)
    ap.add_argument("--H", type=int, default=208)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fused-adam", action="store_true")
    ap.add_argument("--fused-loss", action="store_true")
    ap.add_argument("--fused-pre", action="store_true")
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--depth", default="noise", choices=("noise", "smooth"), help="depth maps of the synthetic sequence (das3r_amd.train.synthetic_sequence)")
    ap.add_argument("--depth-l1", nargs=2, type=float, default=(0.0, 0.0), metavar=("INIT", "FINAL"), help="time the depth-supervised step: weights of the "
                    "inverse-depth L1 term (OptimParams.depth_l1_weight_init / _final; upstream 3DGS: 1.0 0.01); the cameras then carry the sequence's depth maps")
    ap.add_argument("--exposure-lr", nargs=2, type=float, default=(0.0, 0.0), metavar=("INIT", "FINAL"), help="time the step with per-frame exposure "
                    "compensation: learning rates of the exposure group (OptimParams.exposure_lr_init / _final; upstream 3DGS: 0.01 0.001)")
    ap.add_argument("--dynamic-fraction", type=float, default=0.0, help="mark a rectangle of this share of every frame dynamic (dyna_avg = 1) before the "
                    "model is built (the synthetic sequences' own moving disc covers about 2 %% of a frame)")
    ap.add_argument("--prune-min-opacity", type=float, default=0.0, help="> 0: also time the step after one prune event at this threshold "
                    "(das3r_amd.prune.prune_points), alternating with the unpruned model")
    ap.add_argument("--rounds", type=int, default=3, help="with --prune-min-opacity: alternations of (unpruned, pruned), --iters steps each")
    args = ap.parse_args()
    from types import SimpleNamespace
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence, train_step
    seq = synthetic_sequence(frames=args.frames, W=args.W, H=args.H, focal=600.0, n_splats=20000, seed=0, depth=args.depth)
    if args.dynamic_fraction > 0:   # a centred rectangle with the frame's aspect ratio
        f = min(args.dynamic_fraction, 1.0) ** 0.5
        h, w = max(1, round(args.H * f)), max(1, round(args.W * f))
        y0, x0 = (args.H - h) // 2, (args.W - w) // 2
        seq["dyna_avg"][:, y0:y0 + h, x0:x0 + w] = 1.0
    w0, w1 = args.depth_l1
    model, cams = build_from_sequence(seq, depth_targets=w0 > 0 or w1 > 0)
    e0, e1 = args.exposure_lr
    opt = OptimParams(iterations=4000, depth_l1_weight_init=w0, depth_l1_weight_final=w1, exposure_lr_init=e0, exposure_lr_final=e1)
    model.training_setup(opt, fused=args.fused_adam) if args.fused_adam else model.training_setup(opt)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device="cuda")
    kw = dict(fused=True) if args.fused_pre else {}
    for it in range(1, args.warmup + 1):
        train_step(model, cams[it % len(cams)], opt, it, pipe, bg, **kw)
    torch.cuda.synchronize()

    def timed(m, first):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(first, first + args.iters):
            train_step(m, cams[it % len(cams)], opt, it, pipe, bg, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters * 1e3

    ms = timed(model, args.warmup + 1)
    pruning = None
    if args.prune_min_opacity > 0:
        import copy
        from das3r_amd.prune import prune_points
        model.__dict__.pop("_fast_state", None)   # (per-model buffers of the direct iteration, rebuilt on demand)
        pruned = copy.deepcopy(model)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = prune_points(pruned, min_opacity=args.prune_min_opacity)
        torch.cuda.synchronize()
        event_ms = (time.perf_counter() - t0) * 1e3
        nxt = args.warmup + args.iters + 1
        for m in (model, pruned):   # a warm-up of each: the pruned model is a new shape to the library
            for it in range(nxt, nxt + args.warmup):
                train_step(m, cams[it % len(cams)], opt, it, pipe, bg, **kw)
        nxt += args.warmup
        before, after = [], []
        for _ in range(args.rounds):
            before.append(round(timed(model, nxt), 3))
            after.append(round(timed(pruned, nxt), 3))
            nxt += args.iters
        pruning = dict(min_opacity=args.prune_min_opacity, dynamic_fraction=args.dynamic_fraction, path=info["path"], splats_before=info["before"],
                       splats_after=info["after"], first_event_ms=round(event_ms, 3), before_ms=before, after_ms=after)
    out = {"train_step_ms": round(ms, 3), "splats": int(model.get_xyz.shape[0]), "frames": args.frames, "image": [args.W, args.H],
           "iters_per_s": round(1e3 / ms, 2), "fused_adam": bool(args.fused_adam), "fused_pre": bool(args.fused_pre),
           "depth_l1": [w0, w1], "exposure_lr": [e0, e1]}
    if pruning is not None:
        out["prune"] = pruning
    if args.breakdown:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for it in range(1000, 1005):
                train_step(model, cams[it % len(cams)], opt, it, pipe, bg, **kw)
            torch.cuda.synchronize()
        rows = sorted(prof.key_averages(), key=lambda e: -e.device_time_total)[:40]
        out["breakdown_ms"] = {r.key[:60]: round(r.device_time_total / 5 / 1e3, 3) for r in rows}
        out["kernel_launches_per_step"] = sum(r.count for r in prof.key_averages()) / 5
        out["device_ms_per_step"] = round(sum(r.device_time_total for r in prof.key_averages()) / 5 / 1e3, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
