#!/usr/bin/env python3
"""What the trainable field of view (OptimParams.fov_lr) costs a fused train step, on one GPU.

    python tools/focal_bench.py [--out profiles/focal_train_step.jsonl] [--repeats 5] [--label this]

The method of tools/thin_bench.py `train`'s step figure: train.consistent_sequence at the Sintel shape (seed 0), the model as built with
the held-out split, 100 fused train steps after 20 warm-ups, HIP events around the hundred — here `--repeats` times per setting, each on a
freshly built model, so that the spread from run to run is on record beside the figures.  Settings:

    fov_lr 0            the default step (on a tree from before the feature, copied beside this one, the same rows are the parent's:
                        --label names the tree; the script only passes fov_lr where it is not 0)
    fov_lr 1e-3         the step with the focal kernel, the per-step read-back of FoVx / FoVy and the two more tensors of the gated launch
    fov_lr 1e-3, no read-back   the same with fast_step._read_fov answered from a value read once before the loop (the field of view the
                        step renders with then lags the parameter: a measurement, not a mode) — the difference is what the read-back costs
    kernels             focal_grad_kernel and focal_finish_kernel by the library's own event profiler, over 20 steps

One JSON line per (setting, repeat), appended as it is measured."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SINTEL = dict(frames=22, W=512, H=208, focal=600.0, n_splats=20000)
PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def build(seq, fov_lr):
    from das3r_amd import _lib
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence
    _lib.forget_shapes()
    model, cams, _ = build_from_sequence(seq, heldout=True)
    opt = OptimParams(iterations=600, **({"fov_lr": fov_lr} if fov_lr else {}))
    model.training_setup(opt, fused=True)
    return model, cams, opt


def step_ms(seq, fov_lr, cached_fov=False):
    from das3r_amd import fast_step
    from das3r_amd.train import train_step
    model, cams, opt = build(seq, fov_lr)
    bg = torch.zeros(3, device="cuda")
    real = getattr(fast_step, "_read_fov", None)
    try:
        if cached_fov:
            fixed = real(model)
            fast_step._read_fov = lambda m: fixed
        for it in range(1, 21):
            train_step(model, cams[it % len(cams)], opt, it, PIPE, bg, fused=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for it in range(21, 121):
            train_step(model, cams[it % len(cams)], opt, it, PIPE, bg, fused=True)
        b.record()
        b.synchronize()
    finally:
        if cached_fov:
            fast_step._read_fov = real
    return a.elapsed_time(b) / 100.0, int(model._xyz.shape[0])


def kernel_ms(seq, fov_lr, steps=20):
    from das3r_amd import _lib
    from das3r_amd.train import train_step
    model, cams, opt = build(seq, fov_lr)
    bg = torch.zeros(3, device="cuda")
    for it in range(1, 11):
        train_step(model, cams[it % len(cams)], opt, it, PIPE, bg, fused=True)
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(True)
    for it in range(11, 11 + steps):
        train_step(model, cams[it % len(cams)], opt, it, PIPE, bg, fused=True)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    rep = _lib.profile_report()
    return {k: round(ms / n, 5) for k, (n, ms) in rep.items() if k.startswith("focal_") or k.startswith("preprocess_backward") or k == "depth_fold_kernel"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="this", help="names the tree the rows are from (the parent commit's copy: parent)")
    ap.add_argument("--fov-lr", type=float, default=1e-3)
    ap.add_argument("--only-default", action="store_true", help="the fov_lr = 0 rows alone (a tree from before the feature)")
    args = ap.parse_args()
    from das3r_amd.train import consistent_sequence
    seq = consistent_sequence(seed=0, moving=True, **SINTEL)
    out = open(args.out, "a") if args.out else None

    def emit(row):
        row = dict(tree=args.label, shape="sintel consistent_sequence seed 0", **row)
        print(json.dumps(row), flush=True)
        if out:
            out.write(json.dumps(row) + "\n")
            out.flush()

    settings = [("fov_lr 0", 0.0, False)]
    if not args.only_default:
        settings += [(f"fov_lr {args.fov_lr:g}", args.fov_lr, False), (f"fov_lr {args.fov_lr:g}, no read-back", args.fov_lr, True)]
    for rep in range(args.repeats):   # (interleaved: a drift of the machine lands on every setting alike)
        for name, lr, cached in settings:
            ms, P = step_ms(seq, lr, cached)
            emit(dict(setting=name, repeat=rep, P=P, step_ms=round(ms, 4)))
            torch.cuda.empty_cache()
    if not args.only_default:
        emit(dict(setting=f"fov_lr {args.fov_lr:g} kernels", per_launch_ms=kernel_ms(seq, args.fov_lr)))


if __name__ == "__main__":
    main()
