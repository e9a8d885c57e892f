#!/usr/bin/env python3
"""What the mesh clean-up (das3r_amd.mesh) costs, on one GPU.

    python tools/mesh_bench.py [--out profiles/mesh_components.json] [--small]

mesh.components and mesh.filter_components with the HIP kernels against the torch form (components_torch, boolean-index filter) on the same
device in the same process, and against scipy's connected_components on the CPU, on two meshes: the mesh extracted from the fused 256^3 grid of
tools/tsdf_bench.py (about 120 k vertices, 238 k triangles) and a synthetic height field of about 2 M vertices and 4 M triangles with 1 000
octahedral debris blobs behind it.  Wall-clock medians after warm-ups with the device synchronised on both sides (every form reads counts back
to the host, so events alone would not cover it); the kernels' labels are compared with the torch form's and scipy's on the meshes they were
timed on; each launch's share is the library's own event timing.  --small: toy sizes, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def fused_mesh(small):
    from tsdf_bench import SHAPES, SMALL, scene
    from das3r_amd.tsdf import TSDFGrid
    shp = (SMALL if small else SHAPES)["sintel"]
    sc = scene(**shp)
    grid = TSDFGrid(sc["origin"], sc["voxel"], sc["dims"], device="cuda")
    grid.integrate(sc["depth"], sc["viewmatrix"], sc["tanfovx"], sc["tanfovy"], colour=sc["colour"], trunc=sc["trunc"], use_kernels=True)
    return grid.extract()


def height_field(n, blobs, device="cuda"):
    """n x n vertices of a relief, two triangles per cell, then `blobs` octahedra (6 vertices, 8 triangles each)"""
    i = torch.arange(n, device=device)
    jj, ii = torch.meshgrid(i, i, indexing="ij")
    v = torch.stack([ii.float(), jj.float(), 4.0 * torch.sin(ii * 0.01) * torch.cos(jj * 0.013)], -1).reshape(-1, 3)
    a = (jj[:-1, :-1] * n + ii[:-1, :-1]).reshape(-1)
    f = torch.cat([torch.stack([a, a + 1, a + n], 1), torch.stack([a + 1, a + n + 1, a + n], 1)], 1).reshape(-1, 3)
    octa = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], device=device)
    corners = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=torch.float32, device=device)
    g = torch.Generator(device=device).manual_seed(2)
    centres = torch.rand(blobs, 3, device=device, generator=g) * torch.tensor([n, n, 1.0], device=device) + torch.tensor([0.0, 0.0, 20.0], device=device)
    bv = (centres[:, None, :] + corners[None]).reshape(-1, 3)
    bf = (octa[None] + (n * n + 6 * torch.arange(blobs, device=device))[:, None, None]).reshape(-1, 3)
    vertices = torch.cat([v, bv], 0).contiguous()
    return dict(vertices=vertices, normals=torch.nn.functional.normalize(vertices, dim=1).contiguous(), colours=torch.rand_like(vertices),
                faces=torch.cat([f, bf], 0).to(torch.int32).contiguous())


def wall(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def scipy_components(faces_np, Nv):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    rows, cols = np.concatenate([faces_np[:, 0], faces_np[:, 1]]), np.concatenate([faces_np[:, 1], faces_np[:, 2]])
    n, lab = connected_components(coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(Nv, Nv)), directed=False)
    lowest = np.full(n, Nv, np.int64)
    np.minimum.at(lowest, lab, np.arange(Nv))
    return lowest[lab]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--torch-runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mesh_bench.py measures on a GPU; none is visible")
    from das3r_amd import _lib
    from das3r_amd.mesh import components, filter_components
    meshes = (("fused_256", lambda: fused_mesh(args.small), 100), ("height_field", lambda: height_field(64 if args.small else 1448, 20 if args.small else 1000), 100))
    rows = []
    for name, build, min_faces in meshes:
        mesh = build()
        faces, Nv, Nf = mesh["faces"], int(mesh["vertices"].shape[0]), int(mesh["faces"].shape[0])
        k = components(faces, Nv, use_kernels=True)
        t = components(faces, Nv, use_kernels=False)
        faces_np = faces.cpu().numpy().astype(np.int64)
        ref = scipy_components(faces_np, Nv)
        same = bool(torch.equal(k["vertex_label"].long(), t["vertex_label"]) and torch.equal(k["face_label"].long(), t["face_label"])
                    and torch.equal(k["_full"].long(), t["_full"]) and np.array_equal(k["vertex_label"].cpu().numpy(), ref))
        k_ms = wall(lambda: components(faces, Nv, use_kernels=True), 2, args.runs)
        t_ms = wall(lambda: components(faces, Nv, use_kernels=False), 1, args.torch_runs)
        t0 = time.perf_counter()
        scipy_components(faces_np, Nv)
        s_ms = (time.perf_counter() - t0) * 1e3
        fk, rep = filter_components(mesh, min_faces=min_faces, use_kernels=True)
        ft, _ = filter_components(mesh, min_faces=min_faces, use_kernels=False)
        same_filter = all(torch.equal(fk[a].view(torch.int32), ft[a].view(torch.int32)) for a in ("vertices", "normals", "colours", "faces"))
        fk_ms = wall(lambda: filter_components(mesh, min_faces=min_faces, use_kernels=True), 2, args.runs)
        ft_ms = wall(lambda: filter_components(mesh, min_faces=min_faces, use_kernels=False), 1, args.torch_runs)
        _lib.profile_report()
        _lib.profile_enable(True)
        for _ in range(args.runs):
            filter_components(mesh, min_faces=min_faces, use_kernels=True)
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        prof = {kn: round(ms / args.runs, 4) for kn, (n, ms) in _lib.profile_report().items() if kn.startswith(("mesh_", "prune_"))}
        total = sum(prof.values())
        km, tm, fkm, ftm = (statistics.median(x) for x in (k_ms, t_ms, fk_ms, ft_ms))
        rows.append(dict(mesh=name, vertices=Nv, faces=Nf, components=int(k["roots"].numel()), face_components=rep["components"],
                         components_kernels_ms_median=round(km, 3), components_kernels_ms_min=round(min(k_ms), 3),
                         components_torch_ms_median=round(tm, 3), components_torch_ms_min=round(min(t_ms), 3),
                         components_scipy_cpu_ms=round(s_ms, 3), components_speedup_over_torch=round(tm / km, 1),
                         filter_min_faces=min_faces, filter_kept_components=rep["kept_components"], filter_faces_after=rep["faces_after"],
                         filter_kernels_ms_median=round(fkm, 3), filter_kernels_ms_min=round(min(fk_ms), 3), filter_torch_ms_median=round(ftm, 3),
                         filter_torch_ms_min=round(min(ft_ms), 3), filter_speedup_over_torch=round(ftm / fkm, 1),
                         kernel_ms_per_call=prof, launch_share={kn: round(v / total, 3) for kn, v in prof.items()} if total else {},
                         labels_identical_to_torch_form_and_scipy=same, filter_identical_to_torch_form=same_filter))
        print(json.dumps(rows[-1]), flush=True)
        del mesh, k, t, fk, ft
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(what="mesh.components / mesh.filter_components with the HIP kernels vs the torch form on the same device and vs scipy's "
                                "connected_components on the CPU (tools/mesh_bench.py): wall-clock medians with the device synchronised on both sides "
                                "(host reads and output allocations included); filter times include the components; kernel_ms_per_call are the "
                                "library's own event timings summed over one filter_components call (mesh_flag_kernel, prune_scan_kernel and "
                                "prune_rank_kernel run twice in it, once for vertices and once for faces), launch_share their fractions of the sum",
                           meshes=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
