"""TSDF fusion and marching-tetrahedra extraction on the device (csrc/tsdf.hip) against the float64 reference (tests/tsdf_reference.py), the
torch form, and themselves; then the whole way from a model's renders to a mesh file.  The shapes are the smallest at which the kernels can go
wrong: one voxel, one short of and one past a wave, rows that end inside a workgroup, several workgroups, more views than a launch takes."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import tsdf_reference as R
from tests.test_tsdf_host import GRIDS, check_against_reference, check_mesh_against_reference, extraction_grids

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _scene(kind, dims):
    sc = (R.sphere_scene if kind == "sphere" else R.plane_scene)(dims)
    return sc, R.reference_of(sc)


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fuse(sc, views=None, one_by_one=False, use_kernels=True, device=DEV, grid=None):
    from das3r_amd.tsdf import TSDFGrid
    to = _cu if device == DEV else (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)))
    views = list(range(sc["depth"].shape[0])) if views is None else list(views)
    g = grid if grid is not None else TSDFGrid(sc["origin"], sc["voxel"], sc["dims"], device=device, colour=sc["colour_img"] is not None)
    pick = lambda a, idx: None if a is None else a[idx]
    for idx in ([[v] for v in views] if one_by_one else [views]):
        g.integrate(to(pick(sc["depth"], idx)), to(sc["viewmatrix"][idx]), sc["tanfovx"][idx], sc["tanfovy"][idx], colour=to(pick(sc["colour_img"], idx)),
                    weight=to(pick(sc["weight_img"], idx)), trunc=sc["trunc"], near=sc["near"], use_kernels=use_kernels)
    return g


def _np(g):
    return g.tsdf.cpu().numpy(), g.weight.cpu().numpy(), None if g.colour is None else g.colour.cpu().numpy()


def _same_bits(a, b):
    return all(x is y or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in ((a.tsdf, b.tsdf), (a.weight, b.weight), (a.colour, b.colour)))


# ---------------------------------------------------------------------------------------------------------------- integration
@pytest.mark.parametrize("kind", ["sphere", "plane"])
@pytest.mark.parametrize("dims", GRIDS)
def test_integrate_kernel_against_reference_and_torch_form(kind, dims):
    sc, ref = _scene(kind, dims)
    t, w, c = _np(_fuse(sc))
    check_against_reference(sc, t, w, c, ref, f"das3r_tsdf_integrate on the {kind}")
    # against integrate_torch run on the CPU: the same check on stable voxels
    tt, tw, tc = _np(_fuse(sc, use_kernels=False, device="cpu"))
    st = ~ref[3]
    assert np.array_equal((w > 0)[st], (tw > 0)[st])
    errs = [np.abs(w - tw)[st].max(initial=0.0), np.abs(t - tt)[st].max(initial=0.0), 0.0 if c is None else np.abs(c - tc)[:, st].max(initial=0.0)]
    print(f"kernel vs integrate_torch on the CPU, {kind} {dims}: weight / tsdf / colour {errs}; bit-identical: "
          f"{np.array_equal(t.view(np.uint32), tt.view(np.uint32)) and np.array_equal(w.view(np.uint32), tw.view(np.uint32))}")
    assert max(errs) <= 2e-5, errs


def test_integrate_batches_chunks_and_runs_are_bit_identical():
    from das3r_amd import _lib
    sc, _ = _scene("plane", (28, 26, 24))
    batch, single = _fuse(sc), _fuse(sc, one_by_one=True)
    assert _same_bits(batch, single), "a batch of four views == four calls of one"
    assert _same_bits(batch, _fuse(sc)), "two runs"
    sp, _ = _scene("sphere", (28, 26, 24))
    assert _same_bits(_fuse(sp), _fuse(sp, one_by_one=True)), "a batch of V = 6 == six calls of V = 1"
    many = [v % 6 for v in range(_lib.TSDF_MAX_VIEWS + 1)]   # one more view than a launch takes: two chunks
    assert _same_bits(_fuse(sp, views=many), _fuse(sp, views=many, one_by_one=True)), "V = cap + 1 == the one-by-one form"
    assert float(_fuse(sp, views=many).weight.max()) > 6.0, "the seventeenth view was taken"


def test_grid_outside_every_frustum_comes_back_untouched():
    from das3r_amd.tsdf import TSDFGrid
    sc, _ = _scene("plane", (28, 26, 24))
    g = TSDFGrid((40.0, -35.0, 50.0), sc["voxel"], (65, 3, 2), device=DEV)
    gen = torch.Generator().manual_seed(9)
    g.tsdf.copy_(torch.randn(g.tsdf.shape, generator=gen))
    g.weight.copy_(torch.rand(g.weight.shape, generator=gen))
    g.colour.copy_(torch.rand(g.colour.shape, generator=gen))
    g.tsdf[0, 0, 0], g.weight[0, 0, 1] = float("nan"), float("inf")
    before = [x.clone() for x in (g.tsdf, g.weight, g.colour)]
    _fuse(sc, grid=g)
    for a, b in zip(before, (g.tsdf, g.weight, g.colour)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_python_layer_refuses_what_the_kernel_cannot_take():
    from das3r_amd.tsdf import TSDFGrid, integrate_kernels
    sc, _ = _scene("sphere", (28, 26, 24))
    g = TSDFGrid(sc["origin"], sc["voxel"], sc["dims"], device=DEV, colour=False)
    with pytest.raises(RuntimeError, match="dense fp32"):
        integrate_kernels(g.tsdf.double(), g.weight, None, g.dims, g.origin, g.voxel, _cu(sc["depth"]), sc["viewmatrix"], 0.45, 0.4, trunc=0.16)
    with pytest.raises(ValueError, match="finite and > 0"):
        g.integrate(_cu(sc["depth"]), sc["viewmatrix"], 0.0, 0.4)
    with pytest.raises(ValueError, match="view matrices"):
        g.integrate(_cu(sc["depth"]), sc["viewmatrix"][:3], 0.45, 0.4)
    assert float(g.weight.max()) == 0.0, "nothing was launched"


# ---------------------------------------------------------------------------------------------------------------- extraction
def _extract(grid):
    from das3r_amd.tsdf import extract_kernels
    t, w, c, origin, voxel = grid
    nz, ny, nx = t.shape
    out = extract_kernels(_cu(t), _cu(w), _cu(c), (nx, ny, nz), origin, voxel)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["sphere", "sphere_holes", "zeros", "all_positive", "plane_70_5_3", "plane_9_1_8", "smooth_40_33_21"])
def test_extract_kernels_against_reference(name):
    grid = extraction_grids()[name]
    out = _extract(grid)
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    check_mesh_against_reference(name, got, grid)
    if name == "sphere":   # the closedness checks on the DEVICE's faces
        assert R.assert_closed(got["faces"]) == (780, 2334, 1556)
        n, ctr = R.triangle_normals(got["vertices"], got["faces"])
        assert (np.einsum("ij,ij->i", n, ctr - np.array([6.1, 5.9, 6.2])) > 0).all()
    if name == "all_positive":
        assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3)
    again = _extract(grid)
    for k, v in out.items():
        if v is None:
            assert again[k] is None
            continue
        a, b = (v.view(torch.int32), again[k].view(torch.int32)) if v.dtype == torch.float32 else (v, again[k])
        assert torch.equal(a, b), f"{name}: {k} differs between two runs"


def test_extract_of_a_fused_grid_closes_around_the_sphere():
    sc, _ = _scene("sphere", (28, 26, 24))
    g = _fuse(sc)
    m = g.extract()
    v, f = m["vertices"].cpu().numpy(), m["faces"].cpu().numpy()
    err = np.abs(np.linalg.norm(v - np.array(sc["centre"]), axis=1) - sc["radius"]) / sc["voxel"]
    print(f"device fusion + extraction of the sphere: {v.shape[0]} vertices, {f.shape[0]} triangles, radial error median {np.median(err):.3f}, "
          f"90th percentile {np.percentile(err, 90):.3f} voxel")
    assert np.median(err) <= 0.25 and np.percentile(err, 90) <= 0.75
    lo, hi = g.box()
    assert (v >= np.array(lo) - 1e-6).all() and (v <= np.array(hi) + 1e-6).all() and f.max() < v.shape[0]
    n = m["normals"].cpu().numpy()
    radial = (v - np.array(sc["centre"])) / np.linalg.norm(v - np.array(sc["centre"]), axis=1)[:, None]
    assert np.median(np.einsum("ij,ij->i", n, radial)) > 0.9, "the normals point to free space"


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_fuse_views_extract_and_save(tmp_path):
    from das3r_amd.io_formats import read_mesh_ply, save_mesh_ply
    from das3r_amd.rasterizer import median_depth_of
    from das3r_amd.render import das3r_render
    from das3r_amd.thin import pixel_footprint
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    from das3r_amd.tsdf import TSDFGrid, bounds_from_points, fuse_views, grid_for_box, view_matrix_of
    seq = synthetic_sequence(frames=6, W=128, H=80)
    model, cams = build_from_sequence(seq)
    voxel = 2.0 * pixel_footprint(seq["depths"], seq["K"])
    origin, dims = grid_for_box(*bounds_from_points(model._xyz, 0.01), voxel)
    grid = TSDFGrid(origin, voxel, dims, device=DEV)
    fuse_views(model, cams, None, None, grid)
    assert float(grid.weight.max()) > 1.0, "voxels seen by several views"
    mesh = grid.extract()
    Nv, Nf = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    assert Nv > 0 and Nf > 0
    lo, hi = grid.box()
    v = mesh["vertices"]
    assert bool((v >= torch.tensor(lo, device=DEV) - 1e-5).all()) and bool((v <= torch.tensor(hi, device=DEV) + 1e-5).all())
    assert int(mesh["faces"].max()) < Nv and int(mesh["faces"].min()) >= 0
    path = str(tmp_path / "mesh.ply")
    save_mesh_ply(path, v, mesh["faces"], normals=mesh["normals"], colours=mesh["colours"])
    back = read_mesh_ply(path)
    assert np.array_equal(back["vertices"], v.cpu().numpy()) and np.array_equal(back["faces"], mesh["faces"].cpu().numpy())
    assert back["colours"].shape == (Nv, 3) and np.array_equal(back["normals"], mesh["normals"].cpu().numpy())
    # recorded, not asserted: how far the mesh lies from the depth it was fused from
    import math
    gaps = []
    with torch.no_grad():
        for cam in cams:
            pose = model.get_RT(cam.uid)
            z = median_depth_of(das3r_render(cam, model, _pipe(), torch.zeros(3, device=DEV), camera_pose=pose, return_state=True)["raster_state"])[0]
            m = view_matrix_of(pose).reshape(4, 4).to(DEV)
            pc = v @ m[:3, :3] + m[3, :3]
            W, H = cam.image_width, cam.image_height
            px = torch.floor((pc[:, 0] / pc[:, 2] / math.tan(cam.FoVx / 2) + 1) * W / 2).long()
            py = torch.floor((pc[:, 1] / pc[:, 2] / math.tan(cam.FoVy / 2) + 1) * H / 2).long()
            ok = (pc[:, 2] > 0.01) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            d = z[py.clamp(0, H - 1), px.clamp(0, W - 1)]
            gap = (pc[:, 2] - d).abs()
            gaps.append(gap[ok & (d > 0) & (gap < grid.trunc)])
    gaps = torch.cat(gaps)
    print(f"end to end: {dims} voxels of edge {voxel:.4f}, {Nv} vertices, {Nf} triangles; median |vertex z - median depth| over {gaps.numel()} "
          f"(vertex, view) pairs closer than trunc: {float(gaps.median()):.5f} world units = {float(gaps.median()) / voxel:.3f} voxel")
    # fuse_views' other modes run and change what is fused
    g2 = TSDFGrid(origin, voxel, dims, device=DEV)
    fuse_views(model, cams[:2], None, None, g2, depth="blended", min_alpha=0.9, static_weight=True)
    assert float(g2.weight.max()) > 0 and not torch.equal(g2.weight, grid.weight)


def _pipe():
    from types import SimpleNamespace
    return SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def test_offline_tsdf_writes_the_mesh_and_the_grid(tmp_path):
    from das3r_amd import io_formats as io, offline
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.train import synthetic_sequence
    seq = synthetic_sequence(frames=6, W=128, H=80)
    data, out = str(tmp_path / "data" / "scene"), str(tmp_path / "job")
    io.write_sequence_dir(seq, data)
    assert run_sequence_job(0, 30, torch.device("cuda:0"), fused=True, seq=seq, out_dir=out)["ok"] == 1
    offline.main(["-m", out, "-s", data, "--fused", "--tsdf"])
    base = os.path.join(out, "interp", "ours_30")
    assert sorted(os.listdir(os.path.join(base, "tsdf"))) == ["mesh.ply", "tsdf.npz"] and len(os.listdir(os.path.join(base, "renders"))) == 6
    mesh = io.read_mesh_ply(os.path.join(base, "tsdf", "mesh.ply"))
    z = np.load(os.path.join(base, "tsdf", "tsdf.npz"))
    assert sorted(z.files) == ["colour", "origin", "trunc", "tsdf", "voxel", "weight"]
    assert mesh["vertices"].shape[0] > 0 and mesh["faces"].shape[0] > 0 and mesh["faces"].max() < mesh["vertices"].shape[0]
    assert mesh["normals"].shape == mesh["vertices"].shape and mesh["colours"].shape == mesh["vertices"].shape
    nz, ny, nx = z["tsdf"].shape
    assert z["weight"].shape == (nz, ny, nx) and z["colour"].shape == (3, nz, ny, nx) and float(z["trunc"]) == pytest.approx(4 * float(z["voxel"]))
    hi = z["origin"] + np.array([nx, ny, nz]) * float(z["voxel"])
    assert (mesh["vertices"] >= z["origin"] - 1e-5).all() and (mesh["vertices"] <= hi + 1e-5).all()
    # the file's grid gives the file's mesh: extraction is a function of the grid alone
    from das3r_amd.tsdf import extract_kernels
    again = extract_kernels(_cu(z["tsdf"]), _cu(z["weight"]), _cu(z["colour"]), (nx, ny, nz), z["origin"], float(z["voxel"]))
    assert np.array_equal(again["faces"].cpu().numpy(), mesh["faces"]) and np.array_equal(again["vertices"].cpu().numpy(), mesh["vertices"])
