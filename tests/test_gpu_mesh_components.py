"""Mesh clean-up on the device (csrc/mesh.hip) against the scipy reference (tests/mesh_reference.py), the kernels' own code run on the host,
the torch form and themselves; then from a fused grid with a planted blob to a cleaned mesh, and through the offline program.  The index-only
meshes are the smallest at which the union-find can go wrong: one face, one short of and one past a wave and a workgroup, deep chains (reversed
ids), a hub whose root keeps moving, many roots, faces that must not be read; one strip and the fans span many workgroups."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_reference as M
from tests.test_mesh_components_host import CASES, host_components, torch_components

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernel_components(faces, Nv):
    from das3r_amd.mesh import components
    c = components(_cu(faces), Nv, use_kernels=True)
    assert c["path"] == "kernels" and c["vertex_label"].dtype == torch.int32 and c["face_label"].dtype == torch.int32
    full, roots = c["_full"].cpu().numpy(), c["roots"].cpu().numpy()
    vl = c["vertex_label"].cpu().numpy()
    assert np.array_equal(roots, np.nonzero(vl == np.arange(Nv))[0]) and np.array_equal(c["face_count"].cpu().numpy(), full[roots])
    assert c["bad_faces"] == c["_info"][2]
    return dict(vertex_label=vl, face_label=c["face_label"].cpu().numpy(), full=full, info=c["_info"])


def _lib_handle():
    from das3r_amd import _lib
    return _lib.load()


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k], np.int64), np.asarray(b[k], np.int64)) for k in ("vertex_label", "face_label", "full")) \
        and [int(x) for x in a["info"]] == [int(x) for x in b["info"]]


@pytest.mark.parametrize("name", CASES)
def test_kernels_against_reference_host_twin_and_themselves(name):
    f, Nv, _ = M.index_cases()[name]
    got = kernel_components(f, Nv)
    assert int(got["info"][3]) == 0, "no loop gave up"
    M.check_expectations(name, got)
    assert _same(got, host_components(_lib_handle(), f, Nv)), f"{name}: the kernels and their own code on the host differ"
    assert _same(got, kernel_components(f, Nv)), f"{name}: two runs differ"


@pytest.mark.parametrize("name", ["two_share_vertex", "strip_257_perm", "combs", "bad_faces", "degenerate", "singletons"])
def test_torch_form_on_the_device_gives_the_same(name):
    f, Nv, _ = M.index_cases()[name]
    M.check_expectations(name, torch_components(f, Nv, device=DEV))


def test_permutation_invariance():
    rng = np.random.default_rng(11)
    m = M.debris_mesh(True)
    f, Nv = m["faces"], m["vertices"].shape[0]
    base = kernel_components(f, Nv)["vertex_label"]
    perm = rng.permutation(Nv)
    g = np.ascontiguousarray(perm[f][rng.permutation(f.shape[0])][:, rng.permutation(3)], np.int32)
    got = kernel_components(g, Nv)
    assert M.same_partition(base, got["vertex_label"][perm])
    assert np.array_equal(got["vertex_label"].astype(np.int64), M.components(g, Nv)["vertex_label"])


def _extract_device(t, w):
    from das3r_amd.tsdf import extract_kernels
    nz, ny, nx = t.shape
    out = extract_kernels(_cu(t), _cu(w), None, (nx, ny, nz), (0.0, 0.0, 0.0), 1.0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("holed", [False, True])
def test_grid_meshes_through_the_device_extraction(holed):
    """The float32 field is fed to the reference extraction and to TSDFGrid's kernels alike; the reference's figures are the expectation."""
    m = M.debris_mesh(holed)
    fig = M.DEBRIS_FIGURES["float32"]["holed" if holed else "plain"]
    mesh = _extract_device(m["tsdf"], m["weight"])
    faces = mesh["faces"].cpu().numpy()
    Nv = mesh["vertices"].shape[0]
    assert np.array_equal(faces, m["faces"]) and Nv == m["vertices"].shape[0] == fig["Nv"] and faces.shape[0] == fig["Nf"]
    from das3r_amd.mesh import components
    c = components(mesh["faces"], Nv)
    assert c["path"] == "kernels", "the kernels are the default on a HIP device"
    ref = M.components(faces, Nv)
    got = dict(vertex_label=c["vertex_label"].cpu().numpy(), face_label=c["face_label"].cpu().numpy(), full=c["_full"].cpu().numpy(), info=c["_info"])
    assert _same(got, dict(vertex_label=ref["vertex_label"], face_label=ref["face_label"], full=ref["full"],
                           info=[ref["n_components"], ref["n_face_components"], 0, 0]))
    assert sorted(c["face_count"][c["face_count"] > 0].tolist(), reverse=True) == fig["counts"] and len(c["roots"]) == fig["components"]
    assert _same(got, host_components(_lib_handle(), faces, Nv))


def test_analytic_sphere_is_one_component():
    from tests import tsdf_reference as R
    t, w = R.analytic_sphere_grid()
    mesh = _extract_device(t.astype(np.float32), w.astype(np.float32))
    assert (mesh["vertices"].shape[0], mesh["faces"].shape[0]) == (780, 1556)
    got = kernel_components(mesh["faces"].cpu().numpy(), 780)
    assert (got["vertex_label"] == 0).all() and (got["face_label"] == 0).all() and got["full"][0] == 1556 and list(got["info"]) == [1, 1, 0, 0]


def _torch_mesh(m):
    return {k: _cu(m[k]) for k in ("vertices", "normals", "colours", "faces")}


def _np_mesh(m):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in m.items() if torch.is_tensor(v) or v is None}


@pytest.mark.parametrize("holed", [False, True])
@pytest.mark.parametrize("case", M.FILTER_CASES)
def test_filter_with_kernels_equals_the_numpy_filter(case, holed):
    from das3r_amd.mesh import filter_components
    m = M.debris_mesh(holed)
    mesh = dict(_torch_mesh(m), edge_mask=torch.zeros(1, device=DEV))
    out, rep = filter_components(mesh, *case, use_kernels=True)
    assert "edge_mask" not in out and rep["path"] == "kernels"
    ref, t, kept = M.check_filtered(_np_mesh(out), m, *case)
    fig = M.DEBRIS_FIGURES["float32"]["holed" if holed else "plain"]
    assert rep["face_counts"] == fig["counts"] and rep["threshold"] == t and rep["kept_components"] == kept == M.FILTER_KEPT[case]
    assert rep["singletons"] == (2 if holed else 0) and rep["bad_faces"] == 0
    assert (rep["vertices_after"], rep["faces_after"]) == (ref["vertices"].shape[0], ref["faces"].shape[0])
    if case == (6000, 0):
        assert out["faces"].shape == (0, 3) and out["vertices"].shape == (0, 3) and out["colours"].shape == (0, 3)
    # use_kernels=False on the device, and the default, give the same arrays and the same report
    for use in (False, None):
        again, rep2 = filter_components(mesh, *case, use_kernels=use)
        M.check_filtered(_np_mesh(again), m, *case)
        assert {k: v for k, v in rep2.items() if k != "path"} == {k: v for k, v in rep.items() if k != "path"}
        assert rep2["path"] == ("torch" if use is False else "kernels")
    twice, _ = filter_components(mesh, *case, use_kernels=True)
    for k in ("vertices", "normals", "colours", "faces"):
        assert torch.equal(twice[k].view(torch.int32), out[k].view(torch.int32)), f"two runs differ in {k}"


def test_filter_with_bad_faces_and_without_optional_attributes():
    from das3r_amd.mesh import filter_components
    f, Nv, _ = M.index_cases()["bad_faces"]
    v = np.arange(3 * Nv, dtype=np.float32).reshape(Nv, 3)
    out, rep = filter_components(dict(vertices=_cu(v), normals=None, faces=_cu(f)), 0, 1, use_kernels=True)
    ref, _, _ = M.filter_mesh(dict(vertices=v, normals=None, colours=None, faces=f), 0, 1)
    assert rep["bad_faces"] == 8 and rep["kept_components"] == 2 and rep["faces_after"] == f.shape[0] - 8 and out["normals"] is None
    assert np.array_equal(out["faces"].cpu().numpy(), ref["faces"]) and np.array_equal(out["vertices"].cpu().numpy(), ref["vertices"])
    empty, rep = filter_components(dict(vertices=_cu(v[:5]), faces=torch.zeros(0, 3, dtype=torch.int32, device=DEV)), 0, 0, use_kernels=True)
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and rep["singletons"] == 5 and rep["components"] == 0
    with pytest.raises(RuntimeError, match="int32"):
        filter_components(dict(vertices=_cu(v), faces=_cu(f).long()), 0, 0, use_kernels=True)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _plant_blob(grid, block=6, margin=2):
    """One far-off blob, built as the debris field's balls are: a ball of radius 1.2 voxels inside a block of `block`^3 voxels of weight 1, placed
    where no inside voxel lies within `margin` voxels of the block (so no vertex outside the block changes, normals included).
    -> (lo, hi) world corners of the block"""
    inside = ((grid.weight > 0) & torch.isfinite(grid.tsdf) & (grid.tsdf < 0)).float()[None, None]
    win = block + 2 * margin
    busy = torch.nn.functional.max_pool3d(inside, win, stride=1)[0, 0]
    free = torch.nonzero(busy == 0)
    assert free.shape[0] > 0, "no free block in the grid"
    k0, j0, i0 = (int(x) + margin for x in free[-1])
    ax = torch.arange(block, dtype=torch.float32, device=grid.tsdf.device) + 0.5
    Z, Y, X = torch.meshgrid(ax, ax, ax, indexing="ij")
    d = torch.sqrt((X - 3.1) ** 2 + (Y - 2.9) ** 2 + (Z - 3.2) ** 2) - 1.2
    grid.tsdf[k0:k0 + block, j0:j0 + block, i0:i0 + block] = (d / 4.0).clamp(-1.0, 1.0)
    grid.weight[k0:k0 + block, j0:j0 + block, i0:i0 + block] = 1.0
    lo = np.array(grid.origin) + np.array([i0, j0, k0]) * grid.voxel
    return lo, lo + block * grid.voxel


def test_planted_blob_is_removed_and_the_surface_keeps_its_bits(tmp_path):
    from das3r_amd.io_formats import read_mesh_ply, save_mesh_ply
    from das3r_amd.mesh import filter_components
    from das3r_amd.thin import pixel_footprint
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    from das3r_amd.tsdf import TSDFGrid, bounds_from_points, fuse_views, grid_for_box
    seq = synthetic_sequence(frames=6, W=128, H=80)
    model, cams = build_from_sequence(seq)
    voxel = 2.0 * pixel_footprint(seq["depths"], seq["K"])
    origin, dims = grid_for_box(*bounds_from_points(model._xyz, 0.01), voxel, pad=24)   # room beside the surface for a far-off blob
    grid = TSDFGrid(origin, voxel, dims, device=DEV)
    fuse_views(model, cams, None, None, grid)
    before = grid.extract()
    lo, hi = _plant_blob(grid)
    after = grid.extract()
    v = after["vertices"].cpu().numpy()
    in_blob = ((v >= lo) & (v <= hi)).all(axis=1)
    ref = M.components(after["faces"].cpu().numpy(), v.shape[0])
    blob_labels = np.unique(ref["vertex_label"][in_blob])
    assert in_blob.sum() > 0 and blob_labels.size == 1, "the blob is one piece of its own"
    blob_faces = int(ref["full"][blob_labels[0]])
    assert after["faces"].shape[0] == before["faces"].shape[0] + blob_faces and in_blob.sum() == v.shape[0] - before["vertices"].shape[0]
    assert (ref["vertex_label"][~in_blob] != blob_labels[0]).all()
    t = blob_faces + 1
    cleaned, rep = filter_components(after, min_faces=t)
    base, rep0 = filter_components(before, min_faces=t)
    print(f"end to end: {dims} voxels, {v.shape[0]} vertices, {after['faces'].shape[0]} faces in {rep['components']} pieces {rep['face_counts'][:8]}; "
          f"the blob has {blob_faces} faces; min faces {t} keeps {rep['kept_components']} pieces, {rep['faces_after']} faces")
    assert rep["path"] == "kernels" and rep["components"] == rep0["components"] + 1 and rep["dropped_components"] == rep0["dropped_components"] + 1
    assert rep["kept_components"] == rep0["kept_components"] >= 1 and rep["face_counts"][0] >= t, "the main surface stays"
    for k in ("vertices", "normals", "colours", "faces"):
        assert torch.equal(cleaned[k].view(torch.int32), base[k].view(torch.int32)), f"{k}: the rows that stay are not the parent mesh's, bit for bit"
    cv = cleaned["vertices"].cpu().numpy()
    assert not ((cv >= lo) & (cv <= hi)).all(axis=1).any(), "a vertex of the blob is left"
    M.check_filtered(_np_mesh(cleaned), _np_mesh(after), t, 0)
    path = str(tmp_path / "mesh.ply")
    save_mesh_ply(path, cleaned["vertices"], cleaned["faces"], normals=cleaned["normals"], colours=cleaned["colours"])
    back = read_mesh_ply(path)
    assert np.array_equal(back["faces"], cleaned["faces"].cpu().numpy()) and np.array_equal(back["vertices"], cv)


def test_offline_options_off_is_byte_identical_and_on_writes_the_report(tmp_path):
    from das3r_amd import io_formats as io, offline
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.mesh import read_components_json
    from das3r_amd.train import synthetic_sequence
    seq = synthetic_sequence(frames=6, W=128, H=80)
    data, out = str(tmp_path / "data" / "scene"), str(tmp_path / "job")
    io.write_sequence_dir(seq, data)
    assert run_sequence_job(0, 30, torch.device("cuda:0"), fused=True, seq=seq, out_dir=out)["ok"] == 1
    tsdf_dir = os.path.join(out, "interp", "ours_30", "tsdf")
    ply = os.path.join(tsdf_dir, "mesh.ply")
    offline.main(["-m", out, "-s", data, "--fused", "--tsdf"])
    plain = open(ply, "rb").read()
    assert sorted(os.listdir(tsdf_dir)) == ["mesh.ply", "tsdf.npz"]
    offline.main(["-m", out, "-s", data, "--fused", "--tsdf", "--tsdf-min-faces", "0", "--tsdf-keep-largest", "0"])
    assert open(ply, "rb").read() == plain and sorted(os.listdir(tsdf_dir)) == ["mesh.ply", "tsdf.npz"]
    raw = io.read_mesh_ply(ply)
    offline.main(["-m", out, "-s", data, "--fused", "--tsdf", "--tsdf-keep-largest", "1"])
    assert sorted(os.listdir(tsdf_dir)) == ["components.json", "mesh.ply", "tsdf.npz"]
    rep = read_components_json(os.path.join(tsdf_dir, "components.json"))
    mesh = io.read_mesh_ply(ply)
    ref, t, kept = M.filter_mesh(dict(vertices=raw["vertices"], normals=raw["normals"], colours=raw["colours"], faces=raw["faces"]), 0, 1)
    assert rep["threshold"] == t == rep["face_counts"][0] and rep["kept_components"] == kept and rep["keep_largest"] == 1 and rep["min_faces"] == 0
    assert (rep["vertices_before"], rep["faces_before"]) == (raw["vertices"].shape[0], raw["faces"].shape[0])
    assert (rep["vertices_after"], rep["faces_after"]) == (mesh["vertices"].shape[0], mesh["faces"].shape[0])
    assert np.array_equal(mesh["faces"], ref["faces"]) and M.same_bits(mesh["vertices"], ref["vertices"]) and M.same_bits(mesh["normals"], ref["normals"])
    assert np.array_equal(mesh["colours"], ref["colours"])
