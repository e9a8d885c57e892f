"""Mesh clean-up without a device: the C-ABI surface and its refusals, the kernels' own union and find run serially on host memory
(das3r_debug_mesh_components_host) and the torch form on the CPU against the scipy reference (tests/mesh_reference.py) on every case, the keep
rule, the torch filter against the numpy filter, the offline flags and components.json."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # DAS3R_ERR_INVALID_ARG
SYMBOLS = ("das3r_mesh_components_workspace_bytes", "das3r_mesh_components", "das3r_mesh_filter_select", "das3r_mesh_filter_faces",
           "das3r_debug_mesh_components_host")
CASES = tuple(M.index_cases())


def test_symbols_header_and_abi(hip_lib):
    from das3r_amd import _lib
    for name in SYMBOLS:
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS, name
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "das3r_raster.h")).read()
    for name in SYMBOLS + ("smallest vertex index", "t = max(1, min_faces, c_K)", "shared VERTEX", "info[3]"):
        assert name in text, name
    mk = open(os.path.join(ROOT, "das3r_amd", "csrc", "Makefile")).read()
    assert "mesh.o" in mk.split("OBJS =")[1].split("\n")[0]
    plain = [ln for ln in mk.splitlines() if ln.startswith("api.o") and "%.o: %.hip" in ln][0]
    assert "mesh.o" in plain, "mesh.hip is integers only: the plain rule"


def test_refusals_need_no_device(hip_lib):
    fake = C.c_void_p(0x1000)   # never dereferenced: every call must stop at the argument checks
    host4, host2 = (C.c_int32 * 4)(), (C.c_int32 * 2)()
    err = lambda: hip_lib.das3r_last_error().decode()
    ws = hip_lib.das3r_mesh_components_workspace_bytes
    assert ws(-1, 0) == 0 and ws(0, -1) == 0 and ws((1 << 30) + 1, 0) == 0 and ws(0, (1 << 30) + 1) == 0
    assert ws(0, 0) > 0 and ws(1000, 3000) >= 4 * 1000 + 4 * (1 + 3) and ws(1 << 30, 1 << 30) > 0
    comp = lambda **o: hip_lib.das3r_mesh_components(*list(dict(dict(Nv=4, Nf=2, faces=fake, vl=fake, fl=fake, fc=fake, info=fake, host=host4, ws=fake), **o).values()),
                                                     None)
    for over in (dict(Nv=-1), dict(Nf=-1), dict(Nv=(1 << 30) + 1), dict(faces=None), dict(vl=None), dict(fl=None), dict(fc=None), dict(info=None),
                 dict(host=None), dict(ws=None), dict(ws=C.c_void_p(0x1002))):
        assert comp(**over) == INVALID and "das3r_mesh_components" in err(), over
    sel = lambda **o: hip_lib.das3r_mesh_filter_select(*list(dict(dict(Nv=4, Nf=2, vl=fake, fl=fake, fc=fake, t=1, vd=fake, fd=fake, tot=fake, host=host2, ws=fake),
                                                                  **o).values()), None)
    for over in (dict(Nv=-1), dict(Nf=-2), dict(t=0), dict(t=-5), dict(vl=None), dict(fl=None), dict(fc=None), dict(vd=None), dict(fd=None), dict(tot=None),
                 dict(host=None), dict(ws=None), dict(ws=C.c_void_p(0x1001))):
        assert sel(**over) == INVALID and "das3r_mesh_filter_select" in err(), over
    emit = lambda **o: hip_lib.das3r_mesh_filter_faces(*list(dict(dict(Nv=4, Nf=2, kv=3, kf=1, faces=fake, fd=fake, vd=fake, out=fake), **o).values()), None)
    for over in (dict(Nv=-1), dict(Nf=-1), dict(kv=5), dict(kv=-1), dict(kf=3), dict(kf=-1), dict(faces=None), dict(fd=None), dict(vd=None), dict(out=None)):
        assert emit(**over) == INVALID and "das3r_mesh_filter_faces" in err(), over
    assert emit(kf=0, faces=None, fd=None, vd=None, out=None) == 0, "an all-dropped mesh: no launch, no device"
    host = lambda **o: hip_lib.das3r_debug_mesh_components_host(*list(dict(dict(Nv=4, Nf=2, faces=fake, vl=fake, fl=fake, fc=fake, info=fake), **o).values()))
    for over in (dict(Nv=-1), dict(Nf=-1), dict(faces=None), dict(vl=None), dict(fl=None), dict(fc=None), dict(info=None)):
        assert host(**over) == INVALID, over


def host_components(lib, faces, Nv):
    """das3r_debug_mesh_components_host -> dict(vertex_label, face_label, full, info) as numpy int32"""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    Nf = f.shape[0]
    vl, fl, fc, info = np.full(Nv, -9, np.int32), np.full(Nf, -9, np.int32), np.full(Nv, -9, np.int32), np.full(4, -9, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = lib.das3r_debug_mesh_components_host(Nv, Nf, p(f), p(vl), p(fl), p(fc), p(info))
    assert rc == 0, lib.das3r_last_error()
    return dict(vertex_label=vl, face_label=fl, full=fc, info=info)


def torch_components(faces, Nv, device="cpu"):
    from das3r_amd.mesh import components
    c = components(torch.from_numpy(np.ascontiguousarray(faces)).to(device), Nv, use_kernels=False)
    assert c["path"] == "torch"
    vl = c["vertex_label"].cpu().numpy()
    full = c["_full"].cpu().numpy()
    roots = c["roots"].cpu().numpy()
    assert np.array_equal(roots, np.nonzero(vl == np.arange(Nv))[0]) and np.array_equal(c["face_count"].cpu().numpy(), full[roots])
    return dict(vertex_label=vl, face_label=c["face_label"].cpu().numpy(), full=full, info=[roots.size, int((full > 0).sum()), c["bad_faces"], 0])


@pytest.mark.parametrize("name", CASES)
def test_host_run_kernel_code_against_the_reference(hip_lib, name):
    f, Nv, _ = M.index_cases()[name]
    M.check_expectations(name, host_components(hip_lib, f, Nv))


@pytest.mark.parametrize("name", CASES)
def test_torch_form_against_the_reference(name):
    f, Nv, _ = M.index_cases()[name]
    M.check_expectations(name, torch_components(f, Nv))


def test_permutation_invariance(hip_lib):
    rng = np.random.default_rng(11)
    f, Nv = M.debris_mesh(True)["faces"], M.debris_mesh(True)["vertices"].shape[0]
    base = host_components(hip_lib, f, Nv)["vertex_label"]
    perm = rng.permutation(Nv)
    g = np.ascontiguousarray(perm[f][rng.permutation(f.shape[0])][:, rng.permutation(3)], np.int32)
    for got in (host_components(hip_lib, g, Nv), torch_components(g, Nv)):
        relabelled = got["vertex_label"][perm]   # the label of old vertex v, in new names
        assert M.same_partition(base, relabelled)
        assert np.array_equal(np.asarray(got["vertex_label"], np.int64), M.components(g, Nv)["vertex_label"])


@pytest.mark.parametrize("holed", [False, True])
def test_grid_meshes_have_the_stated_figures(hip_lib, holed):
    """The stated figures were computed with the float64 field; the float32 field is the one the kernels are fed, and there the reference
    extraction's own figures are the expectation (tests/mesh_reference.py DEBRIS_FIGURES says where the two differ)."""
    for dtype_name in ("float64", "float32"):
        fig = M.DEBRIS_FIGURES[dtype_name]["holed" if holed else "plain"]
        m = M.debris_mesh(holed, dtype_name)
        Nv, Nf = m["vertices"].shape[0], m["faces"].shape[0]
        ref = M.components(m["faces"], Nv)
        counts = sorted(ref["face_count"][ref["face_count"] > 0].tolist(), reverse=True)
        print(f"debris field ({dtype_name}, holed={holed}): {Nv} vertices, {Nf} faces, {ref['n_components']} components, face counts {counts}")
        assert (Nv, Nf, ref["n_components"], counts) == (fig["Nv"], fig["Nf"], fig["components"], fig["counts"]), dtype_name
        assert ref["n_components"] - ref["n_face_components"] == (2 if holed else 0), "unreferenced vertices"
        for got in (host_components(hip_lib, m["faces"], Nv), torch_components(m["faces"], Nv)):
            assert np.array_equal(got["vertex_label"], ref["vertex_label"]) and np.array_equal(got["face_label"], ref["face_label"])
            assert np.array_equal(got["full"], ref["full"]) and list(got["info"]) == [ref["n_components"], ref["n_face_components"], 0, 0]
        # connectivity by shared edge gives the same pieces on the extraction's meshes
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        f = m["faces"].astype(np.int64)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
        lo, hi = e.min(1), e.max(1)
        key, owner = np.unique(lo * Nv + hi, return_inverse=True)
        face_of = np.tile(np.arange(f.shape[0]), 3)
        order = np.argsort(owner, kind="stable")
        so, sf = owner[order], face_of[order]
        same = so[1:] == so[:-1]
        n_edge, _ = connected_components(coo_matrix((np.ones(same.sum(), np.int8), (sf[1:][same], sf[:-1][same])), shape=(f.shape[0],) * 2), directed=False)
        assert n_edge == ref["n_face_components"] == 7


def test_analytic_sphere_is_one_component(hip_lib):
    from tests import tsdf_reference as R
    t, w = R.analytic_sphere_grid()
    m = R.extract(t.astype(np.float32), w.astype(np.float32), None, np.zeros(3, np.float32), np.float32(1.0))
    Nv, f = m["vertices"].shape[0], np.ascontiguousarray(m["faces"], np.int32)
    assert (Nv, f.shape[0]) == (780, 1556)
    for got in (host_components(hip_lib, f, Nv), torch_components(f, Nv)):
        assert (got["vertex_label"] == 0).all() and (got["face_label"] == 0).all() and got["full"][0] == 1556 and list(got["info"]) == [1, 1, 0, 0]


def test_keep_threshold():
    from das3r_amd.mesh import keep_threshold
    c = torch.tensor([24, 5758, 0, 1068, 128, 88, 0, 48, 24])
    for (mf, K), t in {(0, 0): 1, (25, 0): 25, (0, 5): 48, (0, 6): 24, (0, 7): 24, (0, 1): 5758, (0, 100): 1, (6000, 0): 6000, (100, 5): 100,
                       (10, 2): 1068, (0, 8): 1}.items():
        assert keep_threshold(c, mf, K) == t == M.threshold(c.numpy(), mf, K), (mf, K)
    assert keep_threshold(torch.zeros(0, dtype=torch.int64), 0, 3) == 1 and keep_threshold([0, 0], 0, 1) == 1
    with pytest.raises(ValueError):
        keep_threshold(c, -1, 0)
    with pytest.raises(ValueError):
        keep_threshold(c, 0, -1)


def _torch_mesh(m, device="cpu"):
    return {k: torch.from_numpy(np.ascontiguousarray(m[k])).to(device) for k in ("vertices", "normals", "colours", "faces")}


def _np_mesh(m):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in m.items() if torch.is_tensor(v) or v is None}


@pytest.mark.parametrize("holed", [False, True])
@pytest.mark.parametrize("case", M.FILTER_CASES)
def test_torch_filter_against_the_numpy_filter(case, holed):
    from das3r_amd.mesh import filter_components
    m = M.debris_mesh(holed)
    mesh = dict(_torch_mesh(m), edge_mask=torch.zeros(1))
    out, rep = filter_components(mesh, *case, use_kernels=False)
    assert "edge_mask" not in out and rep["path"] == "torch"
    ref, t, kept = M.check_filtered(_np_mesh(out), m, *case)
    fig = M.DEBRIS_FIGURES["float32"]["holed" if holed else "plain"]
    assert rep["face_counts"] == fig["counts"] and rep["threshold"] == t and rep["kept_components"] == kept == M.FILTER_KEPT[case]
    assert rep["dropped_components"] == 7 - kept and rep["singletons"] == (2 if holed else 0) and rep["bad_faces"] == 0
    assert (rep["vertices_before"], rep["faces_before"]) == (fig["Nv"], fig["Nf"])
    assert (rep["vertices_after"], rep["faces_after"]) == (ref["vertices"].shape[0], ref["faces"].shape[0])
    assert rep["faces_after"] == sum(c for c in fig["counts"] if c >= t)
    if case == (0, 0):
        assert rep["faces_after"] == fig["Nf"] and rep["vertices_after"] == fig["Nv"] - (2 if holed else 0), "only the singletons go"
    if case == (6000, 0):
        assert out["faces"].shape == (0, 3) and out["vertices"].shape == (0, 3) and out["normals"].shape == (0, 3)


def test_filter_without_optional_attributes_and_with_bad_faces():
    from das3r_amd.mesh import filter_components
    f, Nv, _ = M.index_cases()["bad_faces"]
    v = np.arange(3 * Nv, dtype=np.float32).reshape(Nv, 3)
    mesh = dict(vertices=torch.from_numpy(v), normals=None, faces=torch.from_numpy(f))
    out, rep = filter_components(mesh, 0, 0, use_kernels=False)
    ref, _, _ = M.filter_mesh(dict(vertices=v, normals=None, colours=None, faces=f), 0, 0)
    assert rep["bad_faces"] == 8 and rep["faces_after"] == f.shape[0] - 8 and out["normals"] is None and out["colours"] is None
    assert np.array_equal(out["faces"].numpy(), ref["faces"]) and np.array_equal(out["vertices"].numpy(), ref["vertices"])
    with pytest.raises(RuntimeError, match="HIP device"):
        filter_components(mesh, 0, 0, use_kernels=True)
    from das3r_amd.mesh import components
    with pytest.raises(RuntimeError, match="HIP device"):
        components(torch.from_numpy(f), Nv, use_kernels=True)


def test_offline_flags(monkeypatch):
    from das3r_amd import io_formats, offline
    a = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert (a.tsdf_min_faces, a.tsdf_keep_largest) == (0, 0)
    a = offline.parser().parse_args(["-m", "x", "-s", "y", "--tsdf", "--tsdf-min-faces", "200", "--tsdf-keep-largest", "3"])
    assert (a.tsdf, a.tsdf_min_faces, a.tsdf_keep_largest) == (True, 200, 3)
    for bad in (["--tsdf-min-faces", "-1"], ["--tsdf-keep-largest", "-2"], ["--tsdf-min-faces", "1.5"]):
        with pytest.raises(SystemExit):
            offline.parser().parse_args(["-m", "x", "-s", "y", "--tsdf"] + bad)
    p = inspect.signature(offline.render_sets).parameters
    assert p["tsdf_min_faces"].default == 0 and p["tsdf_keep_largest"].default == 0
    p = inspect.signature(offline.fuse_and_mesh).parameters
    assert p["min_faces"].default == 0 and p["keep_largest"].default == 0
    seen = {}
    monkeypatch.setattr(io_formats, "load_sequence", lambda *a, **k: {"depths": None})
    monkeypatch.setattr(offline, "render_sets", lambda *a, **k: (seen.clear(), seen.update(k), (7, []))[2])
    offline.main(["-m", "x", "-s", "y", "--tsdf"])
    assert "tsdf_min_faces" not in seen and "tsdf_keep_largest" not in seen, "with the options off the program calls what it called"
    offline.main(["-m", "x", "-s", "y", "--tsdf", "--tsdf-min-faces", "0", "--tsdf-keep-largest", "0"])
    assert "tsdf_min_faces" not in seen and "tsdf_keep_largest" not in seen
    offline.main(["-m", "x", "-s", "y", "--tsdf", "--tsdf-keep-largest", "2"])
    assert seen["tsdf"] is True and seen["tsdf_keep_largest"] == 2 and seen["tsdf_min_faces"] == 0


def test_components_json_round_trip(tmp_path):
    from das3r_amd.mesh import filter_components, read_components_json, write_components_json
    m = M.debris_mesh(True)
    _, rep = filter_components(_torch_mesh(m), 25, 0, use_kernels=False)
    path = str(tmp_path / "components.json")
    write_components_json(path, rep)
    back = read_components_json(path)
    assert back == rep and back["face_counts"] == [5758, 1068, 128, 68, 48, 24, 24] and back["threshold"] == 25
    assert (back["kept_components"], back["dropped_components"], back["faces_after"]) == (5, 2, 7118 - 48)
