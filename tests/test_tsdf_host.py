"""TSDF fusion and mesh export without a device: the C-ABI surface and its refusals, the torch form of the integration (fp32, on the CPU)
and the kernels' own per-voxel code run on host memory against the float64 reference, the mesh PLY, the offline flags."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import tsdf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # DAS3R_ERR_INVALID_ARG
SYMBOLS = ("das3r_tsdf_integrate", "das3r_tsdf_extract_workspace_bytes", "das3r_tsdf_extract_count", "das3r_tsdf_extract_emit",
           "das3r_debug_tsdf_integrate_host", "das3r_debug_tsdf_extract_host", "das3r_debug_tsdf_swap_table")
GRIDS = ((1, 1, 1), (63, 1, 1), (65, 3, 2), (28, 26, 24), (130, 5, 3))


def test_symbols_header_and_abi(hip_lib):
    from das3r_amd import _lib
    for name in SYMBOLS:
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS, name
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "das3r_raster.h")).read()
    for name in SYMBOLS + ("DAS3R_TSDF_MAX_VIEWS", "DAS3R_TSDF_MAX_VOXELS", "xyz, xzy, yxz, yzx, zxy, zyx", "+x, +y, +z, +x+y, +x+z, +y+z, +x+y+z"):
        assert name in text, name
    mk = open(os.path.join(ROOT, "das3r_amd", "csrc", "Makefile")).read()
    assert "tsdf.o" in mk.split("OBJS =")[1].split("\n")[0]
    exact = [ln for ln in mk.splitlines() if ln.startswith("preprocess.o") and "%.o: %.hip" in ln][0]
    assert "tsdf.o" in exact, "tsdf.hip is compiled without FMA contraction (the EXACT rule)"
    assert _lib.TSDF_MAX_VIEWS == 16 and _lib.TSDF_MAX_VOXELS == 1 << 28


def _integrate_args(**over):
    fake = C.c_void_p(0x1000)   # never dereferenced: every call must stop at the argument checks
    a = dict(dims=(C.c_int32 * 3)(4, 4, 4), origin=(C.c_float * 3)(0, 0, 0), voxel=C.c_float(0.1), tsdf=fake, weight=fake, colour=None, V=1,
             viewmatrix=fake, tanfovx=(C.c_float * 1)(0.5), tanfovy=(C.c_float * 1)(0.5), H=8, W=8, depth=fake, colour_img=None, weight_img=None,
             trunc=C.c_float(0.4), near=C.c_float(0.01))
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over, text", [
    (dict(tsdf=None), "required"), (dict(weight=None), "required"), (dict(depth=None), "required"),
    (dict(voxel=C.c_float(0.0)), "voxel"), (dict(voxel=C.c_float(-1.0)), "voxel"), (dict(voxel=C.c_float(float("nan"))), "voxel"),
    (dict(voxel=C.c_float(float("inf"))), "voxel"),
    (dict(trunc=C.c_float(0.0)), "trunc"), (dict(trunc=C.c_float(float("nan"))), "trunc"), (dict(trunc=C.c_float(float("inf"))), "trunc"),
    (dict(tanfovx=(C.c_float * 1)(0.0)), "tanfov"), (dict(tanfovy=(C.c_float * 1)(-0.5)), "tanfov"), (dict(tanfovx=(C.c_float * 1)(float("nan"))), "tanfov"),
    (dict(tanfovy=(C.c_float * 1)(float("inf"))), "tanfov"),
    (dict(dims=(C.c_int32 * 3)(0, 4, 4)), "dim"), (dict(dims=(C.c_int32 * 3)(4, 4, -1)), "dim"),
    (dict(dims=(C.c_int32 * 3)(1 << 14, 1 << 14, 2)), "2^28"), (dict(dims=(C.c_int32 * 3)(1 << 30, 1 << 30, 1 << 30)), "2^28"),
    (dict(colour_img=C.c_void_p(0x1000)), "colour"), (dict(colour=C.c_void_p(0x1000)), "colour"),
])
def test_integrate_refusals_need_no_device(hip_lib, over, text):
    rc = hip_lib.das3r_tsdf_integrate(*_integrate_args(**over), None)
    assert rc == INVALID and text in hip_lib.das3r_last_error().decode(), hip_lib.das3r_last_error()


def test_extract_refusals_need_no_device(hip_lib):
    fake = C.c_void_p(0x1000)
    good, org = (C.c_int32 * 3)(4, 4, 4), (C.c_float * 3)(0, 0, 0)
    err = lambda: hip_lib.das3r_last_error().decode()
    assert hip_lib.das3r_tsdf_extract_workspace_bytes(good) == 12 * 64 + 8
    assert hip_lib.das3r_tsdf_extract_workspace_bytes((C.c_int32 * 3)(130, 5, 3)) == 12 * 1950 + 8 * 8
    for bad in ((0, 4, 4), (4, -2, 4), (1 << 14, 1 << 14, 2)):
        d = (C.c_int32 * 3)(*bad)
        assert hip_lib.das3r_tsdf_extract_workspace_bytes(d) == 0
        assert hip_lib.das3r_tsdf_extract_count(d, fake, fake, fake, fake, None) == INVALID and ("dim" in err() or "2^28" in err())
        assert hip_lib.das3r_tsdf_extract_emit(d, org, C.c_float(1.0), fake, fake, None, fake, 3, 1, fake, fake, None, fake, None) == INVALID
    assert hip_lib.das3r_tsdf_extract_workspace_bytes((C.c_int32 * 3)(1 << 14, 1 << 14, 1)) > 0, "2^28 voxels themselves are accepted"
    for args in ((good, None, fake, fake, fake), (good, fake, None, fake, fake), (good, fake, fake, None, fake), (good, fake, fake, fake, None),
                 (good, fake, fake, C.c_void_p(0x1002), fake)):
        assert hip_lib.das3r_tsdf_extract_count(*args, None) == INVALID, args
    emit = lambda **o: hip_lib.das3r_tsdf_extract_emit(*list(dict(dict(dims=good, origin=org, voxel=C.c_float(1.0), tsdf=fake, weight=fake, colour=None,
                                                                       ws=fake, Nv=3, Nf=1, vertices=fake, normals=fake, colours=None, faces=fake), **o).values()), None)
    for over in (dict(tsdf=None), dict(ws=None), dict(voxel=C.c_float(0.0)), dict(voxel=C.c_float(float("nan"))), dict(Nv=-1), dict(Nf=-1),
                 dict(vertices=None), dict(normals=None), dict(faces=None), dict(colour=fake), dict(colours=fake), dict(origin=None)):
        assert emit(**over) == INVALID, over
    assert emit(Nv=0, Nf=0, vertices=None, normals=None, faces=None) == 0, "an empty surface: no launch, no device"


# ---------------------------------------------------------------------------------------------------------------- integration
def _tt(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _torch_grid(sc):
    from das3r_amd.tsdf import TSDFGrid
    g = TSDFGrid(sc["origin"], sc["voxel"], sc["dims"], device="cpu", colour=sc["colour_img"] is not None)
    return g.integrate(_tt(sc["depth"]), _tt(sc["viewmatrix"]), sc["tanfovx"], sc["tanfovy"], colour=_tt(sc["colour_img"]), weight=_tt(sc["weight_img"]),
                       trunc=sc["trunc"], near=sc["near"])


def _host_kernel_grid(lib, sc):
    nx, ny, nz = sc["dims"]
    has = sc["colour_img"] is not None
    t, w = np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)
    c = np.zeros((3, nz, ny, nx), np.float32) if has else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    V = sc["depth"].shape[0]
    arrs = [np.ascontiguousarray(sc[k], np.float32) if sc[k] is not None else None for k in ("viewmatrix", "depth", "colour_img", "weight_img")]
    rc = lib.das3r_debug_tsdf_integrate_host((C.c_int32 * 3)(nx, ny, nz), (C.c_float * 3)(*sc["origin"]), C.c_float(sc["voxel"]), p(t), p(w), p(c), V,
                                             p(arrs[0]), (C.c_float * V)(*sc["tanfovx"]), (C.c_float * V)(*sc["tanfovy"]), sc["H"], sc["W"], p(arrs[1]),
                                             p(arrs[2]), p(arrs[3]), C.c_float(sc["trunc"]), C.c_float(sc["near"]))
    assert rc == 0, lib.das3r_last_error()
    return t, w, c


def check_against_reference(sc, t, w, c, ref, what):
    """The checks every form of the integration is held to: on stable voxels the observation set is identical and weight, tsdf and colour are
    within 2e-5; everywhere the values are finite, tsdf in [-1, 1] and the weight between 0 and the sum of the views' largest weights."""
    T, W, Cc, unstable = ref
    st = ~unstable
    assert unstable.mean() <= 0.05, (what, unstable.mean())
    assert np.array_equal((w > 0)[st], (W > 0)[st]), f"{what}: observation sets differ on {((w > 0) != (W > 0))[st].sum()} stable voxels"
    errs = dict(weight=np.abs(w - W)[st].max(initial=0.0), tsdf=np.abs(t - T)[st].max(initial=0.0),
                colour=0.0 if c is None else np.abs(c - Cc)[:, st].max(initial=0.0))
    print(f"{what} {sc['dims']}: unstable {unstable.mean():.4f}, max errors on stable voxels {errs}")
    for k, e in errs.items():
        assert e <= 2e-5, (what, k, e)
    wi = sc["weight_img"]
    cap = float(sc["depth"].shape[0]) if wi is None else float(sum(np.where(np.isfinite(wi[v]), wi[v], 0.0).max() for v in range(wi.shape[0])))
    assert np.isfinite(t).all() and np.isfinite(w).all() and (c is None or np.isfinite(c).all()), what
    assert t.min() >= -1.0 and t.max() <= 1.0 and w.min() >= 0.0 and w.max() <= cap * (1 + 1e-6), what


@pytest.mark.parametrize("scene", ["sphere", "plane"])
@pytest.mark.parametrize("dims", GRIDS)
def test_torch_form_and_host_run_kernel_against_the_reference(hip_lib, scene, dims):
    sc = (R.sphere_scene if scene == "sphere" else R.plane_scene)(dims)
    ref = R.reference_of(sc)
    g = _torch_grid(sc)
    t, w, c = g.tsdf.numpy(), g.weight.numpy(), None if g.colour is None else g.colour.numpy()
    check_against_reference(sc, t, w, c, ref, f"integrate_torch on the {scene}")
    if scene == "sphere":
        assert np.array_equal(w[~ref[3]], ref[1][~ref[3]]), "unit weights add up exactly"
    # the kernel's per-voxel code, compiled for the host, gives integrate_torch's bits: the torch form IS the definition
    ht, hw, hc = _host_kernel_grid(hip_lib, sc)
    for a, b, name in ((ht, t, "tsdf"), (hw, w, "weight")) + (((hc, c, "colour"),) if c is not None else ()):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{scene} {dims}: {name} differs in bits"


def test_torch_form_batch_equals_one_by_one_and_outside_grid_is_untouched():
    from das3r_amd.tsdf import TSDFGrid
    sc = R.plane_scene((28, 26, 24))
    whole = _torch_grid(sc)
    g = TSDFGrid(sc["origin"], sc["voxel"], sc["dims"], device="cpu")
    for v in range(4):
        g.integrate(_tt(sc["depth"][v]), _tt(sc["viewmatrix"][v:v + 1]), sc["tanfovx"][v:v + 1], sc["tanfovy"][v:v + 1], colour=_tt(sc["colour_img"][v]),
                    weight=_tt(sc["weight_img"][v]), trunc=sc["trunc"])
    assert torch.equal(g.tsdf, whole.tsdf) and torch.equal(g.weight, whole.weight) and torch.equal(g.colour, whole.colour)
    far = TSDFGrid((50.0, 50.0, 50.0), sc["voxel"], (9, 7, 5), device="cpu")
    far.integrate(_tt(sc["depth"]), _tt(sc["viewmatrix"]), sc["tanfovx"], sc["tanfovy"], colour=_tt(sc["colour_img"]), weight=_tt(sc["weight_img"]))
    assert bool((far.tsdf == 1).all()) and bool((far.weight == 0).all()) and bool((far.colour == 0).all())
    assert far.trunc == pytest.approx(4 * 0.04), "trunc defaults to four voxels"
    with pytest.raises(ValueError, match="colour"):
        far.integrate(_tt(sc["depth"]), _tt(sc["viewmatrix"]), sc["tanfovx"], sc["tanfovy"])
    with pytest.raises(RuntimeError, match="HIP device"):
        far.integrate(_tt(sc["depth"]), _tt(sc["viewmatrix"]), sc["tanfovx"], sc["tanfovy"], colour=_tt(sc["colour_img"]), use_kernels=True)
    with pytest.raises(ValueError, match="2\\^28"):
        TSDFGrid((0, 0, 0), 1.0, (1 << 10, 1 << 10, 1 << 9), device="cpu")


# ---------------------------------------------------------------------------------------------------------------- extraction
def host_extract(lib, t, w, c, origin, voxel):
    nz, ny, nx = t.shape
    t, w = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(w, np.float32)
    c = None if c is None else np.ascontiguousarray(c, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    dims, org = (C.c_int32 * 3)(nx, ny, nz), (C.c_float * 3)(*origin)
    ws, tot = np.zeros(lib.das3r_tsdf_extract_workspace_bytes(dims) // 4, np.int32), np.zeros(2, np.int32)
    assert lib.das3r_debug_tsdf_extract_host(dims, org, C.c_float(voxel), p(t), p(w), p(c), p(ws), p(tot), None, None, None, None) == 0
    Nv, Nf = (int(x) for x in tot)
    v, n, f = np.zeros((Nv, 3), np.float32), np.zeros((Nv, 3), np.float32), np.zeros((Nf, 3), np.int32)
    col = None if c is None else np.zeros((Nv, 3), np.float32)
    if Nv:
        assert lib.das3r_debug_tsdf_extract_host(dims, org, C.c_float(voxel), p(t), p(w), p(c), p(ws), p(tot), p(v), p(n), p(col), p(f)) == 0
    return dict(vertices=v, normals=n, colours=col, faces=f, edge_mask=(ws[:nx * ny * nz] & 0x7F).astype(np.uint8).reshape(nz, ny, nx))


def extraction_grids():
    """name -> (tsdf, weight, colour, origin, voxel) as fp32 arrays: the grids the kernels are held to the reference on.  Origins and edges keep
    every coordinate's fp32 spacing below 1e-5 voxel / 3 (three roundings: the sum inside the bracket, the product, the sum with the origin):
    coordinates stay below 64 voxels, except on the 70-voxel row, whose edge is a power of two (the product is exact)."""
    rng = np.random.default_rng(5)
    out = {}
    t, w = R.analytic_sphere_grid()
    t, w = t.astype(np.float32), w.astype(np.float32)
    out["sphere"] = (t, w, rng.random((3,) + t.shape).astype(np.float32), (0.0, 0.0, 0.0), 1.0)
    t2, w2 = t.copy(), w.copy()
    w2[:4, :4, :4] = 0.0
    t2[5, 6, 2], t2[7, 7, 9], t2[6, 2, 6] = np.nan, np.inf, -np.inf   # NaN / inf tsdf at valid weight: invalid voxels
    w2[9, 9, 9], w2[2, 9, 5] = -1.0, np.nan
    out["sphere_holes"] = (t2, w2, rng.random((3,) + t.shape).astype(np.float32), (0.3, -0.2, 0.1), 0.05)
    t3 = np.round(t * 2.0) / 2.0   # quantised: many corners exactly 0, -0.0 among them (where a negative rounds up): neither is inside
    assert (t3 == 0).sum() > 20 and np.signbit(t3[t3 == 0]).any() and not np.signbit(t3[t3 == 0]).all()
    out["zeros"] = (t3.astype(np.float32), w, None, (0.0, 0.0, 0.0), 1.0)
    out["all_positive"] = (np.abs(t) + 0.1, w, rng.random((3,) + t.shape).astype(np.float32), (0.0, 0.0, 0.0), 1.0)
    for name, dims, voxel, origin in (("plane_70_5_3", (70, 5, 3), 0.25, (-1.5, 0.25, 0.5)), ("plane_9_1_8", (9, 1, 8), 0.03, (0.1, 0.2, -0.1))):
        X, Y, Z = R.centres(dims, origin, voxel)
        n = np.array([0.21, 0.35, 0.91])
        n /= np.linalg.norm(n)
        mid = np.array([X.mean(), Y.mean(), Z.mean()])
        tp = ((X - mid[0]) * n[0] + (Y - mid[1]) * n[1] + (Z - mid[2]) * n[2]) / (4 * voxel)
        out[name] = (np.clip(tp, -1, 1).astype(np.float32), np.ones(tp.shape, np.float32), rng.random((3,) + tp.shape).astype(np.float32), origin, voxel)
    nz, ny, nx = 21, 33, 40   # a random smooth field: low-frequency waves; vertex and triangle offsets cross many count groups
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    f = sum(a * np.sin(0.35 * (p * i + q * j + r * k) + ph) for a, p, q, r, ph in rng.normal(size=(6, 5)))
    wv = (rng.random(f.shape) > 0.03).astype(np.float32) * (0.5 + rng.random(f.shape)).astype(np.float32)
    out["smooth_40_33_21"] = ((f / 3.0).astype(np.float32), wv, rng.random((3,) + f.shape).astype(np.float32), (-0.4, 0.1, 0.2), 0.02)
    return out


def check_mesh_against_reference(name, got, grid):
    """Counts, faces, owners and types exactly; positions within 1e-5 voxel, colours within 1e-5, normals within 1e-4 where the reference's
    gradient is longer than 1e-3 and exact zeros where it is zero."""
    t, w, c, origin, voxel = grid
    ref = R.extract(t, w, c, np.asarray(origin, np.float32), np.float32(voxel))
    assert got["vertices"].shape[0] == ref["vertices"].shape[0] and got["faces"].shape[0] == ref["faces"].shape[0], \
        (name, got["vertices"].shape, ref["vertices"].shape, got["faces"].shape, ref["faces"].shape)
    assert got["faces"].dtype == np.int32 and np.array_equal(got["faces"], ref["faces"]), name
    assert np.array_equal(got["edge_mask"], ref["edge_mask"]), f"{name}: vertex owners / types differ"
    if ref["vertices"].shape[0] == 0:
        return ref
    pos = np.abs(got["vertices"] - ref["vertices"]).max() / float(np.float32(voxel))
    col = 0.0 if c is None else np.abs(got["colours"] - ref["colours"]).max()
    long = ref["grad_len"] > 1e-3
    nrm = np.abs(got["normals"] - ref["normals"])[long].max(initial=0.0)
    print(f"{name}: Nv {ref['vertices'].shape[0]}, Nf {ref['faces'].shape[0]}, position {pos:.3g} voxel, colour {col:.3g}, normal {nrm:.3g}")
    assert pos <= 1e-5 and col <= 1e-5 and nrm <= 1e-4, (name, pos, col, nrm)
    zero = ref["grad_len"] == 0
    assert (got["normals"][zero] == 0).all(), name
    return ref


def test_winding_table_is_the_references(hip_lib):
    out = (C.c_uint32 * 6)()
    hip_lib.das3r_debug_tsdf_swap_table(out)
    assert list(out) == R.swap_table()


@pytest.mark.parametrize("name", ["sphere", "sphere_holes", "zeros", "all_positive", "plane_70_5_3", "plane_9_1_8", "smooth_40_33_21"])
def test_host_run_extraction_against_the_reference(hip_lib, name):
    grid = extraction_grids()[name]
    got = host_extract(hip_lib, *grid)
    ref = check_mesh_against_reference(name, got, grid)
    if name == "sphere":
        assert R.assert_closed(got["faces"]) == (780, 2334, 1556)
    if name == "all_positive":
        assert got["vertices"].shape[0] == 0 and got["faces"].shape[0] == 0
    elif name == "plane_9_1_8":
        assert got["vertices"].shape[0] > 0 and got["faces"].shape[0] == 0, "one voxel thick: no cube, so vertices (oriented samples) and no triangle"
    else:
        assert ref["faces"].shape[0] > 0


# ---------------------------------------------------------------------------------------------------------------- files and flags
def test_mesh_ply_round_trip(tmp_path):
    from das3r_amd.io_formats import read_mesh_ply, save_mesh_ply
    rng = np.random.default_rng(1)
    v, n, c = rng.normal(size=(7, 3)).astype(np.float32), rng.normal(size=(7, 3)).astype(np.float32), rng.random((7, 3)).astype(np.float32)
    c[0], c[1] = (0.0, 1.0, 2.0), (-1.0, 0.5, np.nan)
    f = np.array([[0, 1, 2], [2, 3, 4], [6, 5, 4]], np.int32)
    path = str(tmp_path / "sub" / "mesh.ply")
    save_mesh_ply(path, torch.from_numpy(v), torch.from_numpy(f), normals=n, colours=c)
    head = open(path, "rb").read(400).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 7\n") and "property list uchar int vertex_indices" in head
    assert "property uchar red" in head and "property float nx" in head
    m = read_mesh_ply(path)
    assert np.array_equal(m["vertices"], v) and np.array_equal(m["normals"], n) and np.array_equal(m["faces"], f) and m["faces"].dtype == np.int32
    assert m["colours"].dtype == np.uint8 and m["colours"][0].tolist() == [0, 255, 255] and m["colours"][1].tolist() == [0, 128, 0]
    assert np.array_equal(m["colours"][2:], np.floor(c[2:].astype(np.float64) * 255 + 0.5).astype(np.uint8))
    assert os.path.getsize(path) == len(head.split("end_header\n")[0]) + len("end_header\n") + 7 * 27 + 3 * 13
    save_mesh_ply(path, v, np.zeros((0, 3), np.int32))   # a mesh with no faces: still a file that reads back
    m = read_mesh_ply(path)
    assert np.array_equal(m["vertices"], v) and m["faces"].shape == (0, 3) and m["normals"] is None and m["colours"] is None
    save_mesh_ply(path, v[:0], f[:0], normals=n[:0], colours=c[:0])
    m = read_mesh_ply(path)
    assert m["vertices"].shape == (0, 3) and m["faces"].shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        save_mesh_ply(path, v, np.array([[0, 1, 7]]))


def test_offline_flags(monkeypatch):
    from das3r_amd import io_formats, offline
    a = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert (a.tsdf, a.tsdf_voxel, a.tsdf_relative, a.tsdf_trunc, a.tsdf_depth, a.tsdf_min_alpha, a.tsdf_static_weight) == \
        (False, None, None, 4.0, "median", 0.5, False)
    a = offline.parser().parse_args(["-m", "x", "-s", "y", "--tsdf", "--tsdf-voxel", "0.02", "--tsdf-trunc", "3", "--tsdf-depth", "blended",
                                     "--tsdf-min-alpha", "0.7", "--tsdf-static-weight"])
    assert (a.tsdf, a.tsdf_voxel, a.tsdf_trunc, a.tsdf_depth, a.tsdf_min_alpha, a.tsdf_static_weight) == (True, 0.02, 3.0, "blended", 0.7, True)
    with pytest.raises(SystemExit):
        offline.parser().parse_args(["-m", "x", "-s", "y", "--tsdf-voxel", "0.02", "--tsdf-relative", "2"])
    p = inspect.signature(offline.render_sets).parameters
    assert p["tsdf"].default is False and p["tsdf_depth"].default == "median" and p["tsdf_min_alpha"].default == 0.5
    seen = {}
    monkeypatch.setattr(io_formats, "load_sequence", lambda *a, **k: {"depths": None})
    monkeypatch.setattr(offline, "render_sets", lambda *a, **k: (seen.clear(), seen.update(k), (7, []))[2])
    offline.main(["-m", "x", "-s", "y", "--median-depth"])
    assert not [k for k in seen if k.startswith("tsdf")], "without --tsdf the program calls what it called"
    offline.main(["-m", "x", "-s", "y", "--tsdf", "--tsdf-relative", "3"])
    assert seen["tsdf"] is True and seen["tsdf_relative"] == 3.0 and seen["tsdf_voxel"] is None and seen["tsdf_trunc"] == 4.0


def test_bounds_and_grid_helpers():
    from das3r_amd.tsdf import bounds_from_points, grid_for_box
    g = torch.Generator().manual_seed(2)
    xyz = torch.rand(1000, 3, generator=g)
    xyz[0] = torch.tensor([100.0, -100.0, 50.0])   # a floater
    xyz[1] = float("nan")
    lo, hi = bounds_from_points(xyz, 0.01)
    assert all(0.0 <= l < 0.05 for l in lo) and all(0.95 < h <= 1.0 for h in hi)
    lo0, hi0 = bounds_from_points(xyz, 0.0)
    assert hi0[0] == 100.0 and lo0[1] == -100.0
    origin, dims = grid_for_box(lo, hi, 0.1, pad=2)
    assert all(o + n * 0.1 >= h + 0.2 - 1e-9 for o, n, h in zip(origin, dims, hi)) and all(10 <= n <= 16 for n in dims)
