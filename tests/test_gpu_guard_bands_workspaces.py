"""Guard bands and poison (tests/guard_bands.py) round the workspaces and outputs of the entries outside the rasterizer, through their
Python wrappers: distCUDA2 (das3r_knn3_workspace_bytes), the voxel thinning (das3r_thin_workspace_bytes), prune select + compact
(DAS3R_PRUNE_COUNT_WORDS), mesh components and filters (das3r_mesh_components_workspace_bytes), TSDF integration and extraction
(das3r_tsdf_extract_workspace_bytes), the loss kernels (das3r_photometric_blocks, das3r_depth_l1_blocks: partials and dmaps) and the pose
pre-transform.  As in tests/test_gpu_guard_bands.py every case runs once as the product allocates and once under each pattern: intact bands,
the same bits.  Sizes sit at and around each kernel's workgroup, table and tile constants, from the smallest the entry accepts."""
import numpy as np
import pytest
import torch

from tests.guard_bands import assert_same_bits, four_runs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- distCUDA2
@pytest.mark.parametrize("P", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_knn(P):
    """At and around the 256-point workgroup and the 1024-point box, from one point on; every run is also the oracle's bits — with fewer than
    four points a point has fewer than three neighbours, and both sides must then give the same bits, inf included."""
    from das3r_amd import distCUDA2
    from oracle import c_oracle
    pts = torch.rand(P, 3, generator=torch.Generator().manual_seed(100 + P))
    want = torch.from_numpy(np.ascontiguousarray(c_oracle.knn3_mean_dist2(pts.numpy())))
    if P < 3:
        assert torch.isinf(want).all(), want   # (P = 3: two finite distances and the largest finite float for the third)
    dev_pts = pts.to(DEV)

    def op(guard):
        got = distCUDA2(dev_pts).cpu()
        assert_same_bits(got, want, f"P = {P}: distCUDA2 against the oracle")
        return got

    four_runs(op, f"distCUDA2, P = {P}")


# ---------------------------------------------------------------------------------------------------------------- thin
@pytest.mark.parametrize("scored", [False, True], ids=["no_score", "score"])
@pytest.mark.parametrize("P", [1, 31, 32, 33, 1000])
def test_thin_voxel_keep(P, scored):
    """das3r_thin_voxels round the 64-slot floor of its hash table: points in the unit cube with an edge of 1/2 — eight voxels, so nearly every
    insertion collides — and scores with ties; against the torch form, exactly."""
    from das3r_amd.thin import inv_edge_of, voxel_keep_kernels, voxel_keep_torch
    g = torch.Generator().manual_seed(200 + P)
    xyz = torch.rand(P, 3, generator=g).to(DEV)
    score = (torch.randint(0, 4, (P,), generator=g).float() / 4).to(DEV) if scored else None
    inv = inv_edge_of(0.5)
    keep_t, count_t = voxel_keep_torch(xyz, score, inv)

    def op(guard):
        keep, count, info = voxel_keep_kernels(xyz, score, inv)
        torch.cuda.synchronize()
        assert torch.equal(keep.view(torch.bool), keep_t) and torch.equal(count, count_t), "the kernels against the torch form"
        assert info.tolist() == [int(keep_t.sum()), 0] and int(keep_t.sum()) <= 8
        return dict(keep=keep, count=count, info=info)

    four_runs(op, f"thin, P = {P}")


# ---------------------------------------------------------------------------------------------------------------- prune
ROW_BYTES = (4, 8, 12, 16, 36, 108, 180, 192)   # tests/test_gpu_prune.py's


def _sixteen(P):
    """The sixteen-tensor set of tests/test_gpu_prune.py test_compact_equals_boolean_indexing_bit_for_bit, drawn on the device: every row width
    once at a 16-byte aligned address and once 4 bytes off, the int64 index among the 8-byte ones."""
    g = torch.Generator(device=DEV).manual_seed(P)
    tensors = []
    for rb in ROW_BYTES:
        n = rb // 4
        a = torch.randn(P, n, generator=g, device=DEV)
        b = torch.randn(P * n + 1, generator=g, device=DEV)[1:].view(P, n)
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4 and b.is_contiguous()
        tensors += [a, b]
    tensors[2] = torch.randint(-2 ** 62, 2 ** 62, (P,), generator=g, dtype=torch.int64, device=DEV)
    assert len(tensors) == 16
    return tensors


@pytest.mark.parametrize("fraction", ["none", "all", 0.5])
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025, 2 ** 20 + 3])
def test_prune_select_and_compact(P, fraction):
    """prune.select (the count words: DAS3R_PRUNE_COUNT_WORDS) and prune.compact round the 1024-row group, nothing / everything / half kept;
    the compacted tensors are also t[keep], bit for bit."""
    from das3r_amd.prune import compact, select
    from tests.test_gpu_prune import _keep_of
    keep = _keep_of(P, fraction, 5 + P).to(DEV)
    raw, conf, drop = torch.zeros(P, 1, device=DEV), torch.ones(P, device=DEV), ~keep
    tensors = _sixteen(P)
    want = [t[keep] for t in tensors]

    def op(guard):
        dst, count = select(raw, conf, None, 0.005, None, 0.0, drop)
        kept = int(count[0])
        assert kept == int(keep.sum())
        out = compact(dst, kept, tensors)
        torch.cuda.synchronize()
        for o, w in zip(out, want):
            assert o.shape == w.shape and o.is_contiguous() and (o.numel() == 0 or torch.equal(o.view(torch.uint8), w.contiguous().view(torch.uint8)))
        return dict(dst=dst, kept=count[:1], out=[o if P <= 2048 else o.view(torch.uint8).sum(dtype=torch.int64) for o in out])

    four_runs(op, f"prune, P = {P}, kept {fraction}")


# ---------------------------------------------------------------------------------------------------------------- mesh
def _mesh_cases():
    from tests import mesh_reference as M
    return list(M.index_cases())


@pytest.mark.parametrize("name", _mesh_cases())
def test_mesh_components(name):
    """das3r_mesh_components on every index-only mesh of tests/mesh_reference.py; the workspace itself (`_ws`) is scratch, not an output."""
    from das3r_amd.mesh import components
    from tests import mesh_reference as M
    f, Nv, _ = M.index_cases()[name]
    faces = _cu(f)

    def op(guard):
        c = components(faces, Nv, use_kernels=True)
        assert c["path"] == "kernels"
        got = dict(vertex_label=c["vertex_label"].cpu().numpy(), face_label=c["face_label"].cpu().numpy(), full=c["_full"].cpu().numpy(), info=c["_info"])
        M.check_expectations(name, got)
        return {k: v for k, v in c.items() if k != "_ws"}

    four_runs(op, f"mesh components, {name}")


@pytest.mark.parametrize("holed", [False, True], ids=["plain", "holed"])
def test_mesh_filters(holed):
    """filter_components by a face count and by the K largest (every case of mesh_reference.FILTER_CASES) on the debris mesh: the selection's
    destination planes, the remapped faces, the compacted attributes."""
    from das3r_amd.mesh import filter_components
    from tests import mesh_reference as M
    m = M.debris_mesh(holed)
    mesh = {k: _cu(m[k]) for k in ("vertices", "normals", "colours", "faces")}

    def op(guard):
        out = {}
        for case in M.FILTER_CASES:
            got, rep = filter_components(mesh, *case, use_kernels=True)
            assert rep["path"] == "kernels" and rep["kept_components"] == M.FILTER_KEPT[case]
            M.check_filtered({k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}, m, *case)
            out[str(case)] = (got, {k: v for k, v in rep.items()})
        return out

    four_runs(op, f"mesh filters, holed = {holed}")


# ---------------------------------------------------------------------------------------------------------------- tsdf
@pytest.mark.parametrize("kind", ["sphere", "plane"])
def test_tsdf_integrate_and_extract_on_the_smallest_grid(kind):
    """TSDFGrid.integrate and .extract on the smallest of tests/test_tsdf_host.py GRIDS (one voxel) and on the next (63 x 1 x 1)."""
    from tests.test_gpu_tsdf import _fuse, _scene
    from tests.test_tsdf_host import GRIDS
    for dims in sorted(GRIDS, key=lambda d: d[0] * d[1] * d[2])[:2]:
        sc, _ref = _scene(kind, dims)

        def op(guard):
            g = _fuse(sc)
            mesh = g.extract()
            torch.cuda.synchronize()
            return dict(tsdf=g.tsdf, weight=g.weight, colour=g.colour, mesh=mesh)

        four_runs(op, f"tsdf {kind} {dims}")


@pytest.mark.parametrize("name", ["plane_9_1_8", "plane_70_5_3", "all_positive"])
def test_tsdf_extract(name):
    """The extraction grids with a one-voxel axis, with a 70-voxel row, and without any surface (zero-size outputs: nothing to write)."""
    from tests.test_gpu_tsdf import _extract
    from tests.test_tsdf_host import check_mesh_against_reference, extraction_grids
    grid = extraction_grids()[name]

    def op(guard):
        out = _extract(grid)
        check_mesh_against_reference(name, {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}, grid)
        if name == "all_positive":
            assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3)
        return out

    four_runs(op, f"tsdf extract {name}")


# ---------------------------------------------------------------------------------------------------------------- losses
LOSS_SHAPES = [(1, 1), (15, 17), (16, 16), (33, 31), (104, 256)]
ids = lambda hw: f"{hw[0]}x{hw[1]}"


@pytest.mark.parametrize("hw", LOSS_SHAPES, ids=ids)
def test_loss_kernels(hw):
    """The masked photometric loss forward and backward, its exposure forms (identity and a general matrix, with dL/dE), ssim_map forward and
    backward and depth_l1_loss (with and without the static map), on extents round the 16-pixel tile and the 26-pixel halo tile."""
    from das3r_amd.fused import depth_l1_loss, masked_photometric_loss, ssim_map
    from tests import loss_reference as R
    from tests.test_gpu_depth_train import _random_maps
    H, W = hw
    render, gt, static = (t.to(DEV) for t in R.make_inputs("masked", H, W))
    upstream = torch.randn(3, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)
    D, T, m, s = (t.to(DEV) for t in _random_maps(H, W, 31))

    def photometric(exposure):
        r, st = render.clone().requires_grad_(True), static.clone().requires_grad_(True)
        e = None if exposure is None else exposure.to(DEV).requires_grad_(True)
        loss, mse = masked_photometric_loss(r, gt, st, 0.2, exposure=e)
        (3.0 * loss).backward()
        return dict(loss=loss.detach(), mse=mse.detach(), d_render=r.grad, d_static=st.grad, dE=None if e is None else e.grad)

    def op(guard):
        out = dict(plain=photometric(None), identity=photometric(torch.eye(3, 4)), general=photometric(torch.tensor(R.EXPOSURE_B)))
        a, b = (render * static).requires_grad_(True), (gt * static).requires_grad_(True)
        smap = ssim_map(a, b)
        (smap * upstream).sum().backward()
        out["ssim"] = dict(map=smap.detach(), d_img1=a.grad, d_img2=b.grad)
        for name, st in (("depth_l1", None), ("depth_l1_static", s)):
            d = D.clone().requires_grad_(True)
            loss = depth_l1_loss(d, T, m, st, weight=0.37)
            (2.5 * loss).backward()
            out[name] = dict(loss=loss.detach(), d_invdepth=d.grad)
        torch.cuda.synchronize()
        return out

    four_runs(op, f"loss kernels, {H} x {W}")


# ---------------------------------------------------------------------------------------------------------------- pose pre-transform
@pytest.mark.parametrize("masked", [True, False], ids=["mask-index", "no-mask"])
@pytest.mark.parametrize("P", [1, 255, 257])
def test_pose_pretransform(P, masked):
    """fused.pretransform forward and backward (pose matrices, the per-Gaussian kernels, the 28 sums and the pose chain) on one Gaussian and
    either side of a workgroup."""
    from das3r_amd.fused import pretransform
    from tests import pose_reference as PR
    d = PR.make_general("plain", P, seed=3)
    inputs = [d[k].to(DEV).contiguous() for k in PR.INPUT_NAMES]
    conf = d["conf"].to(DEV).contiguous()
    idx = d["idx"].to(DEV) if masked else None
    if not masked:
        conf = conf[:P].contiguous()
    pose = torch.cat([d["q"].reshape(-1), d["t"].reshape(-1)]).float().to(DEV)
    ups = [d[k].to(DEV).contiguous() for k in PR.UPSTREAM_NAMES]

    def op(guard):
        leaves = [t.clone().requires_grad_(True) for t in inputs] + [conf.clone().requires_grad_(True), pose.clone().requires_grad_(True)]
        outs = pretransform(*leaves[:5], idx, leaves[5])
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        torch.cuda.synchronize()
        return dict(outputs=[o.detach() for o in outs], grads=[t.grad for t in leaves])

    four_runs(op, f"pose pre-transform, P = {P}")
