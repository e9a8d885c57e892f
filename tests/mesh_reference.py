"""Reference for the mesh clean-up (das3r_amd/mesh.py, csrc/mesh.hip): canonical component labels from scipy's connected_components mapped to
the minimum index of every component, a numpy filter that follows include/das3r_raster.h's definitions, and the meshes the tests use.  Everything
is integer-valued: every comparison is exact equality, moved attributes bit for bit."""
import functools

import numpy as np

INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------------------------ the definition
def good_faces(faces, Nv):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < Nv)).all(axis=1)


def components(faces, Nv):
    """-> dict(vertex_label [Nv], face_label [Nf], full [Nv]: face_count at the root and 0 elsewhere, roots ascending, face_count per root,
    bad_faces, n_components, n_face_components), int64"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    good = good_faces(f, Nv)
    g = f[good]
    rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    if Nv:
        n, lab = connected_components(coo_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(Nv, Nv)), directed=False)
        lowest = np.full(n, Nv, np.int64)
        np.minimum.at(lowest, lab, np.arange(Nv))
        vertex_label = lowest[lab]
    else:
        vertex_label = np.zeros(0, np.int64)
    face_label = np.full(f.shape[0], -1, np.int64)
    face_label[good] = vertex_label[g[:, 0]]
    full = np.bincount(face_label[good], minlength=Nv).astype(np.int64) if Nv else np.zeros(0, np.int64)
    roots = np.nonzero(vertex_label == np.arange(Nv))[0]
    return dict(vertex_label=vertex_label, face_label=face_label, full=full, roots=roots, face_count=full[roots], bad_faces=int((~good).sum()),
                n_components=int(roots.size), n_face_components=int((full > 0).sum()))


def threshold(face_count, min_faces, keep_largest):
    c = np.sort(np.asarray(face_count, np.int64)[np.asarray(face_count) > 0])[::-1]
    t = max(1, int(min_faces))
    if 1 <= keep_largest <= c.size:
        t = max(t, int(c[keep_largest - 1]))
    return t


def filter_mesh(mesh, min_faces=0, keep_largest=0):
    """mesh: dict of numpy arrays (vertices, normals, colours or None, faces) -> (filtered dict, threshold, kept component count)"""
    f = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    Nv = mesh["vertices"].shape[0]
    c = components(f, Nv)
    t = threshold(c["face_count"], min_faces, keep_largest)
    keep_v = c["full"][c["vertex_label"]] >= t if Nv else np.zeros(0, bool)
    keep_f = np.zeros(f.shape[0], bool)
    ok = c["face_label"] >= 0
    keep_f[ok] = c["full"][c["face_label"][ok]] >= t
    new = np.cumsum(keep_v) - 1
    out = {k: (None if mesh.get(k) is None else mesh[k][keep_v]) for k in ("vertices", "normals", "colours")}
    out["faces"] = new[f[keep_f]].astype(np.int32).reshape(-1, 3)
    return out, t, int((c["face_count"] >= t).sum())


def same_partition(a, b):
    """two labelings describe the same partition"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return np.unique(pairs[:, 0]).size == pairs.shape[0] == np.unique(pairs[:, 1]).size


# ------------------------------------------------------------------------------------------------------------------ mesh builders
def _finish(faces, Nv, ids="natural", shuffle=False, seed=0):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    if ids == "reversed":
        f = Nv - 1 - f
    elif ids == "perm":
        f = rng.permutation(Nv)[f]
    if shuffle:
        f = f[rng.permutation(f.shape[0])]
    return np.ascontiguousarray(f, np.int32), int(Nv)


def strip(n, ids="natural", shuffle=False, seed=0):
    i = np.arange(n)
    return _finish(np.stack([i, i + 1, i + 2], 1), n + 2, ids, shuffle, seed)


def fan(n, hub_last=False):
    i = np.arange(n)
    Nv = n + 2
    f = np.stack([np.full(n, Nv - 1), i, i + 1], 1) if hub_last else np.stack([np.zeros(n, np.int64), i + 1, i + 2], 1)
    return _finish(f, Nv)


def singletons(n=20000, isolated=7):
    Nv = 3 * n + isolated
    lone = (np.arange(isolated) * (Nv // isolated) + 3).astype(np.int64)
    rest = np.setdiff1d(np.arange(Nv), lone)
    return _finish(rest.reshape(n, 3), Nv), lone


def combs(n):
    i = np.arange(n)
    even = np.stack([2 * i, 2 * i + 2, 2 * i + 4], 1)
    return _finish(np.concatenate([even, even + 1], 0), 2 * n + 4, shuffle=True, seed=3)


def with_bad_faces(faces, Nv, seed=4):
    """faces with -1, Nv and 2^31 - 1 among their indices spliced in at fixed random places -> (faces, positions of the bad ones)"""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces, np.int64)
    bad = np.array([[-1, 0, 1], [0, Nv, 1], [2, 1, INT_MAX], [-1, -1, -1], [Nv, Nv + 1, Nv + 2], [INT_MAX, 3, 4], [0, 1, -2 ** 31], [5, -7, Nv - 1]], np.int64)
    at = np.sort(rng.choice(f.shape[0] + 1, bad.shape[0], replace=False))
    out = np.insert(f, at, bad, axis=0)
    where = at + np.arange(bad.shape[0])
    return np.ascontiguousarray(out, np.int32), where


def degenerate():
    """duplicate faces, (a, a, b), (a, a, a): 12 vertices -> components {0, 1, 2}, {3, 4}, {5}, {6}, {7, 8, 9, 10}, {11}"""
    f = [[0, 1, 2], [0, 1, 2], [2, 1, 0], [3, 3, 4], [5, 5, 5], [7, 8, 8], [9, 9, 10], [8, 10, 8], [4, 3, 3]]
    return np.asarray(f, np.int32), 12


STRIP_SIZES = (1, 63, 64, 65, 255, 256, 257, 70001)


@functools.lru_cache(maxsize=None)
def index_cases():
    """name -> (faces int32 [Nf, 3], Nv, expect): expect holds what the issue states for the case beyond the scipy reference (may be empty)"""
    out = {}
    out["empty"] = (np.zeros((0, 3), np.int32), 0, dict(n_components=0))
    out["five_singletons"] = (np.zeros((0, 3), np.int32), 5, dict(n_components=5, n_face_components=0))
    out["one_triangle"] = (np.array([[0, 1, 2]], np.int32), 3, dict(n_components=1))
    out["two_share_edge"] = (np.array([[0, 1, 2], [2, 1, 3]], np.int32), 4, dict(n_components=1))
    out["two_share_vertex"] = (np.array([[0, 1, 2], [2, 3, 4]], np.int32), 5, dict(n_components=1))
    out["two_disjoint"] = (np.array([[0, 1, 2], [3, 4, 5]], np.int32), 6, dict(n_components=2, counts=[1, 1]))
    for n in STRIP_SIZES:
        for ids in ("natural", "reversed", "perm"):
            f, Nv = strip(n, ids, shuffle=True, seed=n)
            out[f"strip_{n}_{ids}"] = (f, Nv, dict(n_components=1, counts=[n], all_label=0))
    for hub_last in (False, True):
        f, Nv = fan(50000, hub_last)
        out[f"fan_hub_{'last' if hub_last else 'first'}"] = (f, Nv, dict(n_components=1, counts=[50000], all_label=0))
    (f, Nv), _ = singletons()
    out["singletons"] = (f, Nv, dict(n_components=20007, n_face_components=20000, max_count=1))
    f, Nv = combs(301)
    out["combs"] = (f, Nv, dict(n_components=2, counts=[301, 301], labels={0, 1}))
    fb, where = with_bad_faces(f, Nv)
    out["bad_faces"] = (fb, Nv, dict(n_components=2, counts=[301, 301], bad_faces=8, bad_at=where, same_vertex_labels_as="combs"))
    f, Nv = degenerate()
    out["degenerate"] = (f, Nv, dict(n_components=6, counts=[3, 2, 1, 3], n_face_components=4))
    return out


@functools.lru_cache(maxsize=None)
def reference_of(name):
    f, Nv, _ = index_cases()[name]
    return components(f, Nv)


def check_expectations(name, got):
    """got: dict(vertex_label, face_label, full [Nv], info [4]) as numpy int arrays — against the scipy reference, exactly, and against what the
    case is built to give"""
    f, Nv, expect = index_cases()[name]
    ref = reference_of(name)
    assert np.array_equal(np.asarray(got["vertex_label"], np.int64), ref["vertex_label"]), f"{name}: vertex labels"
    assert np.array_equal(np.asarray(got["face_label"], np.int64), ref["face_label"]), f"{name}: face labels"
    assert np.array_equal(np.asarray(got["full"], np.int64), ref["full"]), f"{name}: face counts"
    info = [int(x) for x in got["info"]]
    assert info == [ref["n_components"], ref["n_face_components"], ref["bad_faces"], 0], (name, info)
    if "n_components" in expect:
        assert ref["n_components"] == expect["n_components"], name
    if "n_face_components" in expect:
        assert ref["n_face_components"] == expect["n_face_components"], name
    if "counts" in expect:
        assert ref["face_count"][ref["face_count"] > 0].tolist() == expect["counts"], name
    if "all_label" in expect:
        assert (ref["vertex_label"] == expect["all_label"]).all() and (ref["face_label"] == expect["all_label"]).all(), name
    if "labels" in expect:
        assert set(ref["vertex_label"].tolist()) == expect["labels"], name
    if "max_count" in expect:
        assert ref["full"].max() == expect["max_count"], name
    if "bad_faces" in expect:
        assert ref["bad_faces"] == expect["bad_faces"] and (ref["face_label"][expect["bad_at"]] == -1).all(), name
        assert (np.delete(ref["face_label"], expect["bad_at"]) >= 0).all(), name
    if "same_vertex_labels_as" in expect:
        assert np.array_equal(ref["vertex_label"], reference_of(expect["same_vertex_labels_as"])["vertex_label"]), name


# ------------------------------------------------------------------------------------------------------------------ grid fields
DEBRIS_DIMS = (32, 24, 20)   # (nx, ny, nz)
DEBRIS_BALLS = ((10.1, 11.9, 10.2, 7.3), (25.2, 8.1, 6.3, 3.1), (24.9, 18.2, 14.1, 0.9), (27.3, 3.2, 16.4, 0.8), (20.6, 20.7, 3.3, 0.7),
                (28.4, 21.1, 8.2, 1.2), (3.3, 2.9, 17.2, 0.6))
# float64: the figures the feature was specified with.  float32 (the field the kernels are fed): the reference extraction's own — the voxel
# centre (24.5, 17.5, 14.5) lies at sqrt(0.81) from the centre of the ball of radius 0.9, a tie that the two precisions break differently,
# so that ball's piece has 68 faces instead of 88 and the mesh 10 vertices and 20 faces fewer.
DEBRIS_FIGURES = dict(float64=dict(plain=dict(Nv=3684, Nf=7340, components=7, counts=[5960, 1068, 128, 88, 48, 24, 24]),
                                   holed=dict(Nv=3605, Nf=7138, components=9, counts=[5758, 1068, 128, 88, 48, 24, 24])),
                      float32=dict(plain=dict(Nv=3674, Nf=7320, components=7, counts=[5960, 1068, 128, 68, 48, 24, 24]),
                                   holed=dict(Nv=3595, Nf=7118, components=9, counts=[5758, 1068, 128, 68, 48, 24, 24])))


def ball_field(dims, balls, dtype=np.float64):
    """tsdf = clip(min_b(|p - c_b| - r_b) / 4, -1, 1) at the voxel centres i + 1/2, [nz, ny, nx], every operation in `dtype`"""
    nx, ny, nz = dims
    ax = lambda n: np.arange(n, dtype=dtype) + dtype(0.5)
    Z, Y, X = np.meshgrid(ax(nz), ax(ny), ax(nx), indexing="ij")
    d = None
    for cx, cy, cz, r in balls:
        e = np.sqrt((X - dtype(cx)) ** 2 + (Y - dtype(cy)) ** 2 + (Z - dtype(cz)) ** 2) - dtype(r)
        d = e if d is None else np.minimum(d, e)
    return np.clip(d / dtype(4.0), dtype(-1.0), dtype(1.0)).astype(dtype)


def debris_field(holed=False, dtype=np.float64):
    t = ball_field(DEBRIS_DIMS, DEBRIS_BALLS, dtype)
    w = np.ones(t.shape, dtype)
    if holed:
        w[8:12, 10:14, 15:19] = 0
    return t, w


@functools.lru_cache(maxsize=None)
def debris_mesh(holed=False, dtype_name="float32"):
    """The reference extraction (tests/tsdf_reference.extract) of the debris field, with random float32 attributes that carry NaN and
    negative-zero bit patterns -> dict(vertices, normals, colours float32, faces int32, tsdf, weight)"""
    from tests import tsdf_reference as R
    dtype = np.float32 if dtype_name == "float32" else np.float64
    t, w = debris_field(holed, dtype)
    m = R.extract(t, w, None, np.zeros(3, np.float32), np.float32(1.0))
    Nv = m["vertices"].shape[0]
    rng = np.random.default_rng(7)
    normals = rng.normal(size=(Nv, 3)).astype(np.float32)
    colours = rng.random((Nv, 3)).astype(np.float32)
    normals[::97, 1] = np.nan
    colours[::89, 2] = -0.0
    return dict(vertices=m["vertices"].astype(np.float32), normals=normals, colours=colours, faces=np.ascontiguousarray(m["faces"], np.int32), tsdf=t, weight=w)


FILTER_CASES = ((0, 0), (25, 0), (0, 5), (0, 6), (0, 1), (0, 100), (6000, 0))
# kept components of the debris mesh (plain and holed alike: counts c_2 .. c_7 are the same and c_1 < 6000)
FILTER_KEPT = {(0, 0): 7, (25, 0): 5, (0, 5): 5, (0, 6): 7, (0, 1): 1, (0, 100): 7, (6000, 0): 0}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_filtered(got, mesh, min_faces, keep_largest):
    """got: dict of numpy arrays from filter_components — against the numpy filter, exact arrays, attributes bit for bit -> the reference"""
    ref, t, kept = filter_mesh(mesh, min_faces, keep_largest)
    assert got["faces"].dtype == np.int32 and got["faces"].shape == ref["faces"].shape and np.array_equal(got["faces"], ref["faces"]), (min_faces, keep_largest)
    for k in ("vertices", "normals", "colours"):
        assert same_bits(got[k], ref[k]), (k, min_faces, keep_largest)
    return ref, t, kept
