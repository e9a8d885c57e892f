"""The float64 numpy restatement of TSDF fusion and marching-tetrahedra extraction (include/das3r_raster.h das3r_tsdf_integrate /
das3r_tsdf_extract_count / _emit), written from the rule's text and not from the kernels: what tests hold the kernels and the torch form to.

Grid conventions: dims = (nx, ny, nz), arrays [nz, ny, nx], voxel (i, j, k) centred at origin + (i + 1/2, j + 1/2, k + 1/2) * voxel, linear
index (k * ny + j) * nx + i.  Views: [V, 16] matrices in the rasterizer's layout (a row vector times the 4x4: x_c = m0 X + m4 Y + m8 Z + m12)."""
import itertools

import numpy as np

TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))   # the seven owned edges, in order
TYPE_OF = {d: t for t, d in enumerate(TYPES)}
TET_ORDERS = ("xyz", "xzy", "yxz", "yzx", "zxy", "zyx")


def fresh(dims, colour=True):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx)), np.zeros((nz, ny, nx)), (np.zeros((3, nz, ny, nx)) if colour else None)


def centres(dims, origin, voxel):
    """-> X, Y, Z [nz, ny, nx] float64"""
    nx, ny, nz = dims
    o = np.asarray(origin, np.float64)
    x = o[0] + (np.arange(nx) + 0.5) * float(voxel)
    y = o[1] + (np.arange(ny) + 0.5) * float(voxel)
    z = o[2] + (np.arange(nz) + 0.5) * float(voxel)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return X, Y, Z


def integrate(tsdf, weight, colour, dims, origin, voxel, depth, viewmatrix, tanfovx, tanfovy, colour_img=None, weight_img=None, trunc=None,
              near=0.01):
    """One batch, view after view.  -> (tsdf, weight, colour, unstable): new float64 arrays and the per-voxel mask of voxels whose discrete
    decisions an fp32 evaluation may take the other way: for some view the projected u or v lies within 1e-3 pixel of an integer while the
    point is within one pixel of the image, |sdf + trunc| < 1e-4 trunc, or |z - near| < 1e-5."""
    T, Wt = np.array(tsdf, np.float64), np.array(weight, np.float64)
    C = None if colour is None else np.array(colour, np.float64)
    depth = np.asarray(depth, np.float64)
    V, H, W = depth.shape
    vm = np.asarray(viewmatrix, np.float64).reshape(V, 16)
    X, Y, Z = centres(dims, origin, voxel)
    unstable = np.zeros(T.shape, bool)
    trunc, near = float(trunc), float(near)
    for v in range(V):
        m = vm[v]
        xc = m[0] * X + m[4] * Y + m[8] * Z + m[12]
        yc = m[1] * X + m[5] * Y + m[9] * Z + m[13]
        zc = m[2] * X + m[6] * Y + m[10] * Z + m[14]
        unstable |= np.abs(zc - near) < 1e-5
        front = zc > near
        zs = np.where(front, zc, 1.0)
        u = (xc / zs / float(tanfovx[v]) + 1.0) * W / 2.0
        w_ = (yc / zs / float(tanfovy[v]) + 1.0) * H / 2.0
        near_image = front & (u >= -1.0) & (u <= W + 1.0) & (w_ >= -1.0) & (w_ <= H + 1.0)
        unstable |= near_image & ((np.abs(u - np.round(u)) < 1e-3) | (np.abs(w_ - np.round(w_)) < 1e-3))
        inside = front & (u >= 0) & (u < W) & (w_ >= 0) & (w_ < H)
        px = np.clip(np.floor(np.where(inside, u, 0.0)).astype(np.int64), 0, W - 1)
        py = np.clip(np.floor(np.where(inside, w_, 0.0)).astype(np.int64), 0, H - 1)
        d = depth[v][py, px]
        with np.errstate(invalid="ignore"):
            ok = inside & (d > 0) & np.isfinite(d)
            wt = np.ones_like(d) if weight_img is None else np.asarray(weight_img, np.float64)[v][py, px]
            ok &= (wt > 0) & np.isfinite(wt)
            sdf = np.where(ok, d - zc, 0.0)
        unstable |= ok & (np.abs(sdf + trunc) < 1e-4 * trunc)
        ok &= ~(sdf < -trunc)
        ts = np.minimum(1.0, sdf / trunc)
        wt = np.where(ok, wt, 0.0)
        Wn = Wt + wt
        safe = np.where(ok, Wn, 1.0)
        T = np.where(ok, (T * Wt + ts * wt) / safe, T)
        if C is not None:
            ci = np.asarray(colour_img, np.float64)[v]
            for ch in range(3):
                C[ch] = np.where(ok, (C[ch] * Wt + np.where(ok, ci[ch][py, px], 0.0) * wt) / safe, C[ch])
        Wt = np.where(ok, Wn, Wt)
    return T, Wt, C, unstable


def tet_paths():
    """The six Kuhn tetrahedra as four corner offsets each, from (0, 0, 0) to (1, 1, 1), the axes added in TET_ORDERS' order."""
    out = []
    for order in TET_ORDERS:
        p, path = [0, 0, 0], [(0, 0, 0)]
        for ax in order:
            p["xyz".index(ax)] = 1
            path.append(tuple(p))
        out.append(path)
    return out


def plain_triangles(inside):
    """The triangles of one tetrahedron before any swap, as (X, Y) pairs of path positions: I / O the inside / outside corners in path order."""
    I = [q for q in range(4) if inside[q]]
    O = [q for q in range(4) if not inside[q]]
    if len(I) == 1:
        return [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
    if len(I) == 3:
        return [[(O[0], I[0]), (O[0], I[1]), (O[0], I[2])]]
    if len(I) == 2:
        return [[(I[0], O[0]), (I[0], O[1]), (I[1], O[1])], [(I[0], O[0]), (I[1], O[1]), (I[1], O[0])]]
    return []


def case_triangles(path, inside):
    """The triangles of one tetrahedron: path = its four corners, inside = four booleans.  -> list of triangles, each three (X, Y) pairs of
    path positions, wound so that the normal points from the inside corners to the outside ones (decided on integer lattice vectors: a vertex
    stands at the sum of its two corners, twice the edge's midpoint)."""
    I = [q for q in range(4) if inside[q]]
    O = [q for q in range(4) if not inside[q]]
    c = np.array(path, np.int64)
    out = []
    for tri in plain_triangles(inside):
        direction = len(I) * c[O].sum(0) - len(O) * c[I].sum(0)
        P = [c[a] + c[b] for a, b in tri]
        det = int(np.dot(np.cross(P[1] - P[0], P[2] - P[0]), direction))
        assert det != 0
        out.append([tri[0], tri[2], tri[1]] if det < 0 else tri)
    return out


def swap_table():
    """What das3r_debug_tsdf_swap_table returns, from this file's own rule: word t has bit 2 c + k set where triangle k of case c (bit q: path
    corner q inside) of tetrahedron t has its last two indices swapped."""
    words = []
    for path in tet_paths():
        w = 0
        for c in range(16):
            inside = [bool((c >> q) & 1) for q in range(4)]
            for k, (tri, plain) in enumerate(zip(case_triangles(path, inside), plain_triangles(inside))):
                if tri != plain:
                    w |= 1 << (2 * c + k)
        words.append(w)
    return words


def _shift(a, d, fill):
    """a[k + dz, j + dy, i + dx] with `fill` outside, d = (dx, dy, dz) each in {-1, 0, 1}"""
    out = np.full(a.shape, fill, a.dtype)
    nz, ny, nx = a.shape
    src = [slice(max(s, 0), n + min(s, 0)) for s, n in ((d[2], nz), (d[1], ny), (d[0], nx))]
    dst = [slice(max(-s, 0), n + min(-s, 0)) for s, n in ((d[2], nz), (d[1], ny), (d[0], nx))]
    out[tuple(dst)] = a[tuple(src)]
    return out


def gradients(tsdf, valid):
    """[3, nz, ny, nx] in tsdf units per voxel: central where both neighbours are valid, one-sided where one is, 0 where neither."""
    t = np.where(valid, tsdf, 0.0)
    g = np.zeros((3,) + t.shape)
    for ax in range(3):
        d = [0, 0, 0]
        d[ax] = 1
        tp, vp = _shift(t, d, 0.0), _shift(valid, d, False)
        d[ax] = -1
        tm, vm = _shift(t, d, 0.0), _shift(valid, d, False)
        g[ax] = np.where(vp & vm, (tp - tm) * 0.5, np.where(vp, tp - t, np.where(vm, t - tm, 0.0)))
    return g


def extract(tsdf, weight, colour, origin, voxel):
    """-> dict(vertices [Nv, 3], normals [Nv, 3], grad_len [Nv] (length of the lerped gradient, tsdf units per voxel), colours [Nv, 3] or None,
    faces [Nf, 3] int32, owner [Nv] int64 linear index, type [Nv], edge_mask [nz, ny, nx] uint8), all float64 from the inputs as they are."""
    tsdf = np.asarray(tsdf, np.float64)
    weight = np.asarray(weight, np.float64)
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        valid = (weight > 0) & np.isfinite(tsdf)
        inside = valid & (tsdf < 0)
    t = np.where(valid, tsdf, 0.0)
    g = gradients(tsdf, valid)
    has = np.zeros((nz, ny, nx, 7), bool)
    for ty, d in enumerate(TYPES):
        has[..., ty] = valid & _shift(valid, d, False) & (inside != _shift(inside, d, False))
    flat = has.reshape(-1, 7)
    vid = (np.cumsum(flat.reshape(-1)) - flat.reshape(-1)).reshape(-1, 7)   # exclusive: the index of (owner, type)
    owner, typ = np.nonzero(flat)
    Nv = owner.size
    k, j, i = np.unravel_index(owner, (nz, ny, nx))
    d = np.array(TYPES, np.int64)[typ]
    a = t[k, j, i]
    b = t[k + d[:, 2], j + d[:, 1], i + d[:, 0]]
    s = a / (a - b) if Nv else np.zeros(0)
    o = np.asarray(origin, np.float64)
    p = np.stack([i, j, k], 1).astype(np.float64)
    vertices = o[None] + (p + 0.5 + s[:, None] * d) * float(voxel)
    ga = g[:, k, j, i].T
    gb = g[:, k + d[:, 2], j + d[:, 1], i + d[:, 0]].T
    gl = ga + s[:, None] * (gb - ga)
    length = np.sqrt((gl ** 2).sum(1))
    good = (length > 0) & np.isfinite(length)
    normals = np.where(good[:, None], gl / np.where(good, length, 1.0)[:, None], 0.0)
    colours = None
    if colour is not None:
        c = np.asarray(colour, np.float64)
        ca, cb = c[:, k, j, i].T, c[:, k + d[:, 2], j + d[:, 1], i + d[:, 0]].T
        colours = ca + s[:, None] * (cb - ca)
    # triangles
    faces = np.zeros((0, 3), np.int32)
    if nx > 1 and ny > 1 and nz > 1:
        corner = lambda arr, c: arr[c[2]:nz - 1 + c[2], c[1]:ny - 1 + c[1], c[0]:nx - 1 + c[0]]
        active = np.ones((nz - 1, ny - 1, nx - 1), bool)
        for c in itertools.product((0, 1), repeat=3):
            active &= corner(valid, c)
        cube_lin = (np.arange(nz - 1)[:, None, None] * ny + np.arange(ny - 1)[None, :, None]) * nx + np.arange(nx - 1)[None, None, :]
        slots = np.full(active.shape + (6, 2, 3), -1, np.int64)
        vid3 = vid.reshape(nz, ny, nx, 7)
        for ti, path in enumerate(tet_paths()):
            ins = np.stack([corner(inside, c) for c in path], -1)
            code = (ins * (1 << np.arange(4))).sum(-1)
            for case in range(1, 15):
                sel = active & (code == case)
                if not sel.any():
                    continue
                kk, jj, ii = np.nonzero(sel)
                for tk, tri in enumerate(case_triangles(path, [bool((case >> q) & 1) for q in range(4)])):
                    for vk, (qa, qb) in enumerate(tri):
                        lo, hi = path[min(qa, qb)], path[max(qa, qb)]
                        ty = TYPE_OF[tuple(h - l for h, l in zip(hi, lo))]
                        slots[kk, jj, ii, ti, tk, vk] = vid3[kk + lo[2], jj + lo[1], ii + lo[0], ty]
        rows = slots.reshape(-1, 3)   # (cube, tetrahedron, triangle) order: cubes in (k, j, i) order = by linear index
        assert (np.diff(cube_lin.reshape(-1)) > 0).all()
        faces = rows[rows[:, 0] >= 0].astype(np.int32)
    mask = (has * (1 << np.arange(7))).sum(-1).astype(np.uint8)
    return dict(vertices=vertices, normals=normals, grad_len=length, colours=colours, faces=faces, owner=owner, type=typ, edge_mask=mask)


# ------------------------------------------------------------------------------------------------------------------ mesh checks
def edge_stats(faces):
    """-> (directed-edge multiplicities, undirected-edge multiplicities) as arrays of counts"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    n = int(f.max()) + 1 if f.size else 1
    _, cd = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    lo, hi = e.min(1), e.max(1)
    _, cu = np.unique(lo * n + hi, return_counts=True)
    return cd, cu


def assert_closed(faces, n_vertices_used=None):
    """every undirected edge in exactly two triangles, every directed edge in exactly one, V - E + F = 2  -> (V, E, F)"""
    cd, cu = edge_stats(faces)
    assert (cu == 2).all(), f"undirected edge multiplicities {np.unique(cu)}"
    assert (cd == 1).all(), f"directed edge multiplicities {np.unique(cd)}"
    V = np.unique(np.asarray(faces)).size if n_vertices_used is None else n_vertices_used
    E, F = cu.size, len(faces)
    assert V - E + F == 2, (V, E, F)
    return V, E, F


def triangle_normals(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0


def enclosed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ------------------------------------------------------------------------------------------------------------------ scenes
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """A view matrix in the rasterizer's layout (16 floats; +z looks at the target, x right, y down) as float32."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    up = np.asarray(up, np.float64)
    if abs(np.dot(f, up)) > 0.99:
        up = np.array([0.0, 1.0, 0.0])
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    dn = np.cross(f, r)
    R = np.stack([r, dn, f], 0)   # world -> camera rows
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = -R @ eye
    return np.ascontiguousarray(M.T.reshape(16).astype(np.float32))   # row-vector convention: the transpose, flattened


def pixel_rays(H, W, tanx, tany):
    x = ((2 * np.arange(W) + 1) / W - 1.0) * tanx
    y = ((2 * np.arange(H) + 1) / H - 1.0) * tany
    return np.meshgrid(x, y, indexing="xy")   # rx, ry [H, W]


def sphere_depth(viewmatrix, H, W, tanx, tany, centre, radius):
    """View-space z of the first hit of every pixel's central ray on the sphere (0 where it misses), float32."""
    M = np.asarray(viewmatrix, np.float64).reshape(4, 4).T
    c = M[:3, :3] @ np.asarray(centre, np.float64) + M[:3, 3]
    rx, ry = pixel_rays(H, W, tanx, tany)
    dirs = np.stack([rx, ry, np.ones_like(rx)], -1)   # the point at depth z is z * dirs
    A = (dirs ** 2).sum(-1)
    B = dirs @ c
    disc = B * B - A * (c @ c - radius * radius)
    z = (B - np.sqrt(np.maximum(disc, 0.0))) / A
    return np.where((disc > 0) & (z > 0), z, 0.0).astype(np.float32)


def plane_depth(viewmatrix, H, W, tanx, tany, normal, offset):
    """View-space z of every pixel's ray on the plane {x: normal . x = offset} (0 where it is behind or parallel), float32."""
    M = np.asarray(viewmatrix, np.float64).reshape(4, 4).T
    n = M[:3, :3] @ np.asarray(normal, np.float64)
    off = float(offset) + n @ M[:3, 3]   # n_c . x_c = offset + n_c . t
    rx, ry = pixel_rays(H, W, tanx, tany)
    den = n[0] * rx + n[1] * ry + n[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = off / den
    return np.where(np.isfinite(z) & (z > 0), z, 0.0).astype(np.float32)


SPHERE = dict(radius=0.35, centre=(0.02, -0.01, 0.03), H=48, W=56, tanx=0.45, tany=0.4, dims=(28, 26, 24), voxel=0.04, trunc=0.16)


JITTER = (0.007, 0.003, -0.007)


def grid_origin(dims, voxel):
    """The grid centred on the world origin, moved by JITTER: with the centre exactly there the axis-aligned cameras of the sphere scene see
    rows of voxel centres on exact pixel boundaries (tan 0.4, 48 rows, voxel 0.04), and 43 % of the grid counts as unstable."""
    return np.array([-0.5 * n * voxel + j for n, j in zip(dims, JITTER)], np.float32)


def sphere_scene(dims=None):
    """Scene (c): six views from +-1.5 along the axes of a sphere; the grid is centred (nearly: grid_origin) on the world origin.  -> dict"""
    s = dict(SPHERE)
    if dims is not None:
        s["dims"] = tuple(dims)
    eyes = [(1.5, 0, 0), (-1.5, 0, 0), (0, 1.5, 0), (0, -1.5, 0), (0, 0, 1.5), (0, 0, -1.5)]
    vm = np.stack([look_at(e, (0.0, 0.0, 0.0)) for e in eyes], 0)
    s["viewmatrix"] = vm
    s["tanfovx"] = np.full(6, s["tanx"], np.float32)
    s["tanfovy"] = np.full(6, s["tany"], np.float32)
    s["depth"] = np.stack([sphere_depth(m, s["H"], s["W"], s["tanx"], s["tany"], s["centre"], s["radius"]) for m in vm], 0)
    s["origin"] = grid_origin(s["dims"], s["voxel"])
    s["colour_img"] = s["weight_img"] = None
    s["near"] = 0.01
    return s


def plane_scene(dims=(28, 26, 24)):
    """A tilted plane seen by four views, with a colour image, a weight image holding 0, negative, NaN and inf, depth holding 0, negative, NaN
    and inf, one camera inside the grid (voxels behind it exist) and one view that sees only part of the grid.  The grid is centred like the
    sphere scene's (grid_origin); the plane passes 0.05 below the world origin, so every grid meets it."""
    H, W, tanx, tany, voxel = 40, 52, 0.5, 0.42, 0.04
    normal = np.array([0.3, -0.2, 0.93])
    normal /= np.linalg.norm(normal)
    eyes = [(0.1, -0.2, 1.4), (1.2, 0.3, 0.9), (-0.13, 0.11, 0.27), (-1.6, -1.3, 0.8)]
    targets = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.05, -0.02, -0.4), (-0.25, -0.2, -0.05)]
    tans = [(tanx, tany), (tanx, tany), (0.6, 0.5), (0.12, 0.1)]   # the last view is narrow: part of the grid only
    vm = np.stack([look_at(e, t) for e, t in zip(eyes, targets)], 0)
    depth = np.stack([plane_depth(m, H, W, tx, ty, normal, -0.05) for m, (tx, ty) in zip(vm, tans)], 0)
    rng = np.random.default_rng(7)
    colour = rng.random((4, 3, H, W)).astype(np.float32)
    weight = (0.25 + rng.random((4, H, W))).astype(np.float32)
    for v in range(4):   # poisoned pixels, spread over the images
        idx = rng.permutation(H * W)[:64]
        wv, dv = weight[v].reshape(-1), depth[v].reshape(-1)
        wv[idx[0:8]], wv[idx[8:16]], wv[idx[16:24]], wv[idx[24:32]] = 0.0, -1.0, np.nan, np.inf
        dv[idx[32:40]], dv[idx[40:48]], dv[idx[48:56]], dv[idx[56:64]] = 0.0, -0.7, np.nan, np.inf
    return dict(H=H, W=W, dims=tuple(dims), voxel=voxel, trunc=0.16, near=0.01, viewmatrix=vm, tanfovx=np.array([t[0] for t in tans], np.float32),
                tanfovy=np.array([t[1] for t in tans], np.float32), depth=depth, colour_img=colour, weight_img=weight,
                origin=grid_origin(dims, voxel))


def reference_of(scene, colour=None):
    """The float64 integration of a scene into a fresh grid -> (tsdf, weight, colour, unstable)"""
    has_colour = scene["colour_img"] is not None if colour is None else colour
    t, w, c = fresh(scene["dims"], has_colour)
    return integrate(t, w, c, scene["dims"], scene["origin"], np.float32(scene["voxel"]), scene["depth"], scene["viewmatrix"], scene["tanfovx"],
                     scene["tanfovy"], scene["colour_img"], scene["weight_img"], np.float32(scene["trunc"]), np.float32(scene["near"]))


def analytic_sphere_grid(n=12, centre=(6.1, 5.9, 6.2), r=3.7):
    """tsdf = distance - r at voxel centres i + 1/2 of an n^3 grid, everything valid"""
    c = np.arange(n) + 0.5
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    t = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r
    return t, np.ones_like(t)
