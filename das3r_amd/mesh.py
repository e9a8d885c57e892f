"""Mesh clean-up (opt-in): label the connected pieces of an extracted mesh, keep the large ones, drop the debris and its vertices.

Imperfectly masked movers and faint floaters leave small closed blobs in a fused TSDF, and marching tetrahedra turns each blob into a piece of
mesh.  include/das3r_raster.h has the rule in full:

    graph       a face is GOOD iff its three indices lie in [0, Nv); a good face joins its three vertices, a bad one joins nothing;
                connectivity is by shared vertex
    labels      vertex_label[v] = the smallest vertex index of v's component; face_label[f] = vertex_label[faces[f, 0]], -1 for a bad face
    keep rule   t = max(1, min_faces, c_K): c_1 >= c_2 >= ... the face counts of the face-bearing components, the c_K term only when
                1 <= keep_largest = K <= their number; a component stays iff it has at least t faces (ties at c_K all stay)
    filter      a vertex stays iff its component does, a face iff it is good and its component stays; both keep their order; faces are
                re-indexed; attribute rows are moved bit for bit

Two forms: csrc/mesh.hip (union-find with minimum roots, a thread per face; selection in prune_select's pattern; attributes through
das3r_prune_compact) for dense int32 faces on a HIP device, and components_torch — plain torch on any device, the DEFINITION."""
import ctypes as C

import torch

from . import _lib

ATTRIBUTES = ("vertices", "normals", "colours")


def _faces2d(faces):
    faces = torch.as_tensor(faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        if faces.numel() == 0:
            return faces.reshape(0, 3)
        raise ValueError(f"mesh: faces must be [Nf, 3], got {tuple(faces.shape)}")
    return faces


@torch.no_grad()
def components_torch(faces, n_vertices):
    """The definition in torch ops, on faces' device -> (vertex_label int64 [Nv], face_label int64 [Nf]).  The minimum label over a face's
    corners is scattered to the corners and to their current labels (scatter_reduce amin: trees are hooked, not single vertices), then
    pointers are jumped (label = label[label]), until nothing changes: a label is always a vertex of the same component and never rises, and
    at the fixed point it is constant on every face and a root of itself."""
    faces = _faces2d(faces).to(torch.int64)
    Nv = int(n_vertices)
    dev = faces.device
    label = torch.arange(Nv, dtype=torch.int64, device=dev)
    good = ((faces >= 0) & (faces < Nv)).all(dim=1) if faces.shape[0] else torch.zeros(0, dtype=torch.bool, device=dev)
    g = faces[good]
    if g.shape[0] and Nv:
        corners = g.reshape(-1)
        while True:
            low = label[g].amin(dim=1).repeat_interleave(3)
            new = label.scatter_reduce(0, corners, low, "amin", include_self=True)
            new = new.scatter_reduce(0, label[corners], low, "amin", include_self=True)   # the corners' roots too: trees merge, not vertices
            while True:
                jumped = new[new]
                if torch.equal(jumped, new):
                    break
                new = jumped
            if torch.equal(new, label):
                break
            label = new
    face_label = torch.full((faces.shape[0],), -1, dtype=torch.int64, device=dev)
    if g.shape[0]:
        face_label[good] = label[g[:, 0]]
    return label, face_label


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _qualifies(faces):
    return faces.device.type == "cuda" and faces.dtype == torch.int32 and faces.is_contiguous()


def _use_kernels(faces, use_kernels, who):
    ok = _qualifies(faces)
    if use_kernels and not ok:
        raise RuntimeError(f"{who}(use_kernels=True): dense int32 faces on a HIP device only")
    return ok if use_kernels is None else bool(use_kernels)


def _components_kernels(faces, Nv):
    """das3r_mesh_components -> (vertex_label, face_label, face_count [Nv], info list, workspace), int32 device tensors"""
    lib = _lib.load()
    dev = faces.device
    Nf = int(faces.shape[0])
    nbytes = int(lib.das3r_mesh_components_workspace_bytes(Nv, Nf))
    if nbytes == 0:
        raise ValueError(f"das3r_amd.mesh: Nv = {Nv}, Nf = {Nf} are refused (each between 0 and 2^30)")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    vertex_label = torch.empty(Nv, dtype=torch.int32, device=dev)
    face_label = torch.empty(Nf, dtype=torch.int32, device=dev)
    face_count = torch.empty(Nv, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    info_host = (C.c_int32 * 4)()
    from .rasterizer import _on_device
    with _on_device(dev):
        rc = lib.das3r_mesh_components(Nv, Nf, _ptr(faces), _ptr(vertex_label), _ptr(face_label), _ptr(face_count), _ptr(info), info_host,
                                       C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(rc, "das3r_mesh_components")
    return vertex_label, face_label, face_count, [int(x) for x in info_host], ws


@torch.no_grad()
def components(faces, n_vertices, use_kernels=None):
    """-> dict(vertex_label [Nv], face_label [Nf] (-1: a bad face), roots [C] ascending, face_count [C] (per root, in roots' order),
    bad_faces: int, path) on faces' device; the labels int32 from the kernels, int64 from the torch form.  For filter_components the dict
    also carries `_full` (face_count per VERTEX: the count at a root, 0 elsewhere) and, from the kernels, `_ws` (the workspace) and `_info`.
    use_kernels: None = the HIP kernels for dense int32 faces on a HIP device, else torch; False = torch; True = the kernels or an error
    (prune_points' convention)."""
    faces = _faces2d(faces)
    Nv = int(n_vertices)
    if Nv < 0:
        raise ValueError("das3r_amd.mesh: n_vertices must be >= 0")
    if _use_kernels(faces, use_kernels, "components"):
        vertex_label, face_label, full, info, ws = _components_kernels(faces, Nv)
        roots = torch.nonzero(vertex_label == torch.arange(Nv, dtype=torch.int32, device=faces.device)).reshape(-1)
        return dict(vertex_label=vertex_label, face_label=face_label, roots=roots, face_count=full[roots].to(torch.int64), bad_faces=info[2],
                    path="kernels", _full=full, _ws=ws, _info=info)
    vertex_label, face_label = components_torch(faces, Nv)
    roots = torch.nonzero(vertex_label == torch.arange(Nv, dtype=torch.int64, device=faces.device)).reshape(-1)
    good = face_label >= 0
    full = torch.zeros(Nv, dtype=torch.int64, device=faces.device)
    if Nv:
        full.scatter_add_(0, face_label[good], torch.ones_like(face_label[good]))
    return dict(vertex_label=vertex_label, face_label=face_label, roots=roots, face_count=full[roots], bad_faces=int((~good).sum()), path="torch",
                _full=full)


def keep_threshold(face_count, min_faces=0, keep_largest=0):
    """The keep rule -> t (int >= 1).  face_count: the per-component counts (zeros, the faceless singletons, are ignored)."""
    min_faces, K = int(min_faces), int(keep_largest)
    if min_faces < 0 or K < 0:
        raise ValueError("keep_threshold: min_faces and keep_largest must be >= 0")
    t = max(1, min_faces)
    counts = torch.as_tensor(face_count).reshape(-1)
    counts = counts[counts > 0]
    if 1 <= K <= int(counts.numel()):
        t = max(t, int(torch.topk(counts, K).values[-1]))
    return t


@torch.no_grad()
def filter_components(mesh, min_faces=0, keep_largest=0, use_kernels=None):
    """Drop the components with fewer than keep_threshold(...) faces -> (mesh dict without edge_mask, report dict).
    mesh: TSDFGrid.extract's dict (vertices [Nv, 3], faces [Nf, 3]; normals / colours [Nv, 3] or None or absent).  The report:
    face_counts (descending, face-bearing components), threshold, components / kept_components / dropped_components (face-bearing),
    singletons, bad_faces, vertices_before / _after, faces_before / _after, path.  An all-dropped mesh comes back with 0 rows."""
    faces = _faces2d(mesh["faces"])
    vertices = mesh["vertices"]
    Nv, Nf = int(vertices.shape[0]), int(faces.shape[0])
    dev = faces.device
    attrs = {k: mesh.get(k) for k in ATTRIBUTES}
    dense = all(t is None or (t.device == dev and t.is_contiguous() and t.shape[0] == Nv and (t.numel() // max(Nv, 1)) * t.element_size() % 4 == 0)
                for t in attrs.values())
    if use_kernels and not dense:
        raise RuntimeError("filter_components(use_kernels=True): dense attribute tensors with rows of a multiple of 4 bytes, on the faces' device")
    kernels = _use_kernels(faces, use_kernels, "filter_components") and dense
    comp = components(faces, Nv, use_kernels=kernels)
    counts = comp["face_count"]
    bearing = counts[counts > 0]
    t = keep_threshold(bearing, min_faces, keep_largest)
    desc = sorted((int(c) for c in bearing.tolist()), reverse=True)
    if kernels:
        lib = _lib.load()
        vertex_dst = torch.empty(Nv, dtype=torch.int32, device=dev)
        face_dst = torch.empty(Nf, dtype=torch.int32, device=dev)
        totals = torch.empty(2, dtype=torch.int32, device=dev)
        totals_host = (C.c_int32 * 2)()
        from .prune import compact
        from .rasterizer import _on_device
        with _on_device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(lib.das3r_mesh_filter_select(Nv, Nf, _ptr(comp["vertex_label"]), _ptr(comp["face_label"]), _ptr(comp["_full"]), t, _ptr(vertex_dst),
                                                    _ptr(face_dst), _ptr(totals), totals_host, C.c_void_p(comp["_ws"].data_ptr()), stream),
                       "das3r_mesh_filter_select")
            kv, kf = int(totals_host[0]), int(totals_host[1])
            out_faces = torch.empty(kf, 3, dtype=torch.int32, device=dev)
            if kf:
                _lib.check(lib.das3r_mesh_filter_faces(Nv, Nf, kv, kf, _ptr(faces), _ptr(face_dst), _ptr(vertex_dst), _ptr(out_faces), stream),
                           "das3r_mesh_filter_faces")
        present = [k for k in ATTRIBUTES if attrs[k] is not None]
        moved = dict(zip(present, compact(vertex_dst, kv, [attrs[k] for k in present])))
        out = {k: moved.get(k) for k in ATTRIBUTES}
    else:
        full = comp["_full"]
        vl, fl = comp["vertex_label"].to(torch.int64), comp["face_label"].to(torch.int64)
        keep_v = full[vl] >= t if Nv else torch.zeros(0, dtype=torch.bool, device=dev)
        keep_f = (fl >= 0) & (full[fl.clamp_min(0)] >= t) if (Nf and Nv) else torch.zeros(Nf, dtype=torch.bool, device=dev)
        new_index = torch.cumsum(keep_v.to(torch.int64), 0) - 1
        kv, kf = int(keep_v.sum()), int(keep_f.sum())
        out_faces = new_index[faces[keep_f].to(torch.int64)].to(faces.dtype).reshape(kf, 3)
        out = {k: (None if attrs[k] is None else attrs[k][keep_v.to(attrs[k].device)].contiguous()) for k in ATTRIBUTES}
    out["faces"] = out_faces
    for k in mesh:
        if k not in out and k != "edge_mask":
            out[k] = mesh[k]
    kept = sum(1 for c in desc if c >= t)
    report = dict(face_counts=desc, threshold=t, min_faces=int(min_faces), keep_largest=int(keep_largest), components=len(desc), kept_components=kept,
                  dropped_components=len(desc) - kept, singletons=int(counts.numel()) - len(desc), bad_faces=int(comp["bad_faces"]), vertices_before=Nv,
                  vertices_after=kv, faces_before=Nf, faces_after=kf, path="kernels" if kernels else "torch")
    return out, report


def write_components_json(path, report):
    """tsdf/components.json: the descending face counts, the threshold, kept and dropped counts"""
    import json
    with open(path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


def read_components_json(path):
    import json
    with open(path) as f:
        return json.load(f)
