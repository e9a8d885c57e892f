"""Float64 reference of the normal-consistency regulariser (include/das3r_raster.h das3r_gaussian_normals_forward /
das3r_normal_consistency_forward).  TEST INFRASTRUCTURE ONLY: torch ops in float64, gradients from autograd.

The definitions are implemented literally:
  * gaussian_normals: k = argmin scale (ties: the lowest index), a = column k of R(q / |q|), d = mean - campos, flip = (a . d > 0),
    n_world = flip ? -a : a, into view space by the rotation part of the view matrix (row-vector convention).  k and flip are selections: they
    carry no graph, as the library's backward holds them fixed.
  * depth_normals: the PLAIN difference of unprojected points, dx = p(x+1, y) - p(x-1, y), dy = p(x, y+1) - p(x, y-1), p = z ray — not the
    rearranged form the kernels evaluate, so that the comparison checks the rearrangement too — N_d = (dy x dx) / |dy x dx|.
  * normal_consistency: loss = m (alpha - normal . N_d); an invalid pixel is selected to exact zeros (torch.where on sanitised operands, so
    that NaN or inf in the depth image reaches neither a value nor a gradient).
  * end to end: the blending weights come from tests.distortion_reference.rebuild_weights over the dense oracle; N_r = sum w n, A = sum w,
    D = sum w m; the median z is the reference's depths gathered at the LIBRARY's hit plane (tests/test_gpu_median.py pins that plane)."""
import torch


def quat_to_R(q):
    """oracle/raster_oracle.c quat_to_R on [P, 4] (r, x, y, z) -> [P, 3, 3]"""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def gaussian_normals(rotations, scales, means3D, viewmatrix, campos):
    """-> dict(normals [P, 3] float64 with the graph of `rotations`, k [P] int64, flip [P] bool, choice [P] int64 = k | flip << 2,
    cosine [P] = a . d / |d|: how far the flip decision is from its threshold)."""
    q = rotations.double()
    s = scales.detach().double()
    zero = torch.zeros(s.shape[0], dtype=torch.int64, device=s.device)
    k = torch.where(s[:, 0] <= torch.minimum(s[:, 1], s[:, 2]), zero, torch.where(s[:, 1] <= s[:, 2], zero + 1, zero + 2))   # ties: the lowest index
    R = quat_to_R(q / q.norm(dim=1, keepdim=True))
    a = torch.gather(R, 2, k[:, None, None].expand(-1, 3, 1))[:, :, 0]
    d = means3D.detach().double() - campos.double().reshape(1, 3)
    dot = (a.detach() * d).sum(1)
    flip = dot > 0
    n_world = torch.where(flip[:, None], -a, a)
    V = viewmatrix.double().reshape(4, 4)[:3, :3]
    return dict(normals=n_world @ V, k=k, flip=flip, choice=k + 4 * flip.long(), cosine=dot / d.norm(dim=1).clamp_min(1e-300))


def _rays(H, W, tanfovx, tanfovy, device):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device), torch.arange(W, dtype=torch.float64, device=device), indexing="ij")
    return torch.stack([((2 * xs + 1) / W - 1) * tanfovx, ((2 * ys + 1) / H - 1) * tanfovy, torch.ones_like(xs)], 0)   # [3, H, W]


def depth_normals(depth, tanfovx, tanfovy):
    """depth [H, W] -> (N_d [3, H, W] float64 with the graph of `depth`, valid [H, W] bool).  Invalid pixels: exact zeros, no graph."""
    z = depth.double()
    H, W = z.shape
    ok = torch.isfinite(z.detach()) & (z.detach() > 0)
    valid = torch.zeros(H, W, dtype=torch.bool, device=z.device)
    N = torch.zeros(3, H, W, dtype=torch.float64, device=z.device)
    if H < 3 or W < 3:
        return N, valid
    zs = torch.where(ok, z, torch.ones_like(z))                  # sanitised: what an invalid pixel holds never enters the arithmetic
    p = zs[None] * _rays(H, W, float(tanfovx), float(tanfovy), z.device)
    dx = p[:, 1:-1, 2:] - p[:, 1:-1, :-2]
    dy = p[:, 2:, 1:-1] - p[:, :-2, 1:-1]
    c = torch.cross(dy, dx, dim=0)
    n2 = (c * c).sum(0)
    inner = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1] & torch.isfinite(n2.detach()) & (n2.detach() > 0)
    unit = c / torch.sqrt(torch.where(inner, n2, torch.ones_like(n2)))[None]
    valid[1:-1, 1:-1] = inner
    N = torch.nn.functional.pad(torch.where(inner[None], unit, torch.zeros_like(unit)), (1, 1, 1, 1))
    return N, valid


def normal_consistency(depth, normal, alpha, tanfovx, tanfovy, mask=None):
    """-> (loss [H, W] float64 with the graph of depth / normal / alpha, N_d [3, H, W], valid [H, W])"""
    N, valid = depth_normals(depth, tanfovx, tanfovy)
    m = torch.ones_like(N[0]) if mask is None else mask.detach().double().reshape(N[0].shape)
    raw = m * (alpha.double().reshape(N[0].shape) - (normal.double() * N).sum(0))
    return torch.where(valid, raw, torch.zeros_like(raw)), N, valid


def plane_depth(H, W, tanfovx, tanfovy, n, c):
    """The depth image of the plane n . p = c: z = c / (n . ray), float64 [H, W]."""
    rays = _rays(H, W, float(tanfovx), float(tanfovy), torch.device("cpu"))
    nn = torch.as_tensor(n, dtype=torch.float64)
    return float(c) / (nn[:, None, None] * rays).sum(0)


def end_to_end(leaves, settings, H, W, hit_gaussian, normal_depth="median", mask=None, opacity_factor=None):
    """The whole term over the dense oracle -> dict(normals [3, H, W], alpha [H, W], z [H, W], loss [H, W]) in float64 with the graph of
    `leaves` (means3D, means2D, opacities, scales, rotations: float64 tensors on one device).  settings: the oracle's keywords (tanfovx,
    tanfovy, viewmatrix, campos, ...).  hit_gaussian [H, W] int: the LIBRARY's hit plane (normal_depth="median"; -1: empty pixel)."""
    from oracle.dense_oracle import rasterize_dense
    from tests.distortion_reference import rebuild_weights
    op = leaves["opacities"].double()
    if opacity_factor is not None:
        op = op * opacity_factor.double().reshape(op.shape)
    dev = op.device
    P = op.shape[0]
    rest = {k: v for k, v in leaves.items() if k != "opacities"}
    _, _, aux = rasterize_dense(opacities=op, colors_precomp=torch.zeros(P, 3, dtype=torch.float64, device=dev), image_height=H, image_width=W,
                                **rest, **settings)
    w, m, _ = rebuild_weights(aux, op, H, W)                       # [Npix, P] in the oracle's order, m = 1 / depth[order]
    n = gaussian_normals(leaves["rotations"], leaves["scales"], leaves["means3D"], settings["viewmatrix"], settings["campos"])["normals"]
    Nr = (w @ n[aux["order"]]).t().reshape(3, H, W)
    A = w.sum(1).reshape(H, W)
    if normal_depth == "median":
        hit = hit_gaussian.to(dev).long().reshape(-1)
        z = torch.where(hit >= 0, aux["depth"].double()[hit.clamp(min=0)], torch.zeros(H * W, dtype=torch.float64, device=dev)).reshape(H, W)
    else:
        D = (w * m[None]).sum(1).reshape(H, W)
        pos = D.detach() > 0
        z = torch.where(pos, A / torch.where(pos, D, torch.ones_like(D)), torch.zeros_like(D))
    loss, Nd, valid = normal_consistency(z, Nr, A, settings["tanfovx"], settings["tanfovy"], mask)
    return dict(normals=Nr, alpha=A, z=z, loss=loss, depth_normals=Nd, valid=valid)
