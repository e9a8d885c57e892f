"""Float64 reference of the ray-distortion regulariser (include/das3r_raster.h das3r_raster_distortion_forward).  TEST INFRASTRUCTURE ONLY.

It calls oracle.dense_oracle.rasterize_dense and rebuilds the blending weights with autograd from what the oracle hands back in `aux`:
  * aux["order"], aux["keep"], aux["px"], aux["py"], aux["conic"] and the opacities give alpha, with the oracle's straight-through 0.99 clamp;
  * w = alpha * cumprod(1 - alpha) over the kept entries before it;
  * m = 1 / aux["depth"][order].
The rebuilt 1 - prod(1 - alpha) over `keep` must reproduce 1 - aux["T_final"] to 1e-12: asserted here, on every call.

The value returned is the ORDER-FREE pairwise form
    D[pixel] = 1/2 sum_i sum_j w_i w_j |m_i - m_j|,
evaluated pair by pair over each pixel's kept entries (compacted to the front, the pixels taken in chunks).

The derivative at a tie.  |m_i - m_j| has a kink where two depths are equal (duplicated splats: the `depth_ties` scene).  The library's
definition is sum_{j<k} w_j w_k (m_j - m_k) in list order with the order — a discrete decision of the forward — held fixed, which is smooth
there.  So |d| is written as s d with s = sign(d) where d != 0 — taken from the depths themselves, never from the list — and, where d == 0
exactly, s = +1 for the entry earlier in the list: the value is |d| everywhere, and the one-sided derivative picked at a tie is the
fixed-order one.  (torch.abs would pick 0 there: the derivative of no fixed order.)"""
import torch


def rebuild_weights(aux, opacities, H, W, dtype=torch.float64):
    """-> (w [Npix, P], m [P], keep [Npix, P]) in the oracle's global (depth, index) order; w and m carry the autograd graph of the oracle's
    px / py / conic / depth and of `opacities`."""
    o, keep = aux["order"], aux["keep"]
    dev = o.device
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype, device=dev), torch.arange(W, dtype=dtype, device=dev), indexing="ij")
    pix_x, pix_y = xs.reshape(-1, 1), ys.reshape(-1, 1)
    conic = aux["conic"]
    dx = aux["px"][o][None] - pix_x
    dy = aux["py"][o][None] - pix_y
    power = -0.5 * (conic[o, 0][None] * dx * dx + conic[o, 2][None] * dy * dy) - conic[o, 1][None] * dx * dy
    G = torch.exp(torch.clamp(power, max=0.0))
    raw = opacities.to(dtype).reshape(-1)[o][None] * G
    alpha = raw + (torch.clamp(raw, max=0.99) - raw).detach()        # straight-through clamp
    alpha = torch.where(keep, alpha, torch.zeros_like(alpha))
    one_m = 1.0 - alpha
    T_after = torch.cumprod(one_m, dim=1)
    T_before = torch.cat([torch.ones_like(T_after[:, :1]), T_after[:, :-1]], 1)
    w = alpha * T_before
    coverage = 1.0 - one_m.prod(dim=1)
    gap = float((coverage.detach() - (1.0 - aux["T_final"].detach().reshape(-1))).abs().max())
    assert gap <= 1e-12, f"the rebuilt coverage differs from the oracle's 1 - T_final by {gap:.3e}"
    m = 1.0 / aux["depth"].to(dtype)[o]
    return w, m, keep


def compact(w, m, keep):
    """Every pixel's kept entries moved to the front, list order preserved -> (wk [Npix, K], mk [Npix, K], valid [Npix, K]); K = the longest."""
    K = max(int(keep.sum(1).max()), 1)
    idx = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :K]
    return torch.gather(w, 1, idx), m[idx], torch.gather(keep, 1, idx)


def pairwise_form(wk, mk, chunk_elems=1 << 23):
    """1/2 sum_i sum_j w_i w_j |m_i - m_j| per pixel over the compacted entries (a padding entry has w = 0); module docstring: ties."""
    n, K = wk.shape
    step = max(1, chunk_elems // (K * K))
    before = torch.ones(K, K, dtype=wk.dtype, device=wk.device).triu(1) - torch.ones(K, K, dtype=wk.dtype, device=wk.device).tril(-1)   # +1: i before j
    out = []
    for a in range(0, n, step):
        ww, mm = wk[a:a + step], mk[a:a + step]
        d = mm[:, :, None] - mm[:, None, :]
        s = torch.where(d.detach() != 0, torch.sign(d.detach()), before[None])
        out.append(0.5 * (ww[:, :, None] * ww[:, None, :] * (s * d)).sum((1, 2)))
    return torch.cat(out)


def prefix_form(wk, mk):
    """sum_k w_k (B_{k-1} - m_k A_{k-1}) in list order, A and B the running sums of w and w m."""
    A = torch.cumsum(wk, 1) - wk
    B = torch.cumsum(wk * mk, 1) - wk * mk
    return (wk * (B - mk * A)).sum(1)


def distortion_reference(opacities, image_height, image_width, opacity_factor=None, **kw):
    """rasterize_dense(opacities=opacities [* opacity_factor], **kw) -> (D [H, W] float64 with the autograd graph of the inputs, pieces): pieces
    = {"w", "m", "valid": the compacted per-pixel entries, "aux": the oracle's}.  opacity_factor: an antialiased forward's per-Gaussian factor
    (tests/test_gpu_antialiasing.py's reference: the oracle fed opacities * f)."""
    from oracle.dense_oracle import rasterize_dense
    H, W = int(image_height), int(image_width)
    op = opacities.double()
    if opacity_factor is not None:
        op = op * opacity_factor.double().reshape(op.shape)
    _, _, aux = rasterize_dense(opacities=op, image_height=H, image_width=W, **kw)
    if not aux:   # P == 0
        z = torch.zeros(H, W, dtype=torch.float64, device=opacities.device)
        return z, {"w": None, "m": None, "valid": None, "aux": aux}
    w, m, keep = rebuild_weights(aux, op, H, W)
    wk, mk, valid = compact(w, m, keep)
    return pairwise_form(wk, mk).reshape(H, W), {"w": wk, "m": mk, "valid": valid, "aux": aux}
