"""Float64 reference of the median depth and the surface hit (include/das3r_raster.h das3r_raster_median_forward).  TEST INFRASTRUCTURE ONLY.

It calls oracle.dense_oracle.rasterize_dense and rebuilds the blending weights with tests.distortion_reference.rebuild_weights (which asserts
the rebuilt coverage against the oracle's 1 - T_final on every call).  From the weights w over the kept entries, in the oracle's global
(depth, index) order — which, restricted to a pixel's kept entries, is the order of its tile's list:
  * T_after_k  = 1 - sum_{j<=k} w_j   and   T_before_k = T_after_k + w_k   (w_k = alpha_k T_before_k, so sum_{j<k} w_j = 1 - T_before_k);
  * hit        = the last kept column with T_before > tau (column 0 of a covered pixel has T_before = 1 > tau: every covered pixel has one);
  * margin     = min over the kept entries of |T_after_k - tau|: how far the pixel is from choosing another hit.  An fp32 kernel whose T is
                 within delta of the reference's picks the same hit on every pixel whose margin is at least delta.
Nothing here carries an autograd graph: the hit is a selection."""
import torch

from tests.distortion_reference import rebuild_weights


def hits_from_weights(w, keep, depth_sorted, order, tau):
    """w, keep [Npix, P] in the global order, depth_sorted [P] = depth[order], order [P] -> dict of
    T_before / T_after [Npix, P] float64, keep [Npix, P], covered [Npix] bool, hit_col [Npix] int64 (-1: empty pixel), hit_gaussian [Npix]
    int64 (-1), depth [Npix] float64 (0), last_col [Npix] int64 (the last kept column, -1), margin [Npix] float64 (inf: empty pixel)."""
    w = w.detach()
    T_after = 1.0 - torch.cumsum(w, 1)
    T_before = T_after + w
    cols = torch.arange(w.shape[1], device=w.device)[None]
    minus = torch.full_like(cols, -1)
    hit_col = torch.where(keep & (T_before > tau), cols, minus).max(1).values
    last_col = torch.where(keep, cols, minus).max(1).values
    covered = keep.any(1)
    assert bool((hit_col[covered] >= 0).all()) and bool((hit_col[~covered] == -1).all()), "T_0 = 1 > tau: a pixel has a hit iff it has a contributor"
    safe = hit_col.clamp(min=0)
    hit_gaussian = torch.where(covered, order[safe], torch.full_like(safe, -1))
    depth = torch.where(covered, depth_sorted.detach().double()[safe], torch.zeros_like(T_after[:, 0]))
    inf = torch.full_like(T_after, float("inf"))
    margin = torch.where(keep, (T_after - tau).abs(), inf).min(1).values
    return dict(T_before=T_before, T_after=T_after, keep=keep, covered=covered, hit_col=hit_col, hit_gaussian=hit_gaussian, depth=depth,
                last_col=last_col, margin=margin, order=order)


def median_reference(opacities, image_height, image_width, threshold=0.5, opacity_factor=None, **kw):
    """rasterize_dense(opacities=opacities [* opacity_factor], **kw) -> hits_from_weights' dict (+ "H", "W"); None for P == 0.  opacity_factor:
    an antialiased forward's per-Gaussian factor (tests/test_gpu_antialiasing.py's reference: the oracle fed opacities * f)."""
    from oracle.dense_oracle import rasterize_dense
    H, W = int(image_height), int(image_width)
    op = opacities.double()
    if opacity_factor is not None:
        op = op * opacity_factor.double().reshape(op.shape)
    with torch.no_grad():
        _, _, aux = rasterize_dense(opacities=op, image_height=H, image_width=W, **kw)
        if not aux:
            return None
        w, _, keep = rebuild_weights(aux, op, H, W)
        out = hits_from_weights(w, keep, aux["depth"][aux["order"]], aux["order"], float(threshold))
    out["H"], out["W"] = H, W
    return out


def reference_of_scene(sc, mode, threshold, device, antialiased=False):
    """median_reference of a tests/util.py scene (scene_variant's pair) on `device`; colours play no part: zeros.  antialiased: the oracle fed
    opacities * f, f from the conic of a first dense call (tests/test_gpu_antialiasing.py's reference)."""
    from tests import util
    kw = {k: v.to(device).double() for k, v in util.raster_inputs(sc, mode).items() if k not in ("shs", "colors_precomp")}
    kw["means2D"] = torch.zeros(sc.P, 3, dtype=torch.float64, device=device)
    skw = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    colors = torch.zeros(sc.P, 3, dtype=torch.float64, device=device)
    factor = None
    if antialiased:
        from oracle.dense_oracle import rasterize_dense
        from tests.test_gpu_antialiasing import aa_factor
        with torch.no_grad():
            factor = aa_factor(rasterize_dense(colors_precomp=colors, **kw, **skw)[2]["conic"])[0][:, None]
    rest = {k: v for k, v in kw.items() if k != "opacities"}
    return median_reference(kw["opacities"], threshold=threshold, opacity_factor=factor, colors_precomp=colors, **rest, **skw)


def brute_force_hit(w_row, keep_row, tau):
    """The definition, entry by entry, for one pixel, on its own running product: alpha_k = w_k / T_k, T_{k+1} = T_k (1 - alpha_k) ->
    (hit column or -1, [T_before], [T_after]) over all columns (kept or not)."""
    T, hit, before, after = 1.0, -1, [], []
    for k in range(len(w_row)):
        before.append(T)
        if keep_row[k]:
            if T > tau:
                hit = k
            T = T * (1.0 - float(w_row[k]) / T)
        after.append(T)
    return hit, before, after
