"""The float64 reference of the median depth and the surface hit (tests/median_reference.py) on its own: no device, no library.  The kernels
are held to it in tests/test_gpu_median.py; here the hit is checked against the definition taken entry by entry, and the condition the GPU
comparison rests on — few pixels sit within the bar of choosing another hit — is asserted for every variant that comparison uses."""
import pytest
import torch

from tests import median_reference as mref
from tests import util

VARIANTS = ["basic_deg3", "ragged_image", "long_lists", "deep", "culled", "depth_ties", "cov3D_precomp", "single"] + util.CAMERA_VARIANTS
MARGIN_SHARE = 0.05   # at most this share of the covered pixels may be within util.COLOR_TOL * tau of another hit

_CACHE = {}


def _small(tau):
    """tests/test_distortion_reference_host.py's scene (24 x 20 pixels, 40 Gaussians) at threshold tau; computed once, never written to."""
    if tau not in _CACHE:
        from das3r_amd.synth import make_scene
        sc = make_scene(P=40, W=24, H=20, focal=20.0, sh_degree=0, seed=5, s_px=(0.6, 2.5))
        mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
        _CACHE[tau] = mref.reference_of_scene(sc, mode, tau, torch.device("cpu"))
    return _CACHE[tau]


def test_scene_has_rays_with_several_contributors_and_hits_behind_the_first():
    r = _small(0.5)
    n = r["keep"].sum(1)
    first = torch.where(r["keep"], torch.arange(r["keep"].shape[1])[None], torch.full((1, 1), 10 ** 6)).min(1).values
    assert int(n.max()) >= 4 and int((n >= 2).sum()) >= 50 and int((n == 0).sum()) >= 1
    assert int((r["covered"] & (r["hit_col"] > first)).sum()) >= 20, "some hits lie behind the pixel's first contributor"
    assert int((r["covered"] & (r["hit_col"] < r["last_col"])).sum()) >= 20, "and some in front of its last one"


@pytest.mark.parametrize("tau", [0.25, 0.5, 0.75])
def test_hit_is_the_definition_taken_entry_by_entry(tau):
    r = _small(tau)
    w = r["T_before"] - r["T_after"]
    for p in range(r["keep"].shape[0]):
        hit, before, after = mref.brute_force_hit(w[p].tolist(), r["keep"][p].tolist(), tau)
        assert hit == int(r["hit_col"][p]), p
        assert float((torch.tensor(before, dtype=torch.float64) - r["T_before"][p]).abs().max()) <= 1e-12
        assert float((torch.tensor(after, dtype=torch.float64) - r["T_after"][p]).abs().max()) <= 1e-12
        if hit >= 0:
            assert int(r["hit_gaussian"][p]) == int(r["order"][hit])
            # the first entry behind which T <= tau, or the last contributor
            assert before[hit] > tau and (after[hit] <= tau or hit == int(r["last_col"][p]))
        else:
            assert not bool(r["keep"][p].any()) and float(r["depth"][p]) == 0.0 and int(r["hit_gaussian"][p]) == -1


def test_a_smaller_threshold_hits_no_nearer():
    a, b, c = _small(0.25), _small(0.5), _small(0.75)
    assert bool((a["hit_col"] >= b["hit_col"]).all()) and bool((b["hit_col"] >= c["hit_col"]).all())
    assert bool((a["depth"] >= b["depth"]).all()) and bool((b["depth"] >= c["depth"]).all())
    assert bool((a["hit_col"] > c["hit_col"]).any()), "the threshold matters on this scene"


def test_a_pixel_with_one_contributor_hits_it():
    for tau in (0.25, 0.5, 0.75):
        r = _small(tau)
        one = r["keep"].sum(1) == 1
        assert bool(one.any())
        assert torch.equal(r["hit_col"][one], r["last_col"][one])


def _share_within(r, tau):
    delta = util.COLOR_TOL * tau
    covered = r["covered"]
    return float((r["margin"][covered] < delta).double().mean()) if bool(covered.any()) else 0.0


@pytest.mark.parametrize("name,tau", [(v, 0.5) for v in VARIANTS] + [("deep", 0.05)])
def test_few_pixels_sit_within_the_bar_of_another_hit(name, tau):
    """What tests/test_gpu_median.py rests on: off these pixels an fp32 T within util.COLOR_TOL * tau of the reference's picks the reference's hit."""
    sc, mode = util.scene_variant(name)
    r = mref.reference_of_scene(sc, mode, tau, torch.device("cpu"))
    share = _share_within(r, tau)
    print(f"[{name} tau={tau}] covered {int(r['covered'].sum())} of {r['covered'].numel()} pixels, within {util.COLOR_TOL * tau:.1e} of another hit: {100 * share:.3f} %")
    assert bool(r["covered"].any())
    assert share <= MARGIN_SHARE


def test_the_deep_scene_at_a_low_threshold_hits_past_one_staged_batch():
    """tests/test_gpu_median.py's second case: the hit's rank among the pixel's own contributors is a lower bound of its list position."""
    sc, mode = util.scene_variant("deep")
    r = mref.reference_of_scene(sc, mode, 0.05, torch.device("cpu"))
    rank = (torch.cumsum(r["keep"].to(torch.int64), 1) - 1).gather(1, r["hit_col"].clamp(min=0)[:, None])[:, 0]
    rank = rank[r["covered"]]
    print(f"deep at tau 0.05: {int((rank >= 256).sum())} of {rank.numel()} hits at rank 256 or later")
    assert int((rank >= 256).sum()) >= rank.numel() // 2
