"""CPU tests of das3r_amd/csrc/kernel_choice.h: what every DAS3R_* spelling means (parse_switches) and which compositing kernel a forward
and a backward launch (choose_forward / choose_backward).  das3r_debug_parse_switches / das3r_debug_choose_* run the header's functions on
the values the test passes — never the process environment, never the switches the library itself last read.  The expected values are
written out by hand from the rules (the header's comments), not recorded from the code."""
import ctypes as C

import pytest

BUCKET = 1024   # list positions between two checkpoints of a long tile list
FWD = dict(auto=0, quad=1, rows=2, lanes=3, slices=4, regions=5)
BWD = dict(auto=0, dpp=1, mfma=2, scan=3, stream=5, blk=6, regions=7)
# an empty environment, field by field
DEFAULTS = dict(sort_ipl=0, sort_classic=0, rect_upstream=0, verbose=0, binning=0, capacity_exact=0, fused_emit_off=0, no_sh_stage=0, render_fwd=0,
                render_bwd=0, render_bwd_mb=0, render_bwd_atomic=0, render_bwd_pix=0, render_bwd_occ=0, render_bwd_strips=0, tile_chunk=-1,
                scan_items=0, deterministic=0, tile_lpt_off=0, bwd_reduce_set=0, bwd_reduce_shfl=0, ablate_set=0, ablate=0, tickets=-1,
                bwd_pad_lds=0, fwd_pad_lds=0, bwd_buckets=-1, fwd_no_prefetch=0, split_colour=0, tile_strip=8)


def parse(lib, env, experiments=0):
    from das3r_amd import _lib
    names = (C.c_char_p * max(len(env), 1))(*[k.encode() for k in env])
    values = (C.c_char_p * max(len(env), 1))(*[v.encode() for v in env.values()])
    out = _lib.Switches()
    lib.das3r_debug_parse_switches(names, values, len(env), experiments, C.byref(out))
    return out


def fields(s):
    return {n: getattr(s, n) for n, _ in s._fields_}


def expect(lib, env, experiments=0, **changed):
    """Parsing `env` gives the defaults except for `changed`."""
    assert set(changed) <= set(DEFAULTS)
    assert fields(parse(lib, env, experiments)) == {**DEFAULTS, **changed}, env


def backward(lib, sw, num_rendered, ntiles=4, flags=0):
    from das3r_amd import _lib
    out = _lib.BwdChoice()
    lib.das3r_debug_choose_backward(C.byref(sw), num_rendered, ntiles, flags, C.byref(out))
    return out


def forward(lib, sw, ntiles, capacity, local_lists=0, prefer_regions=0):
    from das3r_amd import _lib
    out = _lib.FwdChoice()
    lib.das3r_debug_choose_forward(C.byref(sw), ntiles, capacity, local_lists, prefer_regions, C.byref(out))
    return out


# ---- the parser ----

def test_an_empty_environment_gives_the_defaults(hip_lib):
    from das3r_amd import _lib
    assert [n for n, _ in _lib.Switches._fields_] == list(DEFAULTS)
    expect(hip_lib, {})
    expect(hip_lib, {}, experiments=1)
    expect(hip_lib, {"DAS3R_UNKNOWN": "1", "DAS3R_INJECT_FAULT": "1"})   # (fault injection is a call, not a variable)


# DAS3R_RENDER_BWD: kind by first letter, `stream` tested before s...; the number is the first run of digits; blk looks for p<N> and o<N>
# anywhere, fine for a q or an s anywhere; defaults mb 128 (blk, fine) / 256 (scan), occ 5, pix 0
RENDER_BWD = [
    ("dpp", dict(render_bwd=1)),
    ("mfma", dict(render_bwd=2)),
    ("scan", dict(render_bwd=3, render_bwd_mb=256)),
    ("scan64", dict(render_bwd=3, render_bwd_mb=64)),
    ("scan128", dict(render_bwd=3, render_bwd_mb=128)),
    ("scana256", dict(render_bwd=3, render_bwd_mb=256, render_bwd_atomic=1)),
    ("scana512", dict(render_bwd=3, render_bwd_mb=512, render_bwd_atomic=1)),
    ("stream", dict(render_bwd=5)),
    ("blk", dict(render_bwd=6, render_bwd_mb=128, render_bwd_pix=0, render_bwd_occ=5)),
    ("blk64", dict(render_bwd=6, render_bwd_mb=64, render_bwd_pix=0, render_bwd_occ=5)),
    ("blk128p1", dict(render_bwd=6, render_bwd_mb=128, render_bwd_pix=1, render_bwd_occ=5)),
    ("blk160p1o4", dict(render_bwd=6, render_bwd_mb=160, render_bwd_pix=1, render_bwd_occ=4)),
    ("fine", dict(render_bwd=7, render_bwd_mb=128)),
    ("fine96", dict(render_bwd=7, render_bwd_mb=96)),
    ("fine128q", dict(render_bwd=7, render_bwd_mb=128, render_bwd_strips=1)),
    ("fine128s", dict(render_bwd=7, render_bwd_mb=128, render_bwd_strips=2)),
    # spellings nobody documents, whose handling the matching rules above settle
    ("scanx", dict(render_bwd=3, render_bwd_mb=256)),                                            # no digits: the default; not "scana"
    ("scan1024", dict(render_bwd=3, render_bwd_mb=1024, render_bwd_atomic=1)),                   # 1000 and up meant the atomic flush in the old 1000 + N encoding: kept
    ("scan999", dict(render_bwd=3, render_bwd_mb=999)),
    ("blk128o4p2", dict(render_bwd=6, render_bwd_mb=128, render_bwd_pix=2, render_bwd_occ=4)),   # the suffixes in either order
    ("s", dict(render_bwd=3, render_bwd_mb=256)),                                                # an s that is not "stream": scan
    ("strea", dict(render_bwd=3, render_bwd_mb=256)),
    ("streaming", dict(render_bwd=5)),                                                           # the first six letters decide
    ("b", dict(render_bwd=6, render_bwd_mb=128, render_bwd_pix=0, render_bwd_occ=5)),
    ("d", dict(render_bwd=1)),
    ("fineq", dict(render_bwd=7, render_bwd_mb=128, render_bwd_strips=1)),
    ("x", dict()),                                                                               # no known first letter: not forced
    ("Blk", dict()),                                                                             # (case matters)
]


@pytest.mark.parametrize("spelling,changed", RENDER_BWD, ids=[s for s, _ in RENDER_BWD])
def test_render_bwd_spellings(hip_lib, spelling, changed):
    expect(hip_lib, {"DAS3R_RENDER_BWD": spelling}, **changed)
    expect(hip_lib, {"DAS3R_RENDER_BWD": spelling}, experiments=1, **changed)


@pytest.mark.parametrize("spelling,kind", [("quad", 1), ("rows", 2), ("lanes", 3), ("slices", 4), ("fine", 5), ("q", 1), ("x", 0)])
def test_render_spellings(hip_lib, spelling, kind):
    expect(hip_lib, {"DAS3R_RENDER": spelling}, render_fwd=kind)


def test_the_other_switches_of_every_build(hip_lib):
    for v, want in (("local", 1), ("radix", -1), ("seg", 2), ("seg3", 3), ("other", 0)):
        expect(hip_lib, {"DAS3R_BINNING": v}, binning=want)
    for v, want in (("always", 0), ("never", 1 << 30), ("12", 12), ("junk", -1), ("0", -1)):
        expect(hip_lib, {"DAS3R_TICKETS": v}, tickets=want)
    for v, want in (("0", 0), ("8", 8), ("12", -1), ("128", -1), ("64", 64), ("-2", -1)):   # a power of two in 0 .. 64, else the default
        expect(hip_lib, {"DAS3R_TILE_CHUNK": v}, tile_chunk=want)
    for v, want in (("-3", 0), ("8", 8), ("200", 63), ("0", 0)):                           # clamped to 0 .. 63
        expect(hip_lib, {"DAS3R_TILE_STRIP": v}, tile_strip=want)
    for v, want in (("0", -1), ("1", 1), ("2", 0)):
        expect(hip_lib, {"DAS3R_SPLIT_COLOUR": v}, split_colour=want)
    expect(hip_lib, {"DAS3R_RECT": "upstream"}, rect_upstream=1)
    expect(hip_lib, {"DAS3R_RECT": "tight"})
    expect(hip_lib, {"DAS3R_VERBOSE": "0"}, verbose=1)   # set at all
    expect(hip_lib, {"DAS3R_CAPACITY": "exact"}, capacity_exact=1)
    expect(hip_lib, {"DAS3R_FUSED_EMIT": "0"}, fused_emit_off=1)
    expect(hip_lib, {"DAS3R_FUSED_EMIT": "1"})
    expect(hip_lib, {"DAS3R_TILE_LPT": "0"}, tile_lpt_off=1)
    expect(hip_lib, {"DAS3R_BWD_REDUCE": "shfl"}, bwd_reduce_set=1, bwd_reduce_shfl=1)
    expect(hip_lib, {"DAS3R_BWD_REDUCE": "dpp"}, bwd_reduce_set=1)
    expect(hip_lib, {"DAS3R_DETERMINISTIC": "1"}, deterministic=1)
    expect(hip_lib, {"DAS3R_DETERMINISTIC": "0"})
    expect(hip_lib, {"DAS3R_BWD_BUCKETS": "0"}, bwd_buckets=0)
    expect(hip_lib, {"DAS3R_BWD_BUCKETS": "7"}, bwd_buckets=7)
    # several at once
    expect(hip_lib, {"DAS3R_RENDER_BWD": "blk192", "DAS3R_BINNING": "seg3", "DAS3R_RENDER": "rows"}, render_bwd=6, render_bwd_mb=192, render_bwd_occ=5,
           binning=3, render_fwd=2)


def test_an_empty_string_counts_as_unset(hip_lib):
    every = ("DAS3R_RENDER", "DAS3R_RENDER_BWD", "DAS3R_BINNING", "DAS3R_TICKETS", "DAS3R_TILE_CHUNK", "DAS3R_TILE_STRIP", "DAS3R_SPLIT_COLOUR",
             "DAS3R_RECT", "DAS3R_VERBOSE", "DAS3R_CAPACITY", "DAS3R_FUSED_EMIT", "DAS3R_TILE_LPT", "DAS3R_BWD_REDUCE", "DAS3R_DETERMINISTIC",
             "DAS3R_BWD_BUCKETS")
    expect(hip_lib, {k: "" for k in every})
    experiments_only = ("DAS3R_SORT_IPL", "DAS3R_SORT", "DAS3R_ABLATE", "DAS3R_BWD_PAD_LDS", "DAS3R_FWD_PAD_LDS", "DAS3R_SCAN_ITEMS", "DAS3R_FWD_PREFETCH")
    expect(hip_lib, {k: "" for k in every + experiments_only}, experiments=1)
    # the one switch whose presence alone counts, as it always has (an experiments build's getenv(...) != NULL)
    expect(hip_lib, {"DAS3R_NO_SH_STAGE": ""}, experiments=1, no_sh_stage=1)


EXPERIMENT_ONLY = [
    ("DAS3R_SORT_IPL", "8", dict(sort_ipl=8)),
    ("DAS3R_SORT", "classic", dict(sort_classic=1)),
    ("DAS3R_NO_SH_STAGE", "1", dict(no_sh_stage=1)),
    ("DAS3R_ABLATE", "3", dict(ablate_set=1, ablate=3)),
    ("DAS3R_BWD_PAD_LDS", "4096", dict(bwd_pad_lds=4096)),
    ("DAS3R_FWD_PAD_LDS", "2048", dict(fwd_pad_lds=2048)),
    ("DAS3R_SCAN_ITEMS", "16", dict(scan_items=16)),
    ("DAS3R_FWD_PREFETCH", "0", dict(fwd_no_prefetch=1)),
]


@pytest.mark.parametrize("name,value,changed", EXPERIMENT_ONLY, ids=[n for n, _, _ in EXPERIMENT_ONLY])
def test_experiment_only_variables_are_read_by_an_experiments_build_alone(hip_lib, name, value, changed):
    expect(hip_lib, {name: value}, experiments=0)
    expect(hip_lib, {name: value}, experiments=1, **changed)


def test_experiment_only_values_outside_their_sets(hip_lib):
    expect(hip_lib, {"DAS3R_SORT_IPL": "5"}, experiments=1)      # 4 | 8 | 16
    expect(hip_lib, {"DAS3R_SCAN_ITEMS": "3"}, experiments=1)    # 1 | 2 | 4 | 8 | 16
    expect(hip_lib, {"DAS3R_SORT": "onesweep"}, experiments=1)
    expect(hip_lib, {"DAS3R_FWD_PREFETCH": "1"}, experiments=1)


# ---- the backward choice ----

def check_bwd(c, kernel, mb=None, slices=None, **more):
    assert c.kernel == BWD[kernel], (c.kernel, kernel)
    if mb is not None:
        assert c.mb == mb
    if slices is not None:
        assert c.slices == slices
    for k, v in more.items():
        assert getattr(c, k) == v, k


def test_backward_by_mean_list_length(hip_lib):
    """ntiles = 4.  Mean list (num_rendered / ntiles, rounded down) < 96: pixel per lane; from 96: the block walk with 128-entry rounds and the
    per-pixel constants in LDS (pix 1); from 1024: 192-entry rounds, constants in registers (pix 0)."""
    sw = parse(hip_lib, {})
    check_bwd(backward(hip_lib, sw, 4 * 95), "dpp", slices=1)
    check_bwd(backward(hip_lib, sw, 4 * 96 - 1), "dpp")
    check_bwd(backward(hip_lib, sw, 4 * 96), "blk", 128, 1, pix=1, occ=5)
    check_bwd(backward(hip_lib, sw, 4 * 1023), "blk", 128, 1, pix=1)
    check_bwd(backward(hip_lib, sw, 4 * 1024 - 1), "blk", 128, 1)
    check_bwd(backward(hip_lib, sw, 4 * 1024), "blk", 192, 1, pix=0, occ=5)


def test_backward_regions_need_long_lists_the_forwards_hint_and_few_tiles(hip_lib):
    sw = parse(hip_lib, {})
    check_bwd(backward(hip_lib, sw, 4 * 1024, flags=1), "regions", 128, 1, strips=0)
    check_bwd(backward(hip_lib, sw, 4 * 1023, flags=1), "blk", 128)          # not long enough
    check_bwd(backward(hip_lib, sw, 4 * 1024, flags=2 | 4 | 16), "blk", 192)   # the other flag bits are not the hint
    check_bwd(backward(hip_lib, sw, 1024 * 1024, ntiles=1024, flags=1), "regions", 128)
    check_bwd(backward(hip_lib, sw, 1025 * 1024, ntiles=1025, flags=1), "blk", 192)


def test_backward_with_ablate_set_never_takes_the_region_walk(hip_lib):
    """DAS3R_ABLATE (experiments build: perf experiments on the pixel-per-lane kernel) with long lists and the forward's hint: not the region
    walk.  The rule has a guard of its own for that (`&& !ablate_set`), but ablate_set has sent the unforced choice to the pixel-per-lane
    kernel before the guard is reached — so what is launched, today and before this header existed, is dpp, not blk as a reading of the
    guard alone suggests.  Asserted as it is: this header must not change which kernel a run takes."""
    abl = parse(hip_lib, {"DAS3R_ABLATE": "0"}, experiments=1)
    assert abl.ablate_set == 1
    for ntiles in (4, 1024, 1025):
        c = backward(hip_lib, abl, ntiles * 1024, ntiles=ntiles, flags=1)
        assert c.kernel != BWD["regions"]
        check_bwd(c, "dpp")
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_ABLATE": "0"}, experiments=0), 4 * 1024, flags=1), "regions", 128)   # (the shipped build does not read it)


def test_backward_deterministic_and_reference_reduction(hip_lib):
    det = parse(hip_lib, {"DAS3R_DETERMINISTIC": "1"})
    check_bwd(backward(hip_lib, det, 4 * 10), "blk", 64, 1, pix=0, occ=5)      # short lists too on the block walk
    check_bwd(backward(hip_lib, det, 4 * 96), "blk", 128, pix=1)               # long lists: as without
    check_bwd(backward(hip_lib, det, 4 * 1024, flags=1), "regions", 128)
    red = parse(hip_lib, {"DAS3R_BWD_REDUCE": "shfl"})
    check_bwd(backward(hip_lib, red, 4 * 5000), "dpp")                         # the reference reduction is the pixel-per-lane kernel's
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_BWD_REDUCE": "dpp"}), 4 * 5000, flags=1), "dpp")


def test_backward_slices(hip_lib):
    """slices = min(32, max(1, num_rendered / (BUCKET * ntiles))): the buckets of an average tile."""
    sw = parse(hip_lib, {})
    n = lambda buckets_per_tile: 4 * BUCKET * buckets_per_tile
    check_bwd(backward(hip_lib, sw, n(1)), "blk", 192, 1)
    check_bwd(backward(hip_lib, sw, n(2) - 1), "blk", 192, 1)
    check_bwd(backward(hip_lib, sw, n(2)), "blk", 192, 2)
    check_bwd(backward(hip_lib, sw, n(32)), "blk", 192, 32)
    check_bwd(backward(hip_lib, sw, n(40)), "blk", 192, 32)
    # rounds of more than 256 entries have no bucket-parallel form
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk256"}), n(8)), "blk", 256, 8)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk320"}), n(8)), "blk", 320, 1)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "scan512"}), n(8)), "scan", 512, 1, atomic_flush=0)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "scana256"}), n(8)), "scan", 256, 1, atomic_flush=1)   # nor has the atomic flush
    # DAS3R_BWD_BUCKETS forces the count (0: off), whatever the lists
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_BWD_BUCKETS": "0"}), n(8)), "blk", 192, 0)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_BWD_BUCKETS": "7"}), n(8)), "blk", 192, 7)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_BWD_BUCKETS": "7"}), n(1)), "blk", 192, 7)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_BWD_BUCKETS": "7", "DAS3R_RENDER_BWD": "blk320"}), n(8)), "blk", 320, 1)


def test_backward_hint_of_the_longest_list(hip_lib):
    """flags bits 8 - 15: buckets of the longest list the forward measured.  The region walk launches that many workgroups per tile (at most 64)
    when it is bucket-parallel anyway and the count is not forced."""
    sw = parse(hip_lib, {})
    n = 4 * BUCKET * 8   # 8 buckets per tile on average
    hint = lambda h: 1 | (h << 8)
    check_bwd(backward(hip_lib, sw, n, flags=hint(50)), "regions", 128, 50)
    check_bwd(backward(hip_lib, sw, n, flags=hint(200)), "regions", 128, 64)
    check_bwd(backward(hip_lib, sw, n, flags=hint(8)), "regions", 128, 8)      # not longer than the mean's
    check_bwd(backward(hip_lib, sw, n, flags=hint(5)), "regions", 128, 8)
    check_bwd(backward(hip_lib, sw, n, flags=50 << 8), "blk", 192, 8)          # ignored for blk (bit 0 clear)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk192"}), n, flags=hint(50)), "blk", 192, 8)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_BWD_BUCKETS": "4"}), n, flags=hint(50)), "regions", 128, 4)    # forced count
    check_bwd(backward(hip_lib, sw, 4 * BUCKET, flags=hint(50)), "regions", 128, 1)                                   # slices <= 1: not bucket-parallel
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "fine"}), n, flags=hint(50)), "regions", 128, 50)   # forced kind: the hint still counts


FORCED_BWD = [("dpp", "dpp", 256), ("mfma", "mfma", 256), ("scan", "scan", 256), ("scan64", "scan", 64), ("scana512", "scan", 512),
              ("stream", "stream", 256), ("blk", "blk", 128), ("blk64", "blk", 64), ("blk160p1o4", "blk", 160), ("fine", "regions", 128),
              ("fine96", "regions", 96)]


@pytest.mark.parametrize("spelling,kernel,mb", FORCED_BWD, ids=[s for s, _, _ in FORCED_BWD])
def test_a_forced_backward_passes_through_with_its_mb(hip_lib, spelling, kernel, mb):
    sw = parse(hip_lib, {"DAS3R_RENDER_BWD": spelling})
    for num_rendered, flags in ((40, 0), (4 * 600, 0), (4 * 5000, 1)):   # whatever the lists and the hint
        check_bwd(backward(hip_lib, sw, num_rendered, flags=flags), kernel, mb)


def test_the_forms_a_forced_backward_asks_for(hip_lib):
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk128"}), 4 * 600), "blk", 128, pix=0, occ=5)   # forced: the spelling's pix, not the default's
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk128p1"}), 4 * 600), "blk", 128, pix=1, occ=5)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk128p2o4"}), 4 * 600), "blk", 128, pix=2, occ=4)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "fine128q"}), 4 * 600), "regions", 128, strips=1)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "fine128s"}), 4 * 600), "regions", 128, strips=2)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "scana256"}), 4 * 600), "scan", 256, atomic_flush=1)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "scan256"}), 4 * 600), "scan", 256, atomic_flush=0)


def test_backward_of_nothing_does_not_divide_by_zero(hip_lib):
    sw = parse(hip_lib, {})
    check_bwd(backward(hip_lib, sw, 0), "dpp", slices=1)
    check_bwd(backward(hip_lib, sw, 0, ntiles=0), "dpp", slices=1)
    check_bwd(backward(hip_lib, sw, 5000, ntiles=0), "blk", 192, 4)   # (ntiles counts as 1)
    check_bwd(backward(hip_lib, parse(hip_lib, {"DAS3R_RENDER_BWD": "blk"}), 0, ntiles=0), "blk", 128, 1)


# ---- the forward choice ----

def check_fwd(c, kernel, **more):
    assert c.kernel == FWD[kernel], (c.kernel, kernel)
    for k, v in more.items():
        assert getattr(c, k) == v, k


def test_forward_by_capacity_and_tile_count(hip_lib):
    sw = parse(hip_lib, {})
    for ntiles in (4, 1024, 1025, 8160):
        check_fwd(forward(hip_lib, sw, ntiles, 128 * ntiles - 1), "quad", quad_lanes=0, row_private=0, tile_lpt=0)
        check_fwd(forward(hip_lib, sw, ntiles, 128 * ntiles), "rows", quad_lanes=0, row_private=1)
        check_fwd(forward(hip_lib, sw, ntiles, 1024 * ntiles - 1), "rows", quad_lanes=0)
    check_fwd(forward(hip_lib, sw, 4, 1024 * 4), "lanes", quad_lanes=1)
    check_fwd(forward(hip_lib, sw, 1024, 1024 * 1024), "lanes", quad_lanes=1)
    check_fwd(forward(hip_lib, sw, 1025, 1024 * 1025), "rows", quad_lanes=0, row_private=1)   # too many tiles for a workgroup per tile to pay
    check_fwd(forward(hip_lib, sw, 4, 0), "quad")


def test_forward_regions_where_the_lists_are_skewed(hip_lib):
    sw = parse(hip_lib, {})
    check_fwd(forward(hip_lib, sw, 1024, 1024 * 1024, prefer_regions=1), "regions", quad_lanes=1, tile_lpt=1)
    check_fwd(forward(hip_lib, sw, 1024, 1024 * 1024 - 1, prefer_regions=1), "rows", tile_lpt=0)   # only where the lanes kernel would run
    check_fwd(forward(hip_lib, sw, 1025, 1024 * 1025, prefer_regions=1), "rows", tile_lpt=0)


@pytest.mark.parametrize("forced", ["quad", "rows", "lanes", "slices", "fine"])
def test_local_lists_never_take_the_kernels_that_cannot_sort(hip_lib, forced):
    """Lists in local depth order are sorted by the quad and rows kernels themselves: lanes / slices / regions are never chosen for them,
    whatever is forced."""
    for env in ({}, {"DAS3R_RENDER": forced}):
        sw = parse(hip_lib, env)
        for ntiles, cap in ((4, 4 * 100), (4, 4 * 600), (4, 4 * 2000), (2000, 2000 * 2000)):
            for regions in (0, 1):
                c = forward(hip_lib, sw, ntiles, cap, local_lists=1, prefer_regions=regions)
                assert c.kernel in (FWD["quad"], FWD["rows"]) and c.quad_lanes == 0 and c.tile_lpt == 0
    # forced lanes / slices / fine on local lists: by length, as unforced
    if forced in ("lanes", "slices", "fine"):
        sw = parse(hip_lib, {"DAS3R_RENDER": forced})
        check_fwd(forward(hip_lib, sw, 4, 4 * 128 - 1, local_lists=1), "quad")
        check_fwd(forward(hip_lib, sw, 4, 4 * 128, local_lists=1), "rows")


def test_each_forced_forward(hip_lib):
    shapes = ((4, 40), (4, 4 * 600), (4, 4 * 2000), (2000, 2000 * 2000))
    for ntiles, cap in shapes:
        for regions in (0, 1):
            check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_RENDER": "quad"}), ntiles, cap, 0, regions), "quad", quad_lanes=0, row_private=0)
            check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_RENDER": "rows"}), ntiles, cap, 0, regions), "rows", quad_lanes=0, row_private=1)
            check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_RENDER": "lanes"}), ntiles, cap, 0, regions), "lanes", quad_lanes=1)
            check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_RENDER": "slices"}), ntiles, cap, 0, regions), "slices", quad_lanes=1)
            check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_RENDER": "fine"}), ntiles, cap, 0, regions), "regions", quad_lanes=1)


def test_tile_order_longest_first(hip_lib):
    """Only with the region kernel chosen for a shape the forwards found skewed, ntiles <= 1024, DAS3R_TILE_LPT not 0, DAS3R_RENDER unset or fine."""
    long = lambda ntiles: 1024 * ntiles
    check_fwd(forward(hip_lib, parse(hip_lib, {}), 4, long(4), 0, 1), "regions", tile_lpt=1)
    check_fwd(forward(hip_lib, parse(hip_lib, {}), 4, long(4), 0, 0), "lanes", tile_lpt=0)
    check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_TILE_LPT": "0"}), 4, long(4), 0, 1), "regions", tile_lpt=0)
    check_fwd(forward(hip_lib, parse(hip_lib, {"DAS3R_TILE_LPT": "1"}), 4, long(4), 0, 1), "regions", tile_lpt=1)
    fine = parse(hip_lib, {"DAS3R_RENDER": "fine"})
    check_fwd(forward(hip_lib, fine, 4, long(4), 0, 1), "regions", tile_lpt=1)
    check_fwd(forward(hip_lib, fine, 4, 40, 0, 1), "regions", tile_lpt=1)        # forced: whatever the length
    check_fwd(forward(hip_lib, fine, 4, 0, 0, 1), "regions", tile_lpt=0)         # ... but not of nothing
    check_fwd(forward(hip_lib, fine, 4, long(4), 0, 0), "regions", tile_lpt=0)   # the shape was not found skewed
    check_fwd(forward(hip_lib, fine, 1025, long(1025), 0, 1), "regions", tile_lpt=0)
    check_fwd(forward(hip_lib, fine, 1024, long(1024), 0, 1), "regions", tile_lpt=1)
    for other in ("lanes", "slices", "rows", "quad"):
        assert forward(hip_lib, parse(hip_lib, {"DAS3R_RENDER": other}), 4, long(4), 0, 1).tile_lpt == 0
    assert forward(hip_lib, parse(hip_lib, {}), 4, long(4), 1, 1).tile_lpt == 0   # local lists


# ---- inverse depth ----

def test_which_kernels_have_an_inverse_depth_form_and_what_the_messages_call_them(hip_lib):
    fwd_names = {0: "auto", 1: "quad", 2: "rows", 3: "lanes", 4: "slices", 5: "fine"}
    bwd_names = {0: "auto", 1: "dpp", 2: "mfma", 3: "scan", 5: "stream", 6: "blk", 7: "fine"}
    for k, name in fwd_names.items():
        assert bool(hip_lib.das3r_debug_has_invdepth_form(0, k)) == (k != FWD["slices"]), name
        assert hip_lib.das3r_debug_kernel_name(0, k) == name.encode()
    for k, name in bwd_names.items():
        assert bool(hip_lib.das3r_debug_has_invdepth_form(1, k)) == (k not in (BWD["mfma"], BWD["scan"], BWD["stream"])), name
        assert hip_lib.das3r_debug_kernel_name(1, k) == name.encode()
    # a spelling's name is what the refusal quotes: tests/test_invdepth_host.py, tests/test_focal_host.py assert the whole messages
    for spelling, name in (("scan128", "scan"), ("scana512", "scan"), ("mfma", "mfma"), ("stream", "stream")):
        k = parse(hip_lib, {"DAS3R_RENDER_BWD": spelling}).render_bwd
        assert not hip_lib.das3r_debug_has_invdepth_form(1, k) and hip_lib.das3r_debug_kernel_name(1, k) == name.encode()
    k = parse(hip_lib, {"DAS3R_RENDER": "slices"}).render_fwd
    assert not hip_lib.das3r_debug_has_invdepth_form(0, k) and hip_lib.das3r_debug_kernel_name(0, k) == b"slices"
