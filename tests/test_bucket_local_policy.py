"""CPU tests of the planning rule of the fourth binning plan (das3r_amd/csrc/path_policy.h bucket_local_rule: segmented emission, the lists
finished by the compositing kernel), through das3r_debug_path_policy_* as tests/test_path_policy_host.py drives the other three.  The plan
struct reports it as seg == 2 (1: the segmented path with its segment sort).

The rule, from the call's shape alone: one-sweep binning, at least two key bits free beside the tile ids in the passes they need anyway,
more than 1024 tiles, and the learnt mean list in (256, 384] — 256 being where the rank sort fused with the staging stops taking a list,
384 the LOCAL_AVG up to which the local order is taken at all.  The expected plans are worked out by hand from that."""
import ctypes as C

import pytest

from tests.test_path_policy_host import Shape

LOCAL, SEG, BUCKET, RADIX = (1, 0), (0, 1), (0, 2), (0, 0)
# the bench shapes: name -> (P, W, H, mean tile list as the ledger quotes it)
C1 = (10_000, 256, 256, 40)
C2 = (100_000, 1920, 1080, 32)
C4 = (1_000_000, 1920, 1080, 320)
DS = (5_000_000, 512, 208, 14_000)
TRAIN = (20 * 512 * 208, 512, 208, 5_000)   # the train step renders one 512 x 208 frame of a 20-frame model


@pytest.fixture
def shape(hip_lib):
    return Shape(hip_lib)


def set_shape(shape, P, W, H):
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    tbits = max(1, (ntiles - 1).bit_length())
    shape.shape(P=P, W=W, H=H, ntiles=ntiles, tbits=tbits)
    return ntiles


def steady_plan(shape, P, W, H, mean):
    """The plan of the shape's forwards once its count is known (the second forward on)."""
    ntiles = set_shape(shape, P, W, H)
    shape.plan()
    shape.count(mean * ntiles)
    p = shape.plan()
    shape.count(mean * ntiles)
    q = shape.plan()
    assert (p.local, p.seg, p.seg_bits, p.seg_passes) == (q.local, q.seg, q.seg_bits, q.seg_passes), "the plan is stable"
    return p, ntiles


@pytest.mark.parametrize("name, dims, want", [("c1", C1, LOCAL), ("c2", C2, LOCAL), ("c4", C4, BUCKET), ("ds", DS, SEG), ("dsc", DS, SEG),
                                              ("train", TRAIN, SEG)])
def test_bench_shapes_plan_as_expected(shape, name, dims, want):
    """C4 (8160 tiles: 13 bits of tile id, two passes, three free bits; mean list 320) takes the new plan; C1 (256 tiles, no free bit),
    C2 (mean 32), DS / DSC and the train step (416 tiles, lists of thousands) plan exactly as before it existed."""
    p, ntiles = steady_plan(shape, *dims)
    assert (p.local, p.seg) == want, name
    if want == BUCKET:
        assert (p.seg_bits, p.seg_passes, p.speculate) == (3, 2, 1), "the tile ids' own passes, their three free bits, speculative as the local order is"
        assert shape.s.last_seg == 0, "a list too long for LDS backs off as the local order does, not by one more pass"
        assert shape.forward(320 * ntiles) == "seg2"   # (how tests/test_path_policy_host.py names a plan with seg set)


def test_first_forward_of_c4_is_the_local_order(shape):
    """No history, no rule: the first forward of a shape plans the local order tentatively, as it always did."""
    set_shape(shape, *C4[:3])
    p = shape.plan()
    assert (p.local, p.seg, p.speculate) == (1, 0, 0)


@pytest.mark.parametrize("mean, want", [(256, LOCAL), (257, BUCKET), (320, BUCKET), (384, BUCKET), (385, SEG)])
def test_window_edges_on_the_mean_list(shape, mean, want):
    """(256, 384] x ntiles on the last count: at 256 the local order as before, from 257 the new plan, up to LOCAL_AVG; above it what the
    shape took before (385 x 8160 >> 3 bucket bits is far below SEG_AVG x 8160: the segmented path)."""
    ntiles = set_shape(shape, *C4[:3])
    shape.plan()
    shape.count(mean * ntiles)
    p = shape.plan()
    assert (p.local, p.seg) == want, mean
    shape.count(mean * ntiles + 1)        # one instance past the edge
    p = shape.plan()
    assert (p.local, p.seg) == {256: BUCKET, 384: SEG}.get(mean, want)


@pytest.mark.parametrize("W, H, want", [(512, 512, LOCAL), (528, 512, BUCKET)])
def test_window_edge_on_the_tile_count(shape, W, H, want):
    """More than 1024 tiles: 32 x 32 tiles keep the local order, 33 x 32 take the plan (11 bits of tile id in two passes: five free)."""
    p, _ = steady_plan(shape, 400_000, W, H, 320)
    assert (p.local, p.seg) == want


def test_no_free_key_bits_no_plan(shape):
    """seg_dbits(tbits, tile_passes) >= 2: 2^15 tiles in two passes leave one bit — the local order; 2^14 leave two."""
    for tbits, want in ((15, LOCAL), (14, BUCKET)):
        shape.shape(P=3_000_000, W=16 << (tbits // 2 + tbits % 2), H=16 << (tbits // 2), ntiles=1 << tbits, tbits=tbits)
        shape.plan()
        shape.count(320 << tbits)
        p = shape.plan()
        assert (p.local, p.seg) == want, tbits


def test_back_off_and_classic_passes_keep_their_paths(shape):
    """In the middle of a stint on the global sort the rule does not fire; nor without the one-sweep passes."""
    ntiles = set_shape(shape, *C4[:3])
    shape.plan()
    shape.count(320 * ntiles)
    shape.s.radix_left = 3
    p = shape.plan()
    assert (p.local, p.seg) == RADIX and shape.s.radix_left == 2
    shape.s.radix_left = 0
    shape.onesweep = 0
    p = shape.plan()
    assert (p.local, p.seg) == RADIX


def test_too_long_under_the_plan_is_the_local_orders_back_off(shape):
    """A list that outgrew LDS under the plan (the compositing kernel raises too_long, as on the local path): global sort for 64 forwards,
    no extra partition pass."""
    ntiles = set_shape(shape, *C4[:3])
    shape.plan()
    shape.count(320 * ntiles)
    p = shape.plan()
    assert (p.local, p.seg) == BUCKET
    shape.count(320 * ntiles)
    p = shape.plan(too_long=shape.s.gen)
    assert (p.local, p.seg) == RADIX and shape.s.seg_extra == 0 and shape.s.radix_left == 63


@pytest.mark.parametrize("tbits, onesweep, want", [(5, 1, (0, 2, 3, 1)), (4, 1, (0, 2, 4, 1)), (13, 1, (0, 2, 3, 2)),
                                                   (8, 1, (1, 0, 0, 1)),      # no bucket bit beside eight bits of tile id: the local order
                                                   (7, 1, (1, 0, 1, 1)),      # one bit: not enough either
                                                   (5, 0, (0, 0, 0, 1))])     # the classic passes have no fast path
def test_forced_spelling(hip_lib, shape, tbits, onesweep, want):
    """DAS3R_BINNING=bucket parses to 4 and forces the plan wherever the key has two bucket bits, whatever the history says: from a shape's
    first forward on, at any tile count and list length, in the middle of a stint."""
    from das3r_amd import _lib
    names = (C.c_char_p * 1)(b"DAS3R_BINNING")
    values = (C.c_char_p * 1)(b"bucket")
    sw = _lib.Switches()
    hip_lib.das3r_debug_parse_switches(names, values, 1, 0, C.byref(sw))
    assert sw.binning == 4
    shape.shape(P=1000, W=64, H=64, ntiles=1 << tbits, tbits=tbits)
    shape.forced, shape.onesweep = sw.binning, onesweep
    p = shape.plan()
    assert (p.local, p.seg, p.seg_bits, p.seg_passes) == want
    assert not shape.count(10 ** 9)
    shape.s.radix_left = 5
    p = shape.plan()
    assert (p.local, p.seg, p.seg_bits, p.seg_passes) == want and shape.s.radix_left == 5


@pytest.mark.parametrize("spelling, forced, want", [("local", 1, (1, 0, 2)), ("radix", -1, (0, 0, 2)), ("seg", 2, (0, 1, 2)), ("seg3", 3, (0, 1, 3))])
def test_the_other_spellings_are_unchanged_at_c4(hip_lib, shape, spelling, forced, want):
    from das3r_amd import _lib
    names = (C.c_char_p * 1)(b"DAS3R_BINNING")
    values = (C.c_char_p * 1)(spelling.encode())
    sw = _lib.Switches()
    hip_lib.das3r_debug_parse_switches(names, values, 1, 0, C.byref(sw))
    assert sw.binning == forced
    ntiles = set_shape(shape, *C4[:3])
    shape.forced = forced
    shape.plan()
    shape.count(320 * ntiles)
    p = shape.plan()
    assert (p.local, p.seg, p.seg_passes) == want
