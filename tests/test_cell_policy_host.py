"""CPU tests of the planning rule of the fifth binning plan, "cells" (das3r_amd/csrc/path_policy.h cells_rule: the bucket plan's emission
and finish, the instances partitioned by reserved ranges and finished per cell, csrc/cell_sort.hip), through das3r_debug_path_policy_* as
tests/test_bucket_local_policy.py drives the fourth.  The plan struct reports it as seg == 2 — the compositing kernel finishes the lists,
as under the bucket plan — with cells == 1.

The rule: wherever bucket_local_rule holds and the tile ids take at most two partition passes (a partition key of 8 or 16 bits: up to
2^14 tiles), by shape (ledger (cr): adopted after the interleaved sessions) or forced with DAS3R_BINNING=cells (5).  Back-off is the
bucket plan's: too_long sends the shape to the global sort for a stint, no extra pass.  The expected plans are worked out by hand."""
import ctypes as C

import pytest

from tests.test_bucket_local_policy import C1, C2, C4, DS, TRAIN, set_shape, steady_plan
from tests.test_path_policy_host import Shape


@pytest.fixture
def shape(hip_lib):
    return Shape(hip_lib)


def kind(p):
    return (p.local, p.seg, p.cells)


LOCAL, SEG, BUCKET, CELLS, RADIX = (1, 0, 0), (0, 1, 0), (0, 2, 0), (0, 2, 1), (0, 0, 0)


@pytest.mark.parametrize("name, dims, want", [("c1", C1, LOCAL), ("c2", C2, LOCAL), ("c4", C4, CELLS), ("ds", DS, SEG), ("dsc", DS, SEG), ("train", TRAIN, SEG)])
def test_bench_shapes(shape, name, dims, want):
    """C4 — the one bench shape on the bucket plan — takes the cells plan by shape, with the bucket plan's bits, passes and speculation; C1,
    C2, DS, DSC and the train step plan as before."""
    p, ntiles = steady_plan(shape, *dims)
    assert kind(p) == want, name
    if want == CELLS:
        assert (p.seg_bits, p.seg_passes, p.speculate) == (3, 2, 1)
        assert shape.s.last_seg == 0


def test_first_forward_of_c4_is_the_local_order(shape):
    set_shape(shape, *C4[:3])
    assert kind(shape.plan()) == LOCAL


@pytest.mark.parametrize("mean, want", [(256, LOCAL), (257, CELLS), (384, CELLS), (385, SEG)])
def test_holds_exactly_where_the_bucket_rule_holds(shape, mean, want):
    ntiles = set_shape(shape, *C4[:3])
    shape.plan()
    shape.count(mean * ntiles)
    assert kind(shape.plan()) == want


def parse(hip_lib, spelling):
    from das3r_amd import _lib
    names, values, sw = (C.c_char_p * 1)(b"DAS3R_BINNING"), (C.c_char_p * 1)(spelling.encode()), _lib.Switches()
    hip_lib.das3r_debug_parse_switches(names, values, 1, 0, C.byref(sw))
    return sw.binning


@pytest.mark.parametrize("tbits, onesweep, want", [(5, 1, (0, 2, 1, 3, 1)), (4, 1, (0, 2, 1, 4, 1)), (13, 1, (0, 2, 1, 3, 2)), (14, 1, (0, 2, 1, 2, 2)),
                                                   (20, 1, (0, 2, 0, 4, 3)),     # three passes, a 24-bit key: the bucket plan's stable passes
                                                   (8, 1, (1, 0, 0, 0, 1)),      # no bucket bit beside eight bits of tile id: the local order, as `bucket` falls
                                                   (15, 1, (1, 0, 0, 1, 2)),     # one bit: not enough either
                                                   (5, 0, (0, 0, 0, 0, 1))])     # the classic passes have no fast path
def test_forced_spelling(hip_lib, shape, tbits, onesweep, want):
    """DAS3R_BINNING=cells parses to 5 and forces the plan wherever the key has two bucket bits in one or two passes, whatever the history
    says: from a shape's first forward on, in the middle of a stint."""
    assert parse(hip_lib, "cells") == 5
    shape.shape(P=1000, W=64, H=64, ntiles=1 << tbits, tbits=tbits)
    shape.forced, shape.onesweep = 5, onesweep
    p = shape.plan()
    assert (p.local, p.seg, p.cells, p.seg_bits, p.seg_passes) == want
    assert not shape.count(10 ** 9)
    shape.s.radix_left = 5
    p = shape.plan()
    assert (p.local, p.seg, p.cells, p.seg_bits, p.seg_passes) == want and shape.s.radix_left == 5


@pytest.mark.parametrize("spelling, forced, want", [("bucket", 4, BUCKET), ("local", 1, LOCAL), ("radix", -1, RADIX), ("seg", 2, SEG), ("seg3", 3, SEG)])
def test_the_other_spellings_keep_their_plans_at_c4(hip_lib, shape, spelling, forced, want):
    """Forced bucket stays the fourth plan with its stable passes (the reference of tests/test_gpu_cell_sort.py)."""
    assert parse(hip_lib, spelling) == forced
    ntiles = set_shape(shape, *C4[:3])
    shape.forced = forced
    shape.plan()
    shape.count(320 * ntiles)
    assert kind(shape.plan()) == want


def test_back_off_transitions_are_the_bucket_plans(shape):
    """too_long under the plan (a single bin longer than a round of the finish, or a list the compositing kernel could not order in LDS):
    global sort for 64 forwards, no extra partition pass; the plan again afterwards; a word of an older generation is ignored; a failure
    soon after costs 128."""
    ntiles = set_shape(shape, *C4[:3])
    shape.plan()
    shape.count(320 * ntiles)
    assert kind(shape.plan()) == CELLS
    shape.count(320 * ntiles)
    gen = shape.s.gen
    p = shape.plan(too_long=gen)
    assert kind(p) == RADIX and shape.s.seg_extra == 0 and shape.s.radix_left == 63 and shape.s.backoff == 128 and shape.s.gen != gen
    shape.count(320 * ntiles)
    assert kind(shape.plan(too_long=gen)) == RADIX and shape.s.radix_left == 62, "the old generation's word names nobody"
    for _ in range(62):
        shape.count(320 * ntiles)
        assert kind(shape.plan()) == RADIX
    shape.count(320 * ntiles)
    assert kind(shape.plan()) == CELLS and shape.s.radix_left == 0
    shape.count(320 * ntiles)
    assert kind(shape.plan(too_long=shape.s.gen)) == RADIX and shape.s.radix_left == 127
    shape.forced = 5   # forced: the plan whatever the stint says
    shape.count(320 * ntiles)
    assert kind(shape.plan()) == CELLS and shape.s.radix_left == 127
