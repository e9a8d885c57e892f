"""CPU tests of the binning-path policy (das3r_amd/csrc/path_policy.h): which binning path a forward takes, when a shape backs off to
the global sort and for how long, when it takes one more partition pass, whether it speculates on its capacity, and which compositing
kernels its lists call for.  das3r_debug_path_policy_* runs the header's functions on a state struct the test owns: every test scripts
forwards (inputs, the count the device delivered, the mailbox words its kernels raised) and asserts each plan and the state it leaves.
The expected values are worked out by hand from the rules the docstrings cite, not recorded from the code."""
import ctypes as C

import pytest

LOCAL_AVG = SEG_AVG = 384          # mean list / segment length up to which the local order / the segmented path is taken
CAPACITY_MAX = 0x7FFFFF00
FRESH = dict(P=0, W=0, H=0, last_I=-1, peak_I=0, radix_left=0, backoff=64, seg_extra=0, last_seg=0, fine=0, forwards=0, clean=0, longest=0,
             resume_valid=0, resume_fine=0, resume_forwards=0)


class Shape:
    """One thread's policy state and the forwards of a script.  tbits: bits of a tile id (1 for a single tile), tile_passes = (tbits + 7) / 8."""

    def __init__(self, lib, gen=0):
        from das3r_amd import _lib
        self.lib, self._lib = lib, _lib
        self.s = _lib.PathPolicyState()
        lib.das3r_debug_path_policy_fresh(C.byref(self.s), gen)
        self.shape(P=1000, W=64, H=64, ntiles=16, tbits=4)
        self.forced, self.onesweep, self.capacity_hint, self.capacity_exact = 0, 1, 0, 0

    def shape(self, P, W, H, ntiles, tbits, tile_passes=None):
        self.P, self.W, self.H, self.ntiles, self.tbits = P, W, H, ntiles, tbits
        self.tile_passes = (tbits + 7) // 8 if tile_passes is None else tile_passes
        return self

    def state(self):
        return {n: getattr(self.s, n) for n, _ in self.s._fields_}

    def inputs(self, too_long=0, want_bits=0):
        return self._lib.PathPolicyInputs(self.P, self.W, self.H, self.ntiles, self.tbits, self.tile_passes, too_long, want_bits, self.forced,
                                          self.onesweep, self.capacity_hint, self.capacity_exact)

    def plan(self, too_long=0, want_bits=0):
        self.last_in, self.last_plan = self.inputs(too_long, want_bits), self._lib.PathPolicyPlan()
        self.lib.das3r_debug_path_policy_plan(C.byref(self.s), C.byref(self.last_in), C.byref(self.last_plan))
        return self.last_plan

    def count(self, I):
        """The count of the forward planned last arrives -> must it fall back to the global sort?"""
        return bool(self.lib.das3r_debug_path_policy_count(C.byref(self.s), C.byref(self.last_in), C.byref(self.last_plan), I))

    def forward(self, I, too_long=0, want_bits=0):
        """plan + count -> the path as tests/test_gpu_raster.py names it: "local", "seg<passes>" or "radix"."""
        p = self.plan(too_long, want_bits)
        fell_back = self.count(I)
        if p.speculate:
            assert p.local or p.seg
        else:
            assert p.cap == 0
        if p.local and not (fell_back and not p.speculate):   # (a speculative forward is enqueued before its count arrives: it keeps its path)
            return "local"
        return "seg%d" % p.seg_passes if p.seg else "radix"

    def skew(self, longest, crowd16, cap):
        return bool(self.lib.das3r_debug_path_policy_skew(C.byref(self.s), longest, crowd16, cap, self.ntiles))


@pytest.fixture
def shape(hip_lib):
    return Shape(hip_lib)


def test_fresh_state_and_seg_dbits(hip_lib, shape):
    """Verdict's defaults (api.hip's old Verdict{0, 0, 0, -1, 0, 0, 64, gen}: no count yet, no stint, the shortest back-off) and
    seg_dbits = 8 * min(passes, 3) - tbits."""
    assert shape.state() == dict(FRESH, gen=0)
    assert Shape(hip_lib, gen=77).state() == dict(FRESH, gen=77)
    for tbits, passes, want in ((1, 1, 7), (1, 2, 15), (8, 1, 0), (9, 1, -1), (16, 2, 0), (20, 3, 4), (12, 4, 12), (22, 3, 2)):
        assert hip_lib.das3r_debug_seg_dbits(tbits, passes) == want, (tbits, passes)


@pytest.mark.parametrize("extra, falls_back", [(0, False), (1, True)])
def test_first_forward_of_a_shape(shape, extra, falls_back):
    """First forward of a shape: last_I = -1 plans `local` tentatively and never speculates; a delivered count above 384 * ntiles
    turns it into the global sort, a count at or below keeps it local.  It is forward 0 of the shape: it looks at its tile lists."""
    p = shape.plan()
    assert (p.local, p.seg, p.speculate, p.cap, p.decide_fine) == (1, 0, 0, 0, 1)
    assert p.gen == 1 and shape.s.gen == 1, "meeting a shape starts a generation"
    I = LOCAL_AVG * shape.ntiles + extra
    assert shape.count(I) == falls_back
    assert shape.state() == dict(FRESH, P=1000, W=64, H=64, gen=1, last_I=I, peak_I=I, forwards=1, clean=1)   # (clean++ at planning, even when it then falls back)


def test_replay_of_the_gpu_story_on_one_tile(shape):
    """tests/test_gpu_raster.py test_segmented_binning_is_chosen_for_long_lists_and_backs_off on the host: 16 x 16 pixels (one tile: one bit
    of tile id, one partition pass, 7 bucket bits; 15 with a second pass), counts spread, spread, spread, wall, wall, spread, too_long raised
    with the current generation after each wall.  No history: local tentatively, 19 000 > 384 -> radix.  Then 19 000 >> 7 = 148 <= 384:
    the segmented path with one pass.  The first too_long finds a segmented forward without the extra pass and room for one -> one more
    pass (19 000 >> 15 = 0 <= 384: seg 2); the second finds seg_extra == 1 -> global sort for 64 forwards."""
    shape.shape(P=20011, W=16, H=16, ntiles=1, tbits=1)
    I = 19000
    took = [shape.forward(I) for _ in range(4)]             # spread, spread, spread, wall
    took.append(shape.forward(I, too_long=shape.s.gen))      # wall: the first wall's word
    assert shape.s.seg_extra == 1 and shape.s.radix_left == 0
    took.append(shape.forward(I, too_long=shape.s.gen))      # spread: the second wall's word
    assert took == ["radix", "seg1", "seg1", "seg1", "seg2", "radix"]
    assert (shape.s.radix_left, shape.s.backoff, shape.s.clean) == (63, 128, 0)
    assert shape.s.gen == 3, "the shape, the extra pass and the back-off each started a generation"


def _on_the_segmented_path(shape):
    shape.shape(P=20011, W=16, H=16, ntiles=1, tbits=1)
    assert [shape.forward(19000) for _ in range(3)] == ["radix", "seg1", "seg1"]
    return shape


@pytest.mark.parametrize("word", ["too_long", "want_bits"])
def test_a_stale_word_changes_nothing(hip_lib, shape, word):
    """too_long or want_bits carrying any generation other than the current one changes nothing.  Answering a word bumps the generation,
    so the same word delivered again by the forward already in flight is ignored (round 6: answered twice, "one more partition pass"
    turned straight into "global sort for 64 forwards")."""
    _on_the_segmented_path(shape)
    quiet = _on_the_segmented_path(Shape(hip_lib))
    gen = shape.s.gen
    for stale in (gen - 1, gen + 1, 0xFFFFFFFF, 12345):
        assert shape.forward(19000, **{word: stale}) == quiet.forward(19000) == "seg1"
        assert shape.state() == quiet.state()
    assert shape.forward(19000, **{word: gen}) == "seg2"      # answered: one more pass ...
    assert (shape.s.gen, shape.s.seg_extra, shape.s.radix_left) == (gen + 1, 1, 0)
    assert shape.forward(19000, **{word: gen}) == "seg2"      # ... and the forward in flight raises it again: names nobody now
    assert (shape.s.gen, shape.s.seg_extra, shape.s.radix_left, shape.s.backoff) == (gen + 1, 1, 0, 64)


def test_the_generation_counter_skips_zero(hip_lib):
    """0 in a mailbox word means "not raised": the counter goes from 0xFFFFFFFF to 1, at a new shape and at a decision alike."""
    sh = Shape(hip_lib, gen=0xFFFFFFFF)
    assert sh.plan().gen == 1 and sh.s.gen == 1
    sh = _on_the_segmented_path(Shape(hip_lib, gen=0xFFFFFFFE))
    assert sh.s.gen == 0xFFFFFFFF
    assert sh.forward(19000, too_long=0xFFFFFFFF) == "seg2" and sh.s.gen == 1
    sh.shape(P=5, W=16, H=16, ntiles=1, tbits=1)
    assert sh.plan().gen == 2


def _fail(shape):
    """A forward on the local order met a list too long for LDS; the next forward answers the word.  -> the stint it starts"""
    assert shape.forward(100, too_long=shape.s.gen) == "radix"
    assert shape.s.clean == 0, "clean resets on a failure"
    return shape.s.radix_left + 1   # (that forward was the stint's first)


def test_backoff_stints_double_up_to_4096(shape):
    """Successive failures give stints of 64, 128, ... up to 4096 and no further; radix_left counts down once per unforced forward, and
    the shape is back on its fast path when it reaches 0."""
    assert shape.forward(100) == "local" and shape.forward(100) == "local"
    assert _fail(shape) == 64 and shape.s.backoff == 128
    for left in range(62, -1, -1):
        assert shape.forward(100) == "radix" and shape.s.radix_left == left
    assert shape.s.clean == 0
    assert shape.forward(100) == "local" and shape.s.clean == 1
    stints = []
    for _ in range(8):
        stints.append(_fail(shape))
        shape.s.radix_left = 0    # (the stint served)
        assert shape.forward(100) == "local"
    assert stints == [128, 256, 512, 1024, 2048, 4096, 4096, 4096] and shape.s.backoff == 4096


@pytest.mark.parametrize("clean, stint", [(255, 128), (256, 64)])
def test_a_failure_after_256_clean_forwards_starts_from_64_again(shape, clean, stint):
    """A failure after at least 256 clean fast-path forwards is an occasional one and starts again from 64 (the doubling "never forgot");
    after fewer it doubles."""
    assert shape.forward(100) == "local"
    assert _fail(shape) == 64
    shape.s.radix_left = 0
    for _ in range(clean):
        assert shape.forward(100) == "local"
    assert shape.s.clean == clean
    assert _fail(shape) == stint and shape.s.backoff == 2 * stint


@pytest.mark.parametrize("forced", [1, -1, 2, 3])
def test_forced_modes_never_count_a_stint_down(shape, forced):
    """radix_left counts down only when unforced."""
    shape.forward(100)
    shape.s.radix_left = 10
    shape.forced = forced
    shape.forward(100)
    assert shape.s.radix_left == 10
    shape.forced = 0
    assert shape.forward(100) == "radix" and shape.s.radix_left == 9


def _segmented_with_a_word(shape, tbits, tile_passes, ntiles, seg_extra=0, last_seg=1):
    shape.shape(P=1000, W=64, H=64, ntiles=ntiles, tbits=tbits, tile_passes=tile_passes)
    shape.forward(600 * ntiles)        # (history: too long for the local order)
    shape.s.last_seg, shape.s.seg_extra = last_seg, seg_extra
    return shape.s.gen


def test_escalation_instead_of_backoff(hip_lib):
    """too_long is answered with one more partition pass instead of a back-off only when ALL of: the last forward was segmented,
    seg_extra == 0, tile_passes < 3, seg_dbits(tile_passes + 1) > 0.  want_bits alone never backs off."""
    def outcome(word="too_long", **kw):
        sh = Shape(hip_lib)
        gen = _segmented_with_a_word(sh, **kw)
        sh.plan(**{word: gen})
        assert sh.s.gen == gen + 1
        return sh.s.seg_extra, sh.s.radix_left, sh.s.backoff

    escalated, backed_off = (1, 0, 64), (0, 63, 128)
    assert outcome(tbits=4, tile_passes=1, ntiles=16) == escalated
    assert outcome(tbits=12, tile_passes=2, ntiles=4096) == escalated
    assert outcome(tbits=4, tile_passes=1, ntiles=16, last_seg=0) == backed_off
    assert outcome(tbits=4, tile_passes=1, ntiles=16, seg_extra=1) == (1, 63, 128)
    assert outcome(tbits=20, tile_passes=3, ntiles=1 << 20) == backed_off
    assert outcome(tbits=24, tile_passes=2, ntiles=16) == backed_off        # (8 * 3 - 24 = 0 bucket bits with one more pass)
    assert outcome("want_bits", tbits=4, tile_passes=1, ntiles=16) == escalated
    assert outcome("want_bits", tbits=20, tile_passes=3, ntiles=1 << 20) == escalated


@pytest.mark.parametrize("forced, onesweep, tbits, want", [
    (1, 1, 4, (1, 0, 1)), (-1, 1, 4, (0, 0, 1)), (2, 1, 4, (0, 1, 1)), (3, 1, 4, (0, 1, 2)),
    (2, 1, 8, (0, 0, 1)),      # no key bit free beside 8 bits of tile id in one pass
    (3, 1, 8, (0, 1, 2)),      # ... eight with a second pass
    (3, 1, 20, (0, 0, 4)),     # a fourth pass is never taken
    (0, 0, 4, (0, 0, 1)), (1, 0, 4, (0, 0, 1)), (2, 0, 4, (0, 0, 1)), (3, 0, 4, (0, 0, 2)),   # the classic radix passes have no fast path
])
def test_forced_modes(shape, forced, onesweep, tbits, want):
    """DAS3R_BINNING: local (1) forces the local order, radix (-1) the global sort, seg (2) the segmented path with the tile passes, seg3 (3)
    with one more — where the key has bucket bits free (seg_dbits > 0, at most three passes) — whatever the history and a stint say;
    without the one-sweep passes neither fast path exists.  A forced local order does not fall back on its count."""
    shape.shape(P=1000, W=64, H=64, ntiles=1 << tbits, tbits=tbits)
    shape.forced, shape.onesweep = forced, onesweep
    p = shape.plan()                  # without history ...
    assert (p.local, p.seg, p.seg_passes) == want
    assert not shape.count(10 ** 9)
    shape.s.radix_left = 5
    p = shape.plan()                  # ... and with a count far too large for either fast path, in the middle of a stint
    assert (p.local, p.seg, p.seg_passes) == want
    assert shape.s.radix_left == 5 - (1 if forced == 0 else 0)


def test_speculation(shape):
    """Speculate only with history, with capacity_hint != -1 and not DAS3R_CAPACITY=exact, and only on a fast path;
    cap = max(last_I + last_I / 4, peak_I + peak_I / 20) + 4096, clamped to 0x7FFFFF00."""
    p = shape.plan()
    assert (p.local, p.speculate, p.cap) == (1, 0, 0)        # no history
    shape.count(4000)
    p = shape.plan()
    assert (p.local, p.speculate, p.cap) == (1, 1, 4000 + 1000 + 4096)
    shape.capacity_hint = -1
    assert shape.plan().speculate == 0
    shape.capacity_hint, shape.capacity_exact = 123, 1
    assert shape.plan().speculate == 0
    shape.capacity_exact, shape.forced = 0, -1
    p = shape.plan()
    assert (p.local, p.seg, p.speculate, p.cap) == (0, 0, 0, 0)   # the global sort sizes exactly
    shape.forced = 0
    shape.s.last_I, shape.s.peak_I = 1000, 100000                 # the peak's 5 % over the last count's 25 %
    assert shape.plan().cap == 105000 + 4096
    shape.forced = 1
    shape.s.last_I = shape.s.peak_I = CAPACITY_MAX
    p = shape.plan()
    assert (p.speculate, p.cap) == (1, CAPACITY_MAX)
    shape.s.last_I = shape.s.peak_I = CAPACITY_MAX - 4096 - (CAPACITY_MAX - 4096) // 5 - 1      # just below the clamp
    assert shape.plan().cap == shape.s.last_I + shape.s.last_I // 4 + 4096 < CAPACITY_MAX


def test_the_peak_count_decays(shape):
    """peak_I decays by 1/1024 per forward and never drops below the current count."""
    peaks = []
    for I in (100000, 1000, 1000, 99900, 200000, 0):
        shape.plan()
        shape.count(I)
        assert shape.s.last_I == I
        peaks.append(shape.s.peak_I)
    assert peaks == [100000, 100000 - 97, 99903 - 97, 99900, 200000, 200000 - 195]


def test_the_compositing_choice_is_remade_every_512_forwards(hip_lib, shape):
    """decide_fine fires on forwards 0, 512, 1024, ... of a shape; a resumed `forwards` continues the schedule."""
    assert [i for i in range(1030) if shape.plan().decide_fine] == [0, 512, 1024]
    hip_lib.das3r_debug_path_policy_resume(C.byref(shape.s), 1, 510)
    shape.shape(P=7, W=64, H=64, ntiles=16, tbits=4)
    assert [i for i in range(520) if shape.plan().decide_fine] == [2, 514]


@pytest.mark.parametrize("last_I, cap, longest, crowd16, fine", [
    (2000, 9999, 4095, 0, False), (2000, 9999, 4096, 0, True),          # mean 2000: 1.8 x = 3600, but a list shorter than 4096 is never "long"
    (5000, 9999, 9000, 0, False), (5000, 9999, 9001, 0, True),          # mean 5000: longer than 5000 + 4000
    (5000, 9999, 100, 367, False), (5000, 9999, 100, 368, True),        # crowded: 23 of 64 entries in one quadrant, whatever the skew
    (-1, 4000, 7200, 0, False), (-1, 4000, 7201, 0, True),              # a shape's first forward: the mean of its capacity
    (0, 4000, 7200, 0, False), (0, 4000, 7201, 0, True),                # (an empty last forward likewise)
])
def test_the_compositing_choice(shape, last_I, cap, longest, crowd16, fine):
    """fine is set exactly when longest > mean + 4 * mean / 5 and longest >= 4096, or when crowd16 >= 368; mean = the count the shape
    learnt last (the capacity while it has none) / ntiles.  (A speculative forward measures its lists before its own count is stored, an
    exact one after: which count `mean` sees is the caller's order of calls.)"""
    shape.shape(P=1000, W=16, H=16, ntiles=1, tbits=1)
    shape.plan()
    shape.s.last_I = last_I
    shape.s.fine = 0 if fine else 1
    assert shape.skew(longest, crowd16, cap) == fine
    assert (shape.s.fine, shape.s.longest) == (int(fine), longest)


def test_the_mean_is_per_tile(shape):
    shape.shape(P=1000, W=64, H=64, ntiles=16, tbits=4)
    shape.forward(16 * 5000)
    assert not shape.skew(9000, 0, 1) and shape.skew(9001, 0, 1)


@pytest.mark.parametrize("longest, buckets", [(0, 2), (1023, 2), (1024, 3), (60 * 1024, 62), (61 * 1024, 63), (10 ** 6, 63), (0xFFFFFFFF, 63)])
def test_backward_hint(hip_lib, shape, longest, buckets):
    """das3r_raster_saved.flags of a `fine` forward: 1 | min(63, longest / BUCKET + 2) << 8, BUCKET = 1024 list positions."""
    shape.s.longest = longest
    assert hip_lib.das3r_debug_path_policy_hint(C.byref(shape.s)) == 1 | (buckets << 8)


def test_forget_and_resume(hip_lib, shape):
    """forget: the state of a thread that has met no shape, but the generation keeps counting (a word a forward of the old shape still
    has on its way names nobody).  resume: forget, and hand (fine, forwards) to the next shape only, and only once."""
    _on_the_segmented_path(shape)
    shape.skew(20000, 400, 19000)
    gen = shape.s.gen
    assert shape.s.fine == 1 and shape.s.last_seg == 1
    hip_lib.das3r_debug_path_policy_forget(C.byref(shape.s))
    assert shape.state() == dict(FRESH, gen=gen)
    p = shape.plan()                                         # the same shape again: met anew
    assert (p.local, p.speculate, p.decide_fine, p.gen) == (1, 0, 1, gen + 1)
    shape.count(19000)
    hip_lib.das3r_debug_path_policy_resume(C.byref(shape.s), 1, 700)
    assert shape.state() == dict(FRESH, gen=gen + 1, resume_valid=1, resume_fine=1, resume_forwards=700)
    hip_lib.das3r_debug_path_policy_forget(C.byref(shape.s))        # (das3r_raster_forget_shapes does not take the hand-over back)
    assert shape.s.resume_valid == 1
    p = shape.plan()
    assert (p.decide_fine, p.speculate, p.gen) == (0, 0, gen + 2)
    assert shape.state() == dict(FRESH, P=20011, W=16, H=16, gen=gen + 2, fine=1, forwards=701, clean=1, resume_valid=0, resume_fine=1, resume_forwards=700)
    shape.shape(P=8, W=16, H=16, ntiles=1, tbits=1)           # the shape after that starts from nothing
    p = shape.plan()
    assert p.decide_fine == 1 and (shape.s.fine, shape.s.forwards, shape.s.gen) == (0, 1, gen + 3)
