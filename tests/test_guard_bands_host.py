"""tests/guard_bands.py on the CPU: the checker can fail, and what the stand-ins return is what the originals return.

The out-of-bounds writes here are plain tensor writes by the test into its own arena (through the arena the registry keeps), no kernels."""
import pytest
import torch

from tests import guard_bands
from tests.guard_bands import GUARD_BYTE, NAMES, PATTERNS, assert_same_bits, four_runs, guarded, pattern_bytes

ORIGINALS = {n: getattr(torch, n) for n in NAMES}
CPU = dict(devices=("cpu",))


def _calls():
    """(name, call on the torch module as it is now) of every replaced function, in several spellings"""
    like = ORIGINALS["empty"](5, 7, dtype=torch.float64)
    return [("empty", lambda: torch.empty(3, 5)), ("empty", lambda: torch.empty((3, 5), dtype=torch.int32)),
            ("empty", lambda: torch.empty(torch.Size([2, 3, 4]), dtype=torch.uint8, device="cpu")),
            ("empty", lambda: torch.empty(7, dtype=torch.float16, requires_grad=True)), ("empty", lambda: torch.empty(1, dtype=torch.bool)),
            ("empty_like", lambda: torch.empty_like(like)), ("empty_like", lambda: torch.empty_like(like, dtype=torch.int16)),
            ("zeros", lambda: torch.zeros(4, 4)), ("zeros", lambda: torch.zeros((9,), dtype=torch.int64)),
            ("zeros", lambda: torch.zeros(2, 2, requires_grad=True)), ("zeros_like", lambda: torch.zeros_like(like)),
            ("full", lambda: torch.full((3, 3), 1.5)), ("full", lambda: torch.full((5,), 7)), ("full", lambda: torch.full((2,), True)),
            ("full", lambda: torch.full((3,), 2.0, dtype=torch.float64, requires_grad=True)),
            ("full_like", lambda: torch.full_like(like, -3.25)), ("full_like", lambda: torch.full_like(like, 4, dtype=torch.int32))]


def test_the_guard_byte_and_the_patterns():
    assert GUARD_BYTE not in (0x00, 0xFF) and PATTERNS == (0x00, 0xFF, 0x7FA51C3D)
    assert pattern_bytes(0xFF, 3) == b"\xff\xff\xff" and pattern_bytes(0x7FA51C3D, 6) == b"\x3d\x1c\xa5\x7f\x3d\x1c"
    word = torch.frombuffer(bytearray(pattern_bytes(0x7FA51C3D, 4)), dtype=torch.float32)
    assert torch.isnan(word).all(), "the word pattern is a NaN as a float"


def test_what_the_stand_ins_return_is_what_the_originals_return():
    plain = [(name, call()) for name, call in _calls()]
    with guarded(0xFF, **CPU) as g:
        stood = [(name, call()) for name, call in _calls()]
        assert len(g.arenas) == len(stood), "every one of these requests was guarded"
        g.assert_intact()
        for (name, a), (_n, b), arena in zip(plain, stood, g.arenas):
            assert (b.shape, b.dtype, b.device, b.stride(), b.requires_grad, b.is_contiguous(), b.is_leaf) == \
                   (a.shape, a.dtype, a.device, a.stride(), a.requires_grad, a.is_contiguous(), a.is_leaf), name
            assert b.data_ptr() % 256 == 0 and b.data_ptr() == arena.data_ptr, "the payload starts at byte `low`, 256-byte aligned"
            assert arena.nbytes == a.numel() * a.element_size() and arena.buf.numel() == 4096 + arena.nbytes + 65536
            assert "test_guard_bands_host.py:" in arena.site and "<lambda>" in arena.site
            raw = arena.buf[arena.low:arena.low + arena.nbytes]
            if name.startswith(("zeros", "full")):   # exact payloads, compared as bytes
                assert torch.equal(raw, a.detach().contiguous().view(-1).view(torch.uint8)), name
            else:
                assert (raw == 0xFF).all(), name


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nbytes", [1, 3, 4, 6, 17, 4096])
def test_empty_holds_the_pattern_up_to_its_last_byte(pattern, nbytes):
    with guarded(pattern, **CPU) as g:
        t = torch.empty(nbytes, dtype=torch.uint8)
        assert bytes(t.tolist()) == pattern_bytes(pattern, nbytes)
        assert (g.arenas[0].buf[:4096] == GUARD_BYTE).all() and (g.arenas[0].buf[4096 + nbytes:] == GUARD_BYTE).all()
        assert g.arenas[0].buf[4096 + nbytes:].numel() == 65536
        g.assert_intact()


def test_writes_inside_the_payload_leave_it_intact():
    with guarded(0x7FA51C3D, **CPU) as g:
        t = torch.empty(33, 3)
        t.fill_(1.0)
        t[0, 0], t[-1, -1] = 2.0, 3.0
        u = torch.zeros(5, dtype=torch.uint8)
        u += 9
        g.assert_intact()
        assert g.damage() == []


@pytest.mark.parametrize("side", ["low", "high"])
def test_one_byte_outside_is_reported_with_side_offset_and_call_site(side):
    with guarded(0x00, **CPU) as g:
        torch.empty(10, dtype=torch.float32)
        t = torch.empty(7, dtype=torch.uint8); line = _line()   # noqa: E702 - the request and its line number, on one line
        torch.zeros(3)
        arena = g.arenas[1]
        assert arena.data_ptr == t.data_ptr()
        at = arena.low + arena.nbytes if side == "high" else arena.low - 1   # payload[-1] + 1, payload[0] - 1
        arena.buf[at] = 0
        (hit,) = g.damage()
        assert hit[0] is arena and hit[1:] == (side, 0 if side == "high" else -1, 1)
        with pytest.raises(AssertionError) as e:
            g.assert_intact()
        msg = str(e.value)
        assert f"test_guard_bands_host.py:{line} " in msg and f"{side} band" in msg and "of 7 bytes" in msg
        assert f"offset {0 if side == 'high' else -1}," in msg and "1 bytes changed" in msg and msg.count(" band,") == 1


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_a_long_overrun_reports_its_first_byte_and_its_length():
    with guarded(0xFF, **CPU) as g:
        torch.full((4,), 1.0)
        a = g.arenas[0]
        a.buf[a.low + a.nbytes + 12:a.low + a.nbytes + 28] = 0x11
        a.buf[5] = GUARD_BYTE   # a store of the guard byte itself is invisible: the reason it is no common value
        assert g.damage() == [(a, "high", 12, 16)]


def test_a_superseded_allocation_is_still_checked():
    with guarded(0xFF, **CPU) as g:
        holder = {"buf": torch.empty(64, dtype=torch.uint8)}
        first = g.arenas[0]
        first.buf[first.low + 64] = 1          # the overrun of the first attempt ...
        holder["buf"] = torch.empty(128, dtype=torch.uint8)   # ... whose buffer the caller then replaces and drops
        assert len(g.arenas) == 2 and g.arenas[0] is first and first.buf.data_ptr() != g.arenas[1].buf.data_ptr()
        with pytest.raises(AssertionError, match="of 64 bytes"):
            g.assert_intact()


def test_the_originals_are_back_after_a_normal_exit_and_after_an_exception():
    with guarded(0x00, **CPU):
        assert all(getattr(torch, n) is not ORIGINALS[n] for n in NAMES)
    assert all(getattr(torch, n) is ORIGINALS[n] for n in NAMES)
    with pytest.raises(ZeroDivisionError):
        with guarded(0x00, **CPU):
            torch.empty(3)
            1 / 0
    assert all(getattr(torch, n) is ORIGINALS[n] for n in NAMES)
    with guarded(0x00, **CPU):
        with pytest.raises(RuntimeError, match="already active"):
            with guarded(0xFF, **CPU):
                pass
    assert all(getattr(torch, n) is ORIGINALS[n] for n in NAMES)


def test_what_is_not_guarded_passes_through():
    with guarded(0xFF) as g:   # only "cuda" is guarded
        t = torch.empty(5)
        z = torch.zeros(5, device="cpu")
        assert g.arenas == [] and t._base is None and z._base is None and not z.any()
    like = torch.empty(4, 6).t()
    with guarded(0xFF, **CPU) as g:
        out = torch.empty(3)
        assert torch.zeros(3, out=out) is out and len(g.arenas) == 1
        assert torch.empty(0).numel() == 0 and torch.empty(3, 0, 2).shape == (3, 0, 2) and torch.zeros_like(torch.empty(0)).numel() == 0
        assert torch.empty_like(like).stride() == like.stride(), "a permuted tensor's like keeps the original's strides: not guarded"
        assert torch.empty(2, 3, 4, 5, memory_format=torch.channels_last).is_contiguous(memory_format=torch.channels_last)
        assert torch.empty(4, device="meta").device.type == "meta"
        assert len(g.arenas) == 1   # `out` alone
        g.assert_intact()


def test_bad_band_sizes_are_refused():
    for kw in (dict(low=100), dict(low=0), dict(high=0)):
        with pytest.raises(ValueError):
            with guarded(0, **CPU, **kw):
                pass
    assert all(getattr(torch, n) is ORIGINALS[n] for n in NAMES) and guard_bands._ORIG == ORIGINALS


# ---- the four runs and the comparison


def test_same_bits_is_a_comparison_of_bytes():
    nan = torch.tensor([float("nan"), 1.0])
    assert_same_bits(dict(a=[nan, None], n=3), dict(a=[nan.clone(), None], n=3), "a NaN equals itself")
    assert_same_bits(torch.empty(0, 3), torch.empty(0, 3), "no element")
    for got, want, why in ((torch.tensor([0.0]), torch.tensor([-0.0]), "differs in 1 of 4 bytes"), (torch.zeros(2), torch.zeros(2, dtype=torch.int32), "shape or type"),
                           (torch.zeros(2), torch.zeros(1, 2), "shape or type"), (dict(a=1), dict(b=1), "different entries"), (dict(a=1), dict(a=2), "is 1, not 2"),
                           ([torch.zeros(3)], [None], "shape or type")):
        with pytest.raises(AssertionError, match=why):
            assert_same_bits(got, want, "x")


def test_four_runs_pass_what_is_written_in_full_and_see_what_is_not():
    seen = []

    def written(guard):
        seen.append(guard)
        out = torch.empty(5, 3)
        out.copy_(torch.arange(15.0).reshape(5, 3))
        return dict(out=out)

    base = four_runs(written, "written in full", devices=("cpu",))
    assert seen[0] is None and [g.pattern for g in seen[1:]] == list(PATTERNS) and torch.equal(base["out"], torch.arange(15.0).reshape(5, 3))

    def one_word_short(guard):   # the last word is read as the allocator left it: under a guard, as the pattern
        out = torch.zeros(4) if guard is None else torch.empty(4)
        out[:3] = 0.0
        return out

    with pytest.raises(AssertionError, match="differs in 4 of 16 bytes, the first at byte 12: a read of memory the library never wrote"):
        four_runs(one_word_short, "one word short", devices=("cpu",))

    def one_byte_over(guard):
        out = torch.zeros(4)
        if guard is not None:
            a = guard.arenas[-1]
            a.buf[a.low + a.nbytes] = 0
        return out

    with pytest.raises(AssertionError, match=r"torch.zeros of 16 bytes asked for at .*test_guard_bands_host.py:\d+ \(one_byte_over\): high band"):
        four_runs(one_byte_over, "one byte over", devices=("cpu",))
    with pytest.raises(AssertionError, match="nothing the operation allocates"):
        four_runs(lambda guard: torch.ones(2), "unguarded", devices=("cpu",))


def test_the_slack_behind_the_binning_arrays_shows_a_store_past_the_capacity(hip_lib):
    """tests/test_gpu_guard_bands.py check_slack on a buffer made here: the layout of 1200 Gaussians, 5971 instances on 128 x 64 (host
    arithmetic of the library); entry `capacity` of the first array — what an emission without its clamp would write — is seen, entry
    capacity - 1 and the next array's first entry are not."""
    from das3r_amd import _lib
    from tests.test_gpu_guard_bands import check_slack
    P, cap, W, H = 1200, 5971, 128, 64
    nbytes = _lib.layout(P, cap, W, H)["binning_bytes"]
    stride = (4 * cap + 255) // 256 * 256
    for pattern in PATTERNS:
        with guarded(pattern, **CPU) as g:
            buf = torch.empty(nbytes, dtype=torch.uint8)
            arena = g.arenas[0]
            words = buf[:4 * stride].view(torch.int32)
            words[cap - 1] = 7
            words[stride // 4] = 7
            check_slack(arena, P, cap, W, H, pattern, "in bounds")
            words[cap] = 7
            with pytest.raises(AssertionError, match=f"array 0 of the binning buffer .* was written past entry {cap}"):
                check_slack(arena, P, cap, W, H, pattern, "one entry over")
            g.assert_intact()   # (the bands cannot see it: the store stayed inside the buffer)
    with guarded(0xFF, **CPU) as g:
        torch.empty(_lib.layout(P, 6016, W, H)["binning_bytes"], dtype=torch.uint8)
        with pytest.raises(AssertionError, match="leaves no slack"):
            check_slack(g.arenas[0], P, 6016, W, H, 0xFF, "a multiple of 64 instances")
