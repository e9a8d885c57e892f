"""Guard bands and poison round every buffer the Python layer hands the library.

`with guarded(pattern) as g:` replaces, for its duration, the allocation functions the product code calls by module attribute (torch.empty,
empty_like, zeros, zeros_like, full, full_like).  A request on a guarded device comes back as a view into a uint8 arena of
low + nbytes + high bytes: both bands hold GUARD_BYTE, the view starts at byte `low` (a multiple of 4096: at least 256-byte aligned, as the
caching allocator's own blocks are) and the high band starts at the first byte past the request — not at a rounded-up size, so a 16-byte
store over a 4-byte tail lands in it.  What `empty` / `empty_like` return holds `pattern` (recycled allocator memory is whatever was there:
a kernel that reads a word before writing it sees the pattern); `zeros` / `full` hold what was asked for.  Every arena stays alive in the
registry, with the call site that asked for it, until the context exits — also one the library replaced (the forward's binning buffer when
a speculative forward is redone) — and `g.assert_intact()` checks the bands of all of them.

Not guarded (they go to the original function unchanged): other devices, `out=`, `pin_memory`, zero elements, layouts other than strided,
and a request whose result would not be contiguous (channels_last, `*_like` of a permuted tensor).

A helper module: tests import it explicitly.  It is no conftest and no plugin, and nothing is replaced outside a `with` block.
"""
import contextlib
import os
import sys

import torch

GUARD_BYTE = 0xA7                       # neither 0x00 nor 0xFF; 0xA7A7A7A7 is a negative int32, a huge uint32 and a negative, tiny float
PATTERNS = (0x00, 0xFF, 0x7FA51C3D)     # nothing a kernel zeroes itself is hidden / the worst case of counters, cursors and indices / a NaN
NAMES = ("empty", "empty_like", "zeros", "zeros_like", "full", "full_like")
_HERE = os.path.abspath(__file__)
_ORIG = {n: getattr(torch, n) for n in NAMES}   # (taken at import: guarded() must not be entered twice at once)


def pattern_bytes(pattern, n):
    """-> the n bytes a payload of n bytes is filled with: a value up to 0xFF is a byte, a larger one a little-endian 32-bit word, repeated"""
    pattern = int(pattern)
    unit = bytes([pattern]) if 0 <= pattern <= 0xFF else pattern.to_bytes(4, "little")
    return (unit * (n // len(unit) + 1))[:n]


class Arena:
    __slots__ = ("buf", "low", "nbytes", "high", "site", "name")

    def __init__(self, buf, low, nbytes, high, site, name):
        self.buf, self.low, self.nbytes, self.high, self.site, self.name = buf, low, nbytes, high, site, name

    def bands(self):
        return (("low", self.buf[:self.low]), ("high", self.buf[self.low + self.nbytes:]))

    def payload(self):
        """the bytes between the bands, as the uint8 tensor they are"""
        return self.buf[self.low:self.low + self.nbytes]

    @property
    def data_ptr(self):
        return self.buf.data_ptr() + self.low

    def __repr__(self):
        return f"<{self.name} of {self.nbytes} bytes at {self.site}>"


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return f"{f.f_code.co_filename}:{f.f_lineno} ({f.f_code.co_name})"


class Guard:
    def __init__(self, pattern, devices, low, high):
        if low % 4096 or low <= 0 or high <= 0:
            raise ValueError("low must be a positive multiple of 4096, high positive")
        self.pattern, self.low, self.high = int(pattern), int(low), int(high)
        self.types = {torch.device(d).type for d in devices}
        self.arenas = []

    # ---- allocation

    def _wanted(self, name, args, kwargs):
        """-> the device to guard the request on, or None: pass it through"""
        if kwargs.get("out") is not None or kwargs.get("pin_memory") or kwargs.get("layout", torch.strided) is not torch.strided:
            return None
        dev = kwargs.get("device")
        if dev is None:
            if name.endswith("_like"):
                if not (args and torch.is_tensor(args[0])) or args[0].layout is not torch.strided:
                    return None
                dev = args[0].device
            else:
                dev = torch.get_default_device() if hasattr(torch, "get_default_device") else _ORIG["empty"](0).device
        dev = torch.device(dev)
        return dev if dev.type in self.types else None

    def alloc(self, name, args, kwargs):
        orig = _ORIG[name]
        dev = self._wanted(name, args, kwargs)
        if dev is None:
            return orig(*args, **kwargs)
        proto = orig(*args, **{**kwargs, "device": "meta"})   # the original's own reading of sizes, dtype and format; no memory
        if proto.numel() == 0 or not proto.is_contiguous():
            return orig(*args, **kwargs)
        nbytes = proto.numel() * proto.element_size()
        total = self.low + nbytes + self.high
        raw = _ORIG["empty"](total + 255, dtype=torch.uint8, device=dev)   # (the host allocator aligns to 64 bytes only: the arena starts at
        skew = -raw.data_ptr() % 256                                       #  the first 256-byte boundary of what it gave)
        buf = raw[skew:skew + total]
        buf[:self.low] = GUARD_BYTE
        buf[self.low + nbytes:] = GUARD_BYTE
        payload = buf[self.low:self.low + nbytes]
        out = payload.view(proto.dtype).view(proto.shape)
        if name.startswith("empty"):
            self._poison(payload)
        elif name.startswith("zeros"):
            payload.zero_()
        else:
            out.fill_(args[1] if len(args) > 1 else kwargs["fill_value"])
        self.arenas.append(Arena(buf, self.low, nbytes, self.high, _call_site(), "torch." + name))
        return out.requires_grad_(True) if proto.requires_grad else out

    def _poison(self, payload):
        n = payload.numel()
        if 0 <= self.pattern <= 0xFF:
            payload.fill_(self.pattern)
            return
        word = self.pattern - (1 << 32) if self.pattern >= 1 << 31 else self.pattern
        if n >= 4:
            payload[:n // 4 * 4].view(torch.int32).fill_(word)
        for k, b in enumerate(pattern_bytes(self.pattern, n)[n // 4 * 4:]):
            payload[n // 4 * 4 + k] = b

    # ---- inspection

    def from_site(self, text):
        """the arenas whose call site contains `text`, in the order they were asked for"""
        return [a for a in self.arenas if text in a.site]

    def damage(self):
        """-> [(arena, side, offset of the first changed byte, changed bytes)]; the offset counts from the payload's first byte on the low
        side (-1: the byte before it) and from the first byte past the payload on the high side (0: that byte)"""
        if any(a.buf.is_cuda for a in self.arenas):
            torch.cuda.synchronize()
        found = []
        bands = [(a, side, band) for a in self.arenas for side, band in a.bands()]
        counts = [(band != GUARD_BYTE).count_nonzero() for _a, _side, band in bands]   # (launched first, read afterwards)
        for (a, side, band), n in zip(bands, counts):
            n = int(n)
            if n:
                at = int((band != GUARD_BYTE).nonzero()[0])
                found.append((a, side, at - a.low if side == "low" else at, n))
        return found

    def assert_intact(self):
        found = self.damage()
        if found:
            lines = [f"{a.name} of {a.nbytes} bytes asked for at {a.site}: {side} band, first changed byte at offset {off}, {n} bytes changed"
                     for a, side, off, n in found]
            raise AssertionError("a store outside the buffer it was given (pattern 0x%X):\n  " % self.pattern + "\n  ".join(lines))


def _stand_in(guard, name):
    def fn(*args, **kwargs):
        return guard.alloc(name, args, kwargs)
    fn.__name__ = fn.__qualname__ = name
    fn.__wrapped__ = _ORIG[name]
    return fn


@contextlib.contextmanager
def guarded(pattern, devices=("cuda",), low=4096, high=65536):
    """-> a Guard; see the module docstring.  The originals are back on exit, also when the body raises."""
    for n in NAMES:
        if getattr(torch, n) is not _ORIG[n]:
            raise RuntimeError("guarded() is already active (or torch.%s was replaced by someone else)" % n)
    g = Guard(pattern, devices, low, high)
    try:
        for n in NAMES:
            setattr(torch, n, _stand_in(g, n))
        yield g
    finally:
        for n in NAMES:
            setattr(torch, n, _ORIG[n])
        g.arenas = []


# ---- the four runs of a guarded case: once as the product allocates, once under every pattern


def leaves(x, path=""):
    """(path, tensor / array / scalar) of every leaf of a nest of dicts, lists and tuples; None leaves included"""
    if isinstance(x, dict):
        for k in x:
            yield from leaves(x[k], f"{path}.{k}" if path else str(k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from leaves(v, f"{path}[{i}]")
    else:
        yield path, x


def _bytes_of(v):
    import numpy as np
    if isinstance(v, np.ndarray):
        v = torch.from_numpy(np.ascontiguousarray(v))
    v = v.detach().contiguous().cpu()
    return v.reshape(-1).view(torch.uint8) if v.numel() else v.reshape(-1)


def assert_same_bits(got, want, what):
    """Every leaf of two nests: the same type, shape, dtype and BYTES (a NaN equals itself, -0.0 is not +0.0)."""
    import numpy as np
    a, b = list(leaves(got)), list(leaves(want))
    assert [p for p, _ in a] == [p for p, _ in b], f"{what}: the results have different entries"
    for (path, x), (_p, y) in zip(a, b):
        if torch.is_tensor(x) or isinstance(x, np.ndarray):
            assert type(x) is type(y) and tuple(x.shape) == tuple(y.shape) and x.dtype == y.dtype, f"{what}: {path} changed its shape or type"
            bx, by = _bytes_of(x), _bytes_of(y)
            assert torch.equal(bx, by), (f"{what}: {path} differs in {int((bx != by).sum())} of {bx.numel()} bytes, the first at byte "
                                         f"{int((bx != by).nonzero()[0])}: a read of memory the library never wrote")
        else:
            assert x == y, f"{what}: {path} is {x!r}, not {y!r}"


def four_runs(op, what, compare=assert_same_bits, inspect=None, devices=("cuda",)):
    """op(guard or None) -> a nest of results.  Runs it once unguarded and once under guarded(pattern) for every pattern, asserts the bands
    intact each time and `compare(guarded result, unguarded result, label)`.  inspect(guard, result): further looks at the registry while it
    is alive.  -> the unguarded result."""
    base = op(None)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for pattern in PATTERNS:
        with guarded(pattern, devices=devices) as g:
            got = op(g)
            g.assert_intact()
            assert g.arenas, f"{what}: nothing the operation allocates went through the guarded functions"
            if inspect is not None:
                inspect(g, got)
        compare(got, base, f"{what}, buffers poisoned with 0x{pattern:X}")
    return base
