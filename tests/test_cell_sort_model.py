"""A numpy model of the cells plan (das3r_amd/csrc/cell_sort.hip) and of the tie rule that makes it exact (render_common.h
local_order_tile), against a stable sort of the instances by (tile, bucket, depth bits, Gaussian id).

  A  partition by the top eight partition bits: every workgroup takes a chunk of the emitted triples and reserves, per non-empty bin, a
     run on that bin's cursor.  The model hands the reservations out in a RANDOM interleaving of the workgroups — whatever order the
     atomics land in on the device.
  B  finish per cell: the cell's 256-bin histogram over the low eight partition bits, every entry at its bin's offset plus its place
     inside the bin.  The model fills the bins in an ARBITRARY order (a random permutation of the cell's run), several parts per cell and
     rounds of a few entries, and writes the ranges of the cell's non-empty tiles.
  finish  the compositing kernel ranks a tile's list by (bucket | fraction) and breaks ties by (depth bits, Gaussian id).

Key = tile << (dbits + 16) | bucket << 16 | fraction, bucket and fraction being the top bits of one monotone map of the depth bits, as
segkey.h makes them."""
import numpy as np
import pytest

FBITS = 16


def make_instances(rng, ntiles, tbits, passes, n, depth_values=None, empty_tiles=()):
    """-> (key, gid, depth bits) in emission order: index order, a Gaussian's instances contiguous, at most one per tile."""
    dbits = 8 * passes - tbits
    P = max(1, n // 3)
    depth = (rng.random(P).astype(np.float32) * 9.0 + 1.0) if depth_values is None else rng.choice(np.asarray(depth_values, np.float32), P)
    dkey = depth.view(np.uint32).astype(np.uint64)
    lo, hi = np.float32(1.0).view(np.uint32), np.float32(10.0).view(np.uint32)
    mapped = (dkey - np.uint64(lo)) * np.uint64((1 << (dbits + FBITS)) - 1) // np.uint64(int(hi) - int(lo))   # monotone in the depth bits, ties kept
    allowed = np.setdiff1d(np.arange(ntiles), np.asarray(empty_tiles, dtype=np.int64))
    keys, gids = [], []
    for g in range(P):
        for t in np.sort(rng.choice(allowed, size=min(len(allowed), int(rng.integers(0, 7))), replace=False)):
            keys.append((int(t) << (dbits + FBITS)) | int(mapped[g]))
            gids.append(g)
    return np.asarray(keys, np.uint64), np.asarray(gids, np.int64), dkey, dbits


def partition_a(rng, key, gid, slot, shift, chunk):
    """cell_partition_kernel: bases from the global histogram, one reservation per (workgroup, non-empty bin), in a random interleaving."""
    n = len(key)
    digit = (key >> np.uint64(shift)) & np.uint64(255)
    ghist = np.bincount(digit.astype(np.int64), minlength=256)
    base = np.concatenate([[0], np.cumsum(ghist)[:-1]])
    cursor = np.zeros(256, np.int64)
    out = [np.zeros(n, a.dtype) for a in (key, gid, slot)]
    filled = np.zeros(n, bool)
    wgs = [(b, d) for b in range(0, n, chunk) for d in np.unique(digit[b:b + chunk])]
    for i in rng.permutation(len(wgs)):   # the order the returning atomics are served in
        b, d = wgs[i]
        idx = b + np.flatnonzero(digit[b:b + chunk] == d)   # the workgroup's run of the digit, in its staged (stable) order
        at = base[int(d)] + cursor[int(d)]
        cursor[int(d)] += len(idx)
        dst = at + np.arange(len(idx))
        assert not filled[dst].any()
        filled[dst] = True
        for o, a in zip(out, (key, gid, slot)):
            o[dst] = a[idx]
    assert filled.all() and (cursor == ghist).all(), "the self-check of cell_finish_kernel's first workgroup"
    return out, ghist


def finish_b(rng, key, gid, slot, cell_sizes, kshift, dbits, ntiles, split, round_entries):
    """cell_finish_kernel: per cell the full histogram of the low digit, parts of 256 / split bins, rounds of contiguous bins, arbitrary
    order inside a bin; ranges of the non-empty tiles.  cell_sizes None: one cell (eight partition bits)."""
    n = len(key)
    out = [np.zeros(n, a.dtype) for a in (key, gid, slot)]
    ranges = np.zeros((ntiles, 2), np.int64)
    sizes = [n] if cell_sizes is None else list(cell_sizes)
    base = 0
    for cell, cnt in enumerate(sizes):
        if cnt:
            k = key[base:base + cnt]
            bins = ((k >> np.uint64(kshift)) & np.uint64(255)).astype(np.int64)
            off = np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=256))])
            for t in range(1 << (8 - dbits)):
                tile, lo, hi = (cell << (8 - dbits)) + t, off[t << dbits], off[(t + 1) << dbits]
                if hi > lo and tile < ntiles:
                    ranges[tile] = (base + lo, base + hi)
            for part in range(split):
                r0, end = part * (256 // split), (part + 1) * (256 // split)
                while r0 < end:
                    r1 = r0
                    while r1 < end and off[r1 + 1] - off[r0] <= round_entries:
                        r1 += 1
                    r1 = max(r1, r0 + 1)   # a bin longer than a round: scattered directly
                    arrive = rng.permutation(cnt)   # the order the LDS atomics are served in
                    arrive = arrive[(bins[arrive] >= r0) & (bins[arrive] < r1)]
                    arrive = arrive[np.argsort(bins[arrive], kind="stable")]   # place = bin's offset + entries of the bin served before
                    dst = base + off[r0] + np.arange(len(arrive))
                    assert len(arrive) == off[r1] - off[r0]
                    for o, a in zip(out, (key, gid, slot)):
                        o[dst] = a[base + arrive]
                    r0 = r1
        base += cnt
    return out, ranges


def local_finish(key, gid, slot, ranges, dkey, dbits):
    """local_order_tile with the id tie rule: (bucket | fraction), then (depth bits, Gaussian id)."""
    gid, slot = gid.copy(), slot.copy()
    mask = np.uint64((1 << (dbits + FBITS)) - 1)
    for a, b in ranges:
        if b > a:
            order = np.lexsort((gid[a:b], dkey[gid[a:b]], key[a:b] & mask))
            gid[a:b], slot[a:b] = gid[a:b][order], slot[a:b][order]
    return gid, slot


def reference(key, gid, dkey, dbits, ntiles):
    """Stable sort by (tile, bucket, depth bits, id), and the tile ranges of the result."""
    tile = (key >> np.uint64(dbits + FBITS)).astype(np.int64)
    bucket = ((key >> np.uint64(FBITS)) & np.uint64((1 << dbits) - 1)).astype(np.int64)
    order = np.lexsort((gid, dkey[gid], bucket, tile))
    counts = np.bincount(tile, minlength=ntiles)
    ends = np.cumsum(counts)
    ranges = np.stack([ends - counts, ends], 1)
    ranges[counts == 0] = 0
    return gid[order], order, ranges


CASES = {
    # name: (ntiles, tbits, passes, instances, depth values, empty tiles, chunk, split, round)
    "two_passes":          (300, 9, 2, 6000, None, (), 512, 4, 64),
    "ties":                (300, 9, 2, 6000, (2.0, 3.5, 3.5000002, 7.0), (), 512, 4, 64),
    "empty_tiles_cells":   (1040, 11, 2, 4000, None, tuple(range(100, 900)), 256, 4, 32),
    "not_a_multiple_of_32": (8160 // 16 + 7, 10, 2, 5000, (1.5, 4.0, 9.0), (3, 4, 5), 1024, 2, 48),
    "one_cell_24_tiles":   (24, 5, 1, 3000, None, (7,), 4096, 4, 100),
    "one_cell_33_tiles":   (33, 6, 1, 3000, (2.0, 2.0000002, 6.0), (), 4096, 8, 16),
    "bin_longer_than_a_round": (40, 6, 1, 2500, (5.0,), (), 4096, 4, 8),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cells_plan_equals_the_stable_sort(name):
    ntiles, tbits, passes, n, depths, empty, chunk, split, rnd = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    key, gid, dkey, dbits = make_instances(rng, ntiles, tbits, passes, n, depths, empty)
    slot = np.arange(len(key), dtype=np.int64)
    want_gid, want_slot, want_ranges = reference(key, gid, dkey, dbits, ntiles)
    results = []
    for _ in range(2):   # two runs: another interleaving, another order inside the bins — the same lists
        k, g, s, sizes = key, gid, slot, None
        if passes == 2:
            (k, g, s), sizes = partition_a(rng, key, gid, slot, FBITS + 8, chunk)
        (k, g, s), ranges = finish_b(rng, k, g, s, sizes, FBITS, dbits, ntiles, split, rnd)
        assert np.array_equal(ranges, want_ranges)
        assert np.array_equal(k >> np.uint64(FBITS), np.sort(key >> np.uint64(FBITS))), "ordered by (tile, bucket)"
        assert np.array_equal(gid[s], g), "the slot travels with its id"
        got_gid, got_slot = local_finish(k, g, s, ranges, dkey, dbits)
        assert np.array_equal(got_gid, want_gid) and np.array_equal(got_slot, want_slot)
        results.append((got_gid, got_slot))
    assert all(np.array_equal(a, b) for a, b in zip(*results))


def test_position_ties_would_not_be_exact():
    """Why the tie rule changed: ranked by (depth bits, POSITION), an arbitrary arrival order inside a segment shows in the lists."""
    rng = np.random.default_rng(5)
    key, gid, dkey, dbits = make_instances(rng, 24, 5, 1, 3000, (4.0,), ())
    slot = np.arange(len(key), dtype=np.int64)
    want_gid, _, _ = reference(key, gid, dkey, dbits, 24)
    (k, g, s), ranges = finish_b(rng, key, gid, slot, None, FBITS, dbits, 24, 4, 64)
    by_position = g.copy()
    mask = np.uint64((1 << (dbits + FBITS)) - 1)
    for a, b in ranges:
        order = np.lexsort((np.arange(b - a), dkey[g[a:b]], k[a:b] & mask))
        by_position[a:b] = g[a:b][order]
    assert not np.array_equal(by_position, want_gid)
    assert np.array_equal(local_finish(k, g, s, ranges, dkey, dbits)[0], want_gid)
