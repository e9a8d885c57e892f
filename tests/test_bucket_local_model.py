"""CPU model of the bucket-ordered local finish (das3r_amd/csrc/render_common.h local_order_tile, the 257 - 512 branch of a forward whose
lists arrive ordered by depth bucket: csrc/path_policy.h bucket_local_rule), beside tests/test_segkey_model.py.

A tile's entries arrive in stable (bucket, index) order — what the partition passes leave — with the bucket and sixteen fraction bits of
segkey.h's monotone depth map in the low bits of their key words (dbits = 3, fbits = 16).  The finish, restated in numpy step by step:

  * word of an entry = (bucket << 16 | fraction) << 9 | position in the arrival order;
  * the bounds of a (tile, bucket) segment are the places where the bucket changes;
  * rank = segment start rounded down to four + the number of words below its own among the words from there on, eight at a time, to
    past the segment's end (the words behind a segment, and the padding behind the list, are below nobody of the segment);
  * TIE GROUPS — neighbours by rank that share bucket and fraction — fetch their depth bits and are ranked again inside the group by
    (depth bits, position), as segsort.hip resolves them; everybody else keeps the rank.

The result must be the exact (depth bits, index) order — the global sort's — for every depth distribution below and for n = 257, 320, 511
and 512."""
import numpy as np
import pytest

from tests.test_segkey_model import _bits, bucket_map

DBITS, FBITS, POS = 3, 16, 9


def arrival(bits, gid, f):
    """Stable partition by bucket of entries emitted in index order -> (gid, depth bits, key low bits) in arrival order."""
    v = f(bits).astype(np.uint32)                       # bucket << 16 | fraction
    order = np.argsort(v >> FBITS, kind="stable")       # (gid ascending on the way in: index order inside a bucket)
    return gid[order], bits[order], v[order]


def finish(key, depth_bits):
    """-> (destination rank of every arrival position, whether the tile had a tie group)."""
    n = key.shape[0]
    assert 256 < n <= 512
    word = np.full(520, 0xFFFFFFFF, dtype=np.uint64)
    word[:n] = (key.astype(np.uint64) << POS) | np.arange(n, dtype=np.uint64)
    bucket = (word[:n] >> (FBITS + POS)).astype(np.int64)
    lo, hi = np.zeros(1 << DBITS, dtype=np.int64), np.zeros(1 << DBITS, dtype=np.int64)
    for i in range(n):   # (the kernel: one thread per position, looking at its neighbour in front)
        if i == 0 or bucket[i - 1] != bucket[i]:
            lo[bucket[i]] = i
            if i:
                hi[bucket[i - 1]] = i
        if i == n - 1:
            hi[bucket[i]] = n
    rank = np.empty(n, dtype=np.int64)
    for i in range(n):
        a, b = lo[bucket[i]] & ~3, hi[bucket[i]]
        b8 = a + ((b - a + 7) // 8) * 8
        assert b8 <= 520
        rank[i] = a + int((word[a:b8] < word[i]).sum())
    assert sorted(rank.tolist()) == list(range(n)), "the ranks are a permutation"
    byrank = np.empty(n, dtype=np.uint64)
    byrank[rank] = word[:n]
    f = byrank >> POS                                   # bucket | fraction, by rank
    same = f[1:] == f[:-1]
    tied = np.zeros(n, dtype=bool)                      # by rank: a neighbour shares bucket and fraction
    tied[1:] |= same
    tied[:-1] |= same
    depth = np.zeros(n, dtype=np.uint64)                # by rank; fetched for the tied entries only
    final = rank.copy()
    for i in range(n):
        if tied[rank[i]]:
            depth[rank[i]] = depth_bits[i]
    for i in range(n):
        r = rank[i]
        if not tied[r]:
            continue
        a, b = r, r + 1
        while a > 0 and f[a - 1] == f[r]:
            a -= 1
        while b < n and f[b] == f[r]:
            b += 1
        assert tied[a:b].all()
        pos = byrank[a:b] & np.uint64((1 << POS) - 1)
        final[i] = a + int(((depth[a:b] < depth[r]) | ((depth[a:b] == depth[r]) & (pos < np.uint64(i)))).sum())
    assert sorted(final.tolist()) == list(range(n))
    return final, bool(tied.any())


def depths(case, g, n):
    if case == "random":
        return g.uniform(1.0, 10.0, n)
    if case == "all_equal":
        return np.full(n, 4.0)
    if case == "two_values":
        return np.where(g.random(n) < 0.5, 3.0, 5.5)
    if case == "below_the_fraction":     # neighbouring floats: far below what sixteen fraction bits of an eighth of the scene resolve
        return (_bits(np.float32(4.0)) + g.integers(0, 4, n).astype(np.uint32)).view(np.float32)   # 4.0 and its next three floats
    raise KeyError(case)


@pytest.mark.parametrize("n", [257, 320, 511, 512])
@pytest.mark.parametrize("case", ["random", "all_equal", "two_values", "one_bucket_spike", "below_the_fraction"])
def test_finish_gives_the_exact_depth_index_order(case, n):
    g = np.random.default_rng(1000 * n + len(case))
    if case == "one_bucket_spike":
        # the scene: a spread; the tile: a thin band of it — everything in one bucket, fractions still distinct for most
        scene = g.uniform(1.0, 10.0, 200_000).astype(np.float32)
        z = g.uniform(4.0, 4.05, n).astype(np.float32)
    else:
        z = depths(case, g, n).astype(np.float32)
        scene = np.concatenate([z, g.uniform(1.0, 10.0, 50_000).astype(np.float32)]) if case == "random" else z
    f = bucket_map(_bits(scene), np.ones(scene.shape[0], dtype=np.int64), DBITS)
    gid = np.sort(g.choice(1_000_000, n, replace=False)).astype(np.uint32)   # a tile's splats, in index order
    bits = _bits(z)
    a_gid, a_bits, a_key = arrival(bits, gid, f)
    assert (a_key < (1 << (DBITS + FBITS))).all()
    rank, tie = finish(a_key, a_bits)
    got = np.empty(n, dtype=np.uint32)
    got[rank] = a_gid
    want = gid[np.lexsort((gid, bits))]                  # (depth bits, index): the global sort's order
    assert np.array_equal(got, want), case
    if case in ("all_equal", "two_values", "below_the_fraction"):
        assert tie, "equal (bucket, fraction) pairs must be resolved on their depth bits"
    if case == "one_bucket_spike":
        assert np.unique(a_key >> FBITS).shape[0] == 1, "the spike sits in one bucket"
    if case == "all_equal":
        assert np.array_equal(got, gid), "one depth: the index order"


def test_most_tiles_of_a_spread_scene_have_no_tie():
    """What the finish is for: on spread depths a (tile, bucket) segment of about 40 entries rarely holds two equal fractions, so few tiles
    fetch any depth at all."""
    g = np.random.default_rng(9)
    scene = g.uniform(1.0, 10.0, 400_000).astype(np.float32)
    f = bucket_map(_bits(scene), np.ones(scene.shape[0], dtype=np.int64), DBITS)
    tied = 0
    for t in range(200):
        z = scene[g.choice(scene.shape[0], 320, replace=False)]
        gid = np.arange(320, dtype=np.uint32)
        _, a_bits, a_key = arrival(_bits(z), gid, f)
        tied += finish(a_key, a_bits)[1]
    assert tied <= 60, tied   # (expected: 8 segments x C(40, 2) pairs / 2^16 fractions = 0.1 per tile)
