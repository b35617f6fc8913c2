"""tests/index_model.py held to brute force, without a device: a few hundred small random batches -- sorted and shuffled, with and
without reads that span more than the overhang, with empty contigs, with starts in front of and behind their contig -- on which
every tile's range is derived again from the sites each read really touches, by the slowest rule that is obviously right."""
import random
import re

import numpy as np
import pytest

from tests import index_model as M

LENGTHS = (1, 100, 2047, 2048, 2049, 4096, 5000, 9000, 2048 * 5 + 7)


def random_batch(seed, oracle_ok=False):
    """(length, read_begin, pos, l_seq, cigars, nm) of a small batch.  oracle_ok: only reads a pileup accepts (an NM tag, an
    aligned base), for tests/test_gpu_index.py, which also runs the batch."""
    rng = random.Random(seed)
    shuffled, with_outliers, long_reads = seed % 2 == 1, seed % 4 >= 2, seed % 8 in (4, 6)
    length, read_begin, pos, l_seq, cigars, nm = [], [0], [], [], [], []
    for _ in range(rng.randint(1, 5)):
        ln = rng.choice(LENGTHS)
        n = rng.choice([0, 0, 1, 2, rng.randint(3, 40), rng.randint(20, 60)])
        rs = []
        for _ in range(n):
            l = rng.randint(161, 300) if long_reads and rng.random() < 0.2 else rng.randint(30, 150)
            p = rng.choice([rng.randint(0, ln - 1), rng.randint(-3, 3), ln - 1 - rng.randint(0, 200), ln + rng.randint(0, 3),
                            (rng.randint(0, ln - 1) >> 11 << 11) + rng.choice([-160, -151, -150, -1, 0, 1])])
            a = rng.randint(1, l - 1)
            kind = rng.random()
            if with_outliers and kind < 0.25:
                cg = [(0, a), (rng.choice([2, 3]), rng.choice([11, 161 - l, 2000, 2048 + 160 - l, 6000])), (0, l - a)]
                cg = [(op, max(k, 1)) for op, k in cg]
            elif kind < 0.3:
                cg = [(4, a), (0, l - a)]
            elif kind < 0.35 and not oracle_ok:
                cg = [(4, l)]                                # no aligned base: span 0
            elif kind < 0.4:
                cg = [(5, 2), (7, a), (8, l - a)]
            else:
                cg = [(0, l)]
            rs.append((p, l, cg, rng.choice([0, 1, 1 if oracle_ok else -1])))
        rs.sort(key=lambda r: r[0])
        if shuffled:
            rng.shuffle(rs)
        for p, l, cg, m in rs:
            pos.append(p); l_seq.append(l); cigars.append(cg); nm.append(m)
        length.append(ln)
        read_begin.append(len(pos))
    return length, read_begin, pos, l_seq, cigars, nm


def touched_tiles(m, length, pos, i):
    """Tiles that hold a site read i really covers, by its clamped sites one tile at a time."""
    c = m["contig"][i]
    lo, hi = max(pos[i], 0), min(pos[i] + m["span"][i] - 1, length[c] - 1)
    return set() if hi < lo else set(m["tile_base"][c] + s // 2048 for s in range(lo - lo % 2048, hi + 1, 2048))


@pytest.mark.parametrize("block", range(8))
def test_model_ranges_against_brute_force(block):
    seen = dict(sorted=0, unsorted=0, chunks=0, listed=0, flagged=0, empty=0, long=0)
    for seed in range(block * 40, block * 40 + 40):
        length, read_begin, pos, l_seq, cigars, nm = random_batch(seed)
        m = M.index_model(length, read_begin, pos, l_seq, cigars, nm)
        f, tb, te = m["facts"], m["tbegin"].astype(np.int64), m["tend"].astype(np.int64)
        n = len(pos)
        tb[tb == M.NONE] = 1 << 40
        is_sorted = not f["unsorted"]
        seen["sorted" if is_sorted else "unsorted"] += 1
        seen["chunks"] += f["direct_chunks"]; seen["listed"] += len(m["outliers"]); seen["flagged"] += int(m["tile_flag"].sum())
        seen["long"] += f["direct_overhang"] == 288
        # sortedness, by its definition on the raw columns
        brute_unsorted = False
        for c in range(len(length)):
            cl = [min(max(p, 0), length[c] - 1) for p in pos[read_begin[c]:read_begin[c + 1]]]
            brute_unsorted |= any(a > b for a, b in zip(cl, cl[1:]))
            seen["empty"] += not cl
        assert brute_unsorted == bool(f["unsorted"])
        # every read lies in the range of every tile it touches, and of the tile it starts in
        for i in range(n):
            for t in touched_tiles(m, length, pos, i) | {m["ka"][i]}:
                assert tb[t] <= i < te[t], (seed, i, t, tb[t], te[t])
            # ... and of every tile its reach interval meets, unless it is a listed outlier (then: of those it reaches)
            if m["span"][i] <= f["direct_overhang"] or f["direct_reach_ranges"] == f["direct_reach"]:
                for t in range(m["ka"][i], m["kb"][i] + 1):
                    assert tb[t] <= i < te[t], (seed, i, t)
        # minimality
        reach = {}
        for i in range(n):
            ts = set(range(m["ka"][i], m["kb"][i] + 1))
            if f["direct_reach_ranges"] != f["direct_reach"] and m["span"][i] > f["direct_overhang"]:
                ts |= touched_tiles(m, length, pos, i)
            for t in ts:
                reach.setdefault(t, []).append(i)
        for c in range(len(length)):
            lo, hi = read_begin[c], read_begin[c + 1]
            for t in range(m["tile_base"][c], m["tile_base"][c + 1]):
                if is_sorted:
                    if lo == hi:
                        assert (m["tbegin"][t], m["tend"][t]) == (M.NONE, 0)
                        continue
                    assert te[t] - lo == sum(1 for i in range(lo, hi) if m["ka"][i] <= t), (seed, t)
                    # the least index that can reach t: a read whose start + reach gets there, or a listed outlier that does
                    can = [i for i in range(lo, hi) if m["kb"][i] >= t] + [i for i in reach.get(t, []) if m["ka"][i] <= t]
                    assert tb[t] == (min(can) if can else 1 << 40), (seed, t)
                else:
                    assert (tb[t], te[t]) == ((min(reach[t]), max(reach[t]) + 1) if t in reach else (1 << 40, 0)), (seed, t)
        streams = np.maximum(te - tb, 0)
        assert m["stream_reads"] == int(streams.sum()) and m["max_tile_reads"] == int(streams.max())
    assert seen["sorted"] >= 10 and seen["unsorted"] >= 5 and seen["chunks"] >= 10 and seen["empty"] >= 10, seen


def test_the_random_batches_cover_their_kinds():
    """What keeps the brute-force test from passing on batches that never list an outlier, flag a tile or take the long overhang."""
    listed = flagged = long_overhang = no_chunks_sorted = 0
    for seed in range(320):
        m = M.index_model(*random_batch(seed))
        listed += len(m["outliers"]) > 0
        flagged += bool(m["tile_flag"].any()) and m["chunk_ok"].size > 0 and not m["chunk_ok"].all()
        long_overhang += m["facts"]["direct_overhang"] == 288
        no_chunks_sorted += not m["facts"]["unsorted"] and not m["facts"]["direct_chunks"]
    assert min(listed, flagged, long_overhang, no_chunks_sorted) >= 5, (listed, flagged, long_overhang, no_chunks_sorted)


def test_model_facts_on_hand_made_reads():
    """The per-read rules on cases small enough to do by hand."""
    cg = lambda s: [("MIDNSHP=X".index(op), int(k)) for k, op in re.findall(r"(\d+)([MIDNSHP=X])", s)]
    assert M.cigar_span(cg("5S10M2I3D4N6=7X8S2H")) == 30
    for text, l, fast in (("50M", 50, True), ("5S45M", 50, True), ("45M5S", 50, True), ("5S40M5S", 50, True), ("20M3I27M", 50, True),
                          ("20M3D30M", 50, True), ("5S20M3N25M", 50, True), ("20M3I22M5S", 50, True), ("5S20M3I17M5S", 50, False),
                          ("2H50M", 50, False), ("25=25X", 50, False), ("50M", 51, False), ("50S", 50, False), ("20M65535D30M", 50, True),
                          ("20M65536D30M", 50, False), ("20M2P30M", 50, False), ("50=", 50, True), ("20I30M", 50, False)):
        assert M.fast_shape(cg(text), l) == fast, text
    # one contig of three tiles: reads 0 1 | 2 | - by their start tiles; the third is an outlier into tile 2
    m = M.index_model([5000], [0, 3], [0, -1, 2047 + 1], [50, 50, 50], [cg("50M"), cg("50M"), cg("10M2500N40M")], [0, -1, 0])
    f = m["facts"]
    assert (f["unsorted"], f["max_l"], f["max_span"], f["max_common"], f["n_outliers"], f["n_general"]) == (0, 50, 2550, 50, 1, 1)
    assert (f["direct_reach"], f["direct_reach_ranges"], f["direct_chunks"], f["direct_overhang"]) == (2550, 50, 1, 160)
    assert f["alg"] == 3 * (25 + 50 + 16) + 4 * (1 + 1 + 3)
    assert m["outliers"] == [(2, 2, 2)] and m["tile_flag"].tolist() == [0, 1, 1] and m["chunk_ok"].tolist() == [1]      # (n_chunked == 0)
    assert m["tbegin"].tolist() == [0, 2, 2] and m["tend"].tolist() == [2, 3, 3]
    # pos 0 then -1 is sorted; 1 then 0 is not
    assert M.index_model([100], [0, 2], [0, -1], [30, 30], [cg("30M")] * 2, [0, 0])["facts"]["unsorted"] == 0
    assert M.index_model([100], [0, 2], [1, 0], [30, 30], [cg("30M")] * 2, [0, 0])["facts"]["unsorted"] == 1
    # a drop across a contig border alone leaves the batch sorted
    assert M.index_model([100, 100], [0, 1, 2], [50, 0], [30, 30], [cg("30M")] * 2, [0, 0])["facts"]["unsorted"] == 0
    # the overhang follows the longest read of a sorted batch
    for max_l, want in ((160, 160), (161, 288), (288, 288), (289, 160)):
        got = M.index_model([9000], [0, 1], [0], [max_l], [[(0, max_l)]], [0])
        assert got["facts"]["direct_overhang"] == want and got["chunk_tiles"] == (4 if max_l <= 288 else 1)
