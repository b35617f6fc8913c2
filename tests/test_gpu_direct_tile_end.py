"""The tile end of pileup_direct_kernel -- the write-out of a full tile (no bound per row, four rows of tallies read before the
first is stored, the overhang moved in the rows it reaches, whole allele words) beside the bounded one of a contig's last tile --
and the body whose lanes per read are a compile-time four, at contig lengths on both sides of one, two and four tiles.

Every case holds the direct path to the C oracle at tolerance 0 the way tests/test_gpu_direct_shapes.py does: counts, alleles,
per-species counters, two runs of the batch (a run that reports an error raises; the oracle reports none), then the packed path.

Two sets of contigs, each at most ten tiles of 2048 sites:
  SHORT  2048 | 2048 | 2047 | 2049 | 100 | 2048 + 100     the first two are full tiles of ONE chunk and of two species: the
         per-species flush behind a fast-path tile; 100 is shorter than the overhang, and so is the second tile of 2148
  LONG   8192 + 3 | 4096 | 4097      a chunk of four full tiles, then a tile of three sites (no whole word of alleles)
The reference has lower-case letters and an N in the first and the last four sites of every tile.  Read lengths: 150 (four lanes
of 38 bases: the static body), 151 (five lanes of 32), 114 (three of 38), 38 (two of 30: the lane rule gives 38 bases two lanes)
and 30 (one lane: a phase is one iteration), each with baseq 30 and 0.  A dense layer of plain reads covers every site -- a read
starts on every tile's last site and one ends on every tile's first -- under a layer of reads with a clip, an insertion, a
deletion, N bases, low qualities and shorter lengths.  One more case puts a read with a 200-base deletion into the chunk of
four full tiles: the chunk is flagged and its full tiles are written tile by tile.

What keeps a case from passing empty is asserted from the batch and the oracle alone (tile_end_conditions; without a device in
tests/test_direct_tile_end_host.py): the oracle keeps at least half of the reads, and in every tile the first site, the last
site and a site of each row of 256 sites have a depth above zero."""
import functools
import random

import numpy as np
import pytest

from midas_amd import abi
from oracle import c_oracle
from tests import helpers as H
from tests import test_gpu_direct_shapes as S

pytestmark = pytest.mark.gpu
TILE = H.TILE
ROW = 256                                # sites a workgroup writes out in one round

CONTIG_SETS = {"short": ([2048, 2048, 2047, 2049, 100, 2048 + 100], [0, 1, 1, 0, 0, 1]),
               "long": ([8192 + 3, 4096, 4097], [0, 1, 0])}
READ_LENGTHS = (150, 151, 114, 38, 30)
BASEQS = (30, 0)
OUTLIER_GAP = 200


def tile_end_thresholds(baseq):
    return abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq, mapid=50.0, aln_cov=0.0, readq=0))


def tiles_of(lengths):
    """(contig, first site in the contig, sites) of every tile."""
    return [(k, a, min(TILE, n - a)) for k, n in enumerate(lengths) for a in range(0, n, TILE)]


def _reference(rng, n):
    ref = rng.choices("ACGT", k=n)
    for a in range(0, n, TILE):
        e = min(n, a + TILE)
        for j, ch in zip(range(a, min(e, a + 4)), "aNcg"):
            ref[j] = ch
        for j, ch in zip(range(max(a, e - 4), e), "tgNa"):
            ref[j] = ch
    return "".join(ref)


def _read(rng, pos, cigar, noisy):
    l = sum(n for op, n in cigar if op in (0, 1, 4))
    seq = rng.choices("ACGT", k=l)
    qual = [40] * l
    if noisy:
        for _ in range(1 + l // 16):
            seq[rng.randrange(l)] = "N"
            qual[rng.randrange(l)] = rng.choice([0, 12, 29, 30, 31])
    nm = sum(n for op, n in cigar if op in (1, 2))
    return dict(pos=pos, cigar=cigar, seq="".join(seq), qual=qual, nm=nm, mapq=42)


def _contig_reads(rng, n, length, n_noisy):
    """Plain reads every length // 8 sites from the contig's first to its last (what does not fit is clipped: the last of them
    start on the contig's last site), a read that ends on the first site of every tile but the first, and n_noisy others."""
    def fit(pos, l):             # l bases at pos, soft-clipped at the contig's end
        m = min(l, n - pos)
        return [(0, m)] + ([(4, l - m)] if m < l else [])
    rs = [_read(rng, pos, fit(pos, length), False) for pos in range(0, n, max(1, length // 8))]
    rs.append(_read(rng, n - 1, fit(n - 1, length), False))
    for a in range(TILE, n, TILE):
        rs.append(_read(rng, a - 1, fit(a - 1, length), False))                       # starts on a full tile's last site
        rs.append(_read(rng, a - length + 1, fit(a - length + 1, length), False))     # ends on the next tile's first
    for _ in range(n_noisy):
        l = rng.choice([length, length, length - 1, max(1, length // 2), max(1, length // 3)])
        kind = rng.choice(["plain", "clip", "ins", "del", "tail"]) if l >= 12 else "plain"
        a = rng.randrange(1, l - 1) if l >= 12 else 0
        g = rng.randrange(1, 9)
        if kind == "clip":
            cigar, span = [(4, a), (0, l - a)], l - a
        elif kind == "tail":
            cigar, span = [(0, a), (4, l - a)], a
        elif kind == "ins" and a + g < l:
            cigar, span = [(0, a), (1, g), (0, l - a - g)], l - g
        elif kind == "del":
            cigar, span = [(0, a), (2, g), (0, l - a)], l + g
        else:
            cigar, span = [(0, l)], l
        if span <= n:
            rs.append(_read(rng, rng.randrange(0, n - span + 1), cigar, True))
    rs.sort(key=lambda r: r["pos"])
    return rs


@functools.lru_cache(maxsize=4)
def tile_end_batch(set_name, length, outlier=False):
    """-> (ContigTable, ReadsSoA, reads as dicts, contig lengths), position-sorted inside every contig."""
    lengths, species = CONTIG_SETS[set_name]
    rng = random.Random(9000 + 7 * length + len(lengths) + (1 if outlier else 0))
    reads, begin, ref = [], [0], []
    for k, n in enumerate(lengths):
        rs = _contig_reads(rng, n, length, max(40, n // 8))
        if outlier and k == 0:       # one read that spans more than the overhang: its chunk is piled up tile by tile
            a = length // 2
            rs.append(_read(rng, TILE + 900, [(0, a), (2, OUTLIER_GAP), (0, length - a)], False))
            rs[-1]["nm"] = 2         # (the deletion counted as two mismatches: the read passes mapid)
            rs.sort(key=lambda r: r["pos"])
        reads += rs
        begin.append(len(reads))
        ref.append(_reference(rng, n))
    assert max(len(r["seq"]) for r in reads) == length
    table = abi.ContigTable(length=lengths, species=species, read_begin=begin, ref=np.frombuffer("".join(ref).encode(), np.uint8),
                            n_species=2, ids=["c%d" % k for k in range(len(lengths))], species_ids=["s0", "s1"])
    return table, H.reads_from_border_dicts(reads), reads, tuple(lengths)


def tile_end_conditions(lengths, reads, oracle):
    """No device: the case is a few thousand reads on at most ten tiles, the oracle accepts it and keeps at least half of its
    reads, and every tile has depth on its first site, its last site and in each of its rows of 256 sites."""
    st, er, counts, _, stats = oracle
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    tiles = tiles_of(lengths)
    assert len(tiles) <= 10 and 1000 <= len(reads) <= 9000, (len(tiles), len(reads))
    assert int(stats[:, 0].sum()) == len(reads) and 2 * int(stats[:, 1].sum()) >= len(reads), stats.tolist()
    depth = counts.sum(axis=1)
    base = np.concatenate([[0], np.cumsum(lengths)])
    for k, a, n in tiles:
        d = depth[base[k] + a: base[k] + a + n]
        assert d[0] > 0 and d[-1] > 0, (k, a, n)
        assert all(d[r: r + ROW].max() > 0 for r in range(0, n, ROW)), (k, a, n)
    return tiles


def border_reads_present(lengths, table, reads, length):
    """A read starts on the last site of every full tile and one ends on the first site of every tile behind a full one."""
    for k, n in enumerate(lengths):
        rs = reads[int(table.read_begin[k]): int(table.read_begin[k + 1])]
        starts = set(r["pos"] for r in rs)
        ends = set(r["pos"] + H.cigar_span(r["cigar"]) - 1 for r in rs if r["cigar"] == [(0, length)])
        for a in range(TILE, n + 1, TILE):
            assert a - 1 in starts, (k, a)
            assert a >= n or a in ends or a - length + 1 < 0, (k, a)


def _check(hip_ctx, request, set_name, length, baseq, outlier=False):
    table, soa, reads, lengths = tile_end_batch(set_name, length, outlier)
    thr = tile_end_thresholds(baseq)
    oracle = c_oracle.pileup(thr, table, soa)
    tile_end_conditions(lengths, reads, oracle)
    border_reads_present(lengths, table, reads, length)
    info = S._same_on_both_paths(hip_ctx, thr, table, soa, length, oracle, (H.OVERHANG, 4), request)
    assert (info.lane_bases, info.lanes_per_read) == H.direct_lane_shape(length)
    assert (info.direct_overhang, info.direct_chunk_tiles) == (H.OVERHANG, 4)
    return info


@pytest.mark.parametrize("baseq", BASEQS)
@pytest.mark.parametrize("length", READ_LENGTHS)
@pytest.mark.parametrize("set_name", sorted(CONTIG_SETS))
def test_full_and_partial_tiles_at_every_contig_length(hip_ctx, request, set_name, length, baseq):
    info = _check(hip_ctx, request, set_name, length, baseq)
    want = {150: (38, 4), 151: (32, 5), 114: (38, 3), 38: (30, 2), 30: (30, 1)}[length]
    assert (info.lane_bases, info.lanes_per_read) == want


@pytest.mark.parametrize("baseq", BASEQS)
def test_a_flagged_chunk_writes_its_full_tiles_one_by_one(hip_ctx, request, baseq):
    """A read with a 200-base deletion spans more than the overhang: the chunk of four full tiles it lies in carries nothing from
    tile to tile (every tile streams the reads that reach in), the batch keeps its chunks."""
    table, soa, reads, lengths = tile_end_batch("long", 150, True)
    spans = [H.cigar_span(r["cigar"]) for r in reads]
    assert sorted(spans)[-1] == 150 + OUTLIER_GAP and sorted(spans)[-2] <= H.OVERHANG
    assert reads[spans.index(150 + OUTLIER_GAP)]["pos"] // TILE == 1
    info = _check(hip_ctx, request, "long", 150, baseq, True)
    assert (info.lane_bases, info.lanes_per_read) == (38, 4)
