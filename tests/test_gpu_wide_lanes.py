"""The direct kernel's 38-base lanes (pileup_direct.hip, direct_lane_bases): a batch whose longest read has 129 .. 150 bases
puts a read on four lanes of 38, one of 97 .. 114 bases on three, where 30 or 32 bases per lane take a lane more.  The
cases put the reads where the wider lane can go wrong -- clips and indels on and around the new lane borders (query offsets
38, 76, 114), reads over tile and chunk borders, an outlier deletion, lower-case reference, every base-quality threshold
class -- and hold the device to the C oracle and to the packed path through the C-ABI.  Tolerance 0."""
import random

import numpy as np
import pytest

from midas_amd import abi, synth
from oracle import c_oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu
TILE = 2048
CHUNK = 4 * TILE
BORDERS = (37, 38, 39, 75, 76, 77, 113, 114, 115)      # query offsets on both sides of the lanes' borders


def _same_on_both_paths(ctx, thr, contigs, reads, max_len, runs=1):
    st, er, oc, oa, os_ = c_oracle.pileup(thr, contigs, reads)
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    b = ctx.batch(contigs, reads)
    try:
        b.select_path(abi.PATH_DIRECT)
        info = b.info()
        assert (info.lane_bases, info.lanes_per_read) == H.direct_lane_shape(max_len)
        for _ in range(runs):
            b.run(thr)
            counts, allele, stats = b.fetch()
            bad = np.nonzero((counts != oc).any(axis=1))[0]
            assert bad.size == 0, "direct: counts differ at %d sites, first %s: hip %s oracle %s" % (
                bad.size, bad[:5], counts[bad[:5]].tolist(), oc[bad[:5]].tolist())
            assert np.array_equal(allele, oa) and np.array_equal(stats, os_)
        b.select_path(abi.PATH_PACKED)
        b.run(thr)
        c2, a2, s2 = b.fetch()
        assert np.array_equal(c2, counts) and np.array_equal(a2, allele) and np.array_equal(s2, stats)
    finally:
        b.close()
    return info


@pytest.mark.parametrize("read_len", [97, 114, 129, 149, 150, 152])
def test_seeded_batches_of_one_read_length(hip_ctx, thr_default, read_len):
    contigs, reads = synth.make_dataset(n_species=2, contigs_per_species=2, contig_len=3 * CHUNK + 1111, n_reads=12000,
                                        read_len=read_len, seed=380 + read_len, lowercase_frac=0.1)
    info = _same_on_both_paths(hip_ctx, thr_default, contigs, reads, read_len)
    want = {97: (38, 3), 114: (38, 3), 129: (38, 4), 149: (38, 4), 150: (38, 4), 152: (32, 5)}[read_len]
    assert (info.lane_bases, info.lanes_per_read) == want


def test_150_takes_four_lanes_of_38_and_151_keeps_five_of_32(hip_ctx, thr_default):
    for read_len, want in ((150, (38, 4)), (151, (32, 5))):
        contigs, reads = synth.make_dataset(n_species=1, contigs_per_species=2, contig_len=9000, n_reads=3000,
                                            read_len=read_len, seed=5)
        b = hip_ctx.batch(contigs, reads)
        b.select_path(abi.PATH_DIRECT)
        info = b.info()
        b.close()
        assert (info.lane_bases, info.lanes_per_read) == want
        _same_on_both_paths(hip_ctx, thr_default, contigs, reads, read_len)


@pytest.mark.parametrize("seed", [1, 2])
def test_mixed_lengths_up_to_150(hip_ctx, thr_default, seed):
    contigs, reads = synth.make_dataset(n_species=3, contigs_per_species=3, contig_len=CHUNK + 2 * TILE + 31, n_reads=30000,
                                        read_len=150, seed=3800 + seed, var_len=True, lowercase_frac=0.05)
    assert int(reads.l_seq.max()) == 150 and int(reads.l_seq.min()) < 97
    info = _same_on_both_paths(hip_ctx, thr_default, contigs, reads, 150, runs=2)
    assert (info.lane_bases, info.lanes_per_read) == (38, 4)


def _border_reads(rng, length, max_len, n):
    """Reads whose clips, insertions and deletions start or end on and around the lane borders, half of them placed over a
    tile or chunk border."""
    out = []
    tile_borders = list(range(TILE, length, TILE))
    for _ in range(n):
        l = rng.choice([max_len, max_len, max_len - 1, 120, 97, 77, 76, 39, 38]) if max_len >= 129 else rng.choice([max_len, 97, 77, 76, 39, 38])
        l = min(l, max_len)
        offs = [o for o in BORDERS if 1 <= o <= l - 2] or [l // 2]
        kind = rng.random()
        if kind < 0.15:
            cigar, span = [(0, l)], l
        elif kind < 0.35:                    # a leading / trailing / both-sided soft clip ending on a border
            s = rng.choice(offs) if rng.random() < 0.6 else 0
            t = l - rng.choice([o for o in offs if o > s]) if rng.random() < 0.6 and any(o > s for o in offs) else 0
            m = l - s - t
            cigar = ([(4, s)] if s else []) + [(0, m)] + ([(4, t)] if t else [])
            span = m
        elif kind < 0.60:                    # an insertion that starts or ends on a border
            i = rng.randint(1, 4)
            a = rng.choice(offs) - (i if rng.random() < 0.5 else 0)
            a = max(1, min(l - i - 1, a))
            cigar, span = [(0, a), (1, i), (0, l - a - i)], l - i
        elif kind < 0.85:                    # a deletion at a border (the span stays within the overhang)
            a = rng.choice(offs)
            d = rng.randint(1, max(1, 160 - l))
            cigar, span = [(0, a), (2, d), (0, l - a)], l + d
        elif kind < 0.93:                    # clip + indel: four ops, still settled in registers
            s = rng.choice([o for o in offs if o < l - 12] or [1])
            a = rng.randint(1, l - s - 6)
            i = rng.randint(1, 3)
            cigar, span = [(4, s), (0, a), (1, i), (0, l - s - a - i)], l - s - i
        else:                                # five ops: walked op by op
            a = rng.choice([o for o in offs if o < l - 20] or [5])
            cigar, span = [(0, a), (3, 3), (7, 6), (8, 2), (0, l - a - 8)], l + 3
        if tile_borders and rng.random() < 0.5:
            b = rng.choice(tile_borders)
            pos = b - rng.randint(0, span + 2) + rng.choice([0, 0, 1, -1])
        else:
            pos = rng.randint(-2, length - 1)
        pos = max(-2, min(length - 1, pos))
        out.append(dict(pos=pos, cigar=cigar, seq="".join(rng.choice("ACGTACGTACGTN") for _ in range(l)),
                        qual=[rng.choice([60, 51, 50, 41, 40, 31, 30, 29, 12, 0]) for _ in range(l)], nm=rng.choice([0, 1, 2, 3]),
                        mapq=rng.choice([42, 42, 30, 19])))
    return out


def _border_table(rng, lengths, max_len, extra=None):
    reads, begin, ref = [], [0], []
    for k, n in enumerate(lengths):
        rs = _border_reads(rng, n, max_len, max(60, n // 10))
        if extra:
            rs += extra(k, n)
        rs.sort(key=lambda r: r["pos"])
        reads += rs
        begin.append(len(reads))
        ref.append("".join(rng.choice("ACGTacgtN") for _ in range(n)))
    assert max(len(r["seq"]) for r in reads) == max_len
    soa = H.reads_from_dicts(reads)
    table = abi.ContigTable(length=lengths, species=[k % 2 for k in range(len(lengths))], read_begin=begin,
                            ref=np.frombuffer("".join(ref).encode(), np.uint8), n_species=2,
                            ids=["c%d" % k for k in range(len(lengths))], species_ids=["s0", "s1"])
    return table, soa


@pytest.mark.parametrize("max_len", [150, 149, 129, 114, 97])
@pytest.mark.parametrize("baseq", [0, 30, 41, 51])
def test_clips_and_indels_on_the_lane_borders(hip_ctx, max_len, baseq):
    rng = random.Random(1000 * max_len + baseq)
    table, soa = _border_table(rng, [2 * CHUNK + 5, TILE, TILE * 3 - 1, CHUNK + 160, 700, TILE * 5 + 161], max_len)
    thr = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq, mapid=50.0, aln_cov=0.2, readq=0))
    info = _same_on_both_paths(hip_ctx, thr, table, soa, max_len, runs=2)
    assert info.lane_bases == 38 and info.lanes_per_read == (4 if max_len >= 129 else 3)
    assert info.direct_chunk_tiles == 4 and info.direct_overhang == 160


def test_an_outlier_deletion_among_wide_lanes(hip_ctx):
    """A read whose deletion stretches it beyond the overhang: listed as an outlier, its chunk piled up tile by tile -- with
    the gap on a lane border, and the read over a tile and a chunk border."""
    rng = random.Random(77)

    def outliers(k, n):
        rs = []
        for b in [x for x in (TILE, CHUNK, CHUNK + TILE) if x < n - 800]:
            for a, gap in ((38, 200), (76, 500), (114, 23), (75, TILE + 7)):
                rs.append(dict(pos=b - a - rng.choice([0, 1, gap // 2]), cigar=[(0, a), (2, gap), (0, 150 - a)],
                               seq="".join(rng.choice("ACGT") for _ in range(150)), qual=[40] * 150, nm=gap, mapq=42))
        return rs

    table, soa = _border_table(rng, [3 * CHUNK + 9, CHUNK + TILE + 5, 900], 150, extra=outliers)
    thr = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, mapid=0.0))
    info = _same_on_both_paths(hip_ctx, thr, table, soa, 150, runs=2)
    assert (info.lane_bases, info.lanes_per_read) == (38, 4)
