"""Every instantiation of pileup_direct_kernel<LB, BQ0, OV> other than the two of 38 bases per lane (test_gpu_wide_lanes.py), at
its own edges: each lane width (30, 32), each lane count (1 .. 10), each overhang (160, 288, and 160 without chunks for reads
beyond 288 bases), at the smallest and the largest longest-read length that selects the cell.  Every case holds the direct path
to the C oracle at tolerance 0 -- counts, alleles, stats, two runs of the batch -- and then to the packed path.

The border batches (tests/helpers.py border_batch) put clips, insertions and deletions exactly on and around every lane border
k*LB of the cell; the conditions that keep them from passing for the wrong reason are asserted on the host before anything runs
on the device (helpers.border_conditions; tests/test_direct_shapes_host.py asserts the same without a device).

Which kernel a case launches follows from what it asserts of info() and from its baseq: <lane_bases, baseq <= 0,
direct_overhang>.  One class of cases launches none: the direct layout keeps a quality up to 50 (layout.h kDenseMaxQual), so a
run with baseq 51 over a batch that holds an A/C/G/T quality above 50 -- every border batch does -- is served by the long path
(batch.hip).  Those cases hold that detour to the oracle at these shapes; their cells run once more with baseq 41, so that
every cell launches both of its instantiations.  Reads with a hard clip or a start in front of the contig are walked op by op, as
the five-op reads are: all three count in direct_general_reads."""
import functools

import numpy as np
import pytest

from midas_amd import abi, synth
from oracle import c_oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu
TILE, CHUNK = H.TILE, H.CHUNK

# (lane_bases, overhang, chunk tiles, lanes per read, the smallest and the largest longest read that selects the cell)
CELLS = [(30, 160, 4, 1, (30,)), (30, 160, 4, 2, (33, 60)), (30, 160, 4, 3, (65, 90)), (30, 160, 4, 4, (115, 120)),
         (32, 160, 4, 1, (31, 32)), (32, 160, 4, 2, (61, 64)), (32, 160, 4, 3, (91, 96)), (32, 160, 4, 4, (121, 128)),
         (32, 160, 4, 5, (151, 160)),
         (30, 288, 4, 6, (161, 180)), (30, 288, 4, 7, (193, 210)), (30, 288, 4, 8, (225, 240)), (30, 288, 4, 9, (257, 270)),
         (32, 288, 4, 6, (181, 192)), (32, 288, 4, 7, (211, 224)), (32, 288, 4, 8, (241, 256)), (32, 288, 4, 9, (271, 288)),
         (30, 160, 1, 10, (289, 300)), (32, 160, 1, 10, (301, 320))]
BASEQ_CLASSES = (30, 41, 51)      # dealt to the cells in turn: each meets each lane width and each overhang


def _cell_id(cell, max_len):
    return "lb%d-ov%d%s-%dlanes-len%d" % (cell[0], cell[1], "" if cell[2] > 1 else "nochunks", cell[3], max_len)


def _border_cases():
    out = []
    for k, cell in enumerate(CELLS):
        bq = BASEQ_CLASSES[k % 3]
        for max_len in cell[4]:
            for baseq in (0, bq) + ((41,) if bq > 50 else ()):
                out.append(pytest.param(cell, max_len, baseq, id="%s-baseq%d" % (_cell_id(cell, max_len), baseq)))
    return out


def border_thresholds(baseq):
    return abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq, mapid=50.0, aln_cov=0.2, readq=0))


@functools.lru_cache(maxsize=2)
def border_batch_of(lane_bases, max_len, overhang):
    return H.border_batch(lane_bases, max_len, overhang, seed=1000 * max_len + lane_bases)


def _kernel_name(info, thr, reads):
    if thr.baseq > 50 and bool((reads.qual > 50).any()):
        return "pileup_long (baseq above the direct layout's qualities)"
    return "pileup_direct_kernel<%d, %s, %d>" % (info.lane_bases, "true" if thr.baseq <= 0 else "false", info.direct_overhang)


def _same_on_both_paths(ctx, thr, contigs, reads, max_len, oracle=None, want=None, request=None, kernel=None):
    """The direct path twice against the oracle, then the packed path against the direct one.  want: (overhang, chunk tiles)."""
    st, er, oc, oa, os_ = oracle or c_oracle.pileup(thr, contigs, reads)
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    b = ctx.batch(contigs, reads)
    try:
        b.select_path(abi.PATH_DIRECT)
        info = b.info()
        assert (info.lane_bases, info.lanes_per_read) == H.direct_lane_shape(max_len)
        assert (info.direct_overhang, info.direct_chunk_tiles) == (want or H.direct_overhang_shape(max_len))
        if request is not None:      # (a property of the case's report: which kernel the case launches)
            request.node.user_properties.append(("kernel", kernel or _kernel_name(info, thr, reads)))
        for _ in range(2):
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


# ---- 1, 2: clips and indels on the lane borders of every cell ------------------------------------------------------------------

@pytest.mark.parametrize("cell,max_len,baseq", _border_cases())
def test_clips_and_indels_on_the_lane_borders_of_every_cell(hip_ctx, request, cell, max_len, baseq):
    lane_bases, overhang, chunk_tiles, lanes, _ = cell
    assert H.direct_lane_shape(max_len) == (lane_bases, lanes) and H.direct_overhang_shape(max_len) == (overhang, chunk_tiles)
    table, soa, reads = border_batch_of(lane_bases, max_len, overhang)
    thr = border_thresholds(baseq)
    oracle = c_oracle.pileup(thr, table, soa)
    assert oracle[0] == 0, "oracle refused the input (%d at read %d)" % oracle[:2]
    H.border_conditions(reads, lane_bases, max_len, oracle[2], oracle[4])
    info = _same_on_both_paths(hip_ctx, thr, table, soa, max_len, oracle, (overhang, chunk_tiles), request)
    assert (info.lane_bases, info.lanes_per_read) == (lane_bases, lanes)
    assert 0 < info.direct_general_reads <= len(reads) // 8


# ---- 3: seeded datasets per cell -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def _dataset(read_len, var_len):
    return synth.make_dataset(n_species=2, contigs_per_species=2, contig_len=3 * CHUNK + 1111, n_reads=6000, read_len=read_len,
                              seed=7000 + read_len, var_len=var_len, lowercase_frac=0.1)


def _dataset_cases():
    out = []
    for cell in CELLS:
        for var_len in (False, True) if cell[1] == 160 else (False,):       # (var_len: the lane counts below the cell's share a wave)
            for baseq in (30, 0):
                out.append(pytest.param(cell, var_len, baseq, id="%s%s-baseq%d" % (_cell_id(cell, cell[4][-1]), "-varlen" if var_len else "", baseq)))
    return out


@pytest.mark.parametrize("cell,var_len,baseq", _dataset_cases())
def test_seeded_datasets_of_every_cell(hip_ctx, request, cell, var_len, baseq):
    lane_bases, overhang, chunk_tiles, lanes, lengths = cell
    contigs, reads = _dataset(lengths[-1], var_len)
    assert int(reads.l_seq.max()) == lengths[-1] and (not var_len or int(reads.l_seq.min()) <= max(20, lengths[-1] // 2))
    thr = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq))
    info = _same_on_both_paths(hip_ctx, thr, contigs, reads, lengths[-1], None, (overhang, chunk_tiles), request)
    assert (info.lane_bases, info.lanes_per_read) == (lane_bases, lanes)


# ---- 4: the long overhang's own edges ------------------------------------------------------------------------------------------

OUTLIER_SPANS = (289, 300, 600, TILE + 7)          # beyond the long overhang: listed as outliers
COMMON_SPANS = (288, 287)                          # within it


def _outlier_batch(lane_bases, max_len):
    def stretched(k, n, rng):
        rs = []
        borders = [x for x in (TILE, CHUNK, CHUNK + TILE) if x < n - 800]      # tile, chunk and tile borders
        for j, b in enumerate(borders):
            for span in OUTLIER_SPANS + COMMON_SPANS:
                a = lane_bases * (1 + (j + span) % ((max_len - 1) // lane_bases))      # the gap on a lane border
                gap = span - max_len
                rs.append(dict(pos=b - a - rng.choice([0, 1, gap // 2]), cigar=[(0, a), (2, gap), (0, max_len - a)],
                               seq="".join(rng.choices("ACGT", k=max_len)), qual=[40] * max_len, nm=rng.choice([0, 1, 2]), mapq=42,
                               kind="stretched", events=[]))
        return rs
    return H.border_batch(lane_bases, max_len, 288, seed=4000 + max_len, extra=stretched)


@pytest.mark.parametrize("lane_bases,max_len", [(32, 250), (30, 170)])
@pytest.mark.parametrize("baseq", [0, 30])
def test_outliers_against_the_long_overhang(hip_ctx, request, lane_bases, max_len, baseq):
    """Reads whose deletion stretches them beyond 288 sites -- the gap on a lane border, the read over a tile or a chunk border --
    are listed as outliers and their chunks piled up tile by tile; spans of 288 and 287 are not.  The batch keeps its chunks."""
    table, soa, reads = _outlier_batch(lane_bases, max_len)
    spans = [H.cigar_span(r["cigar"]) for r in reads]
    assert max(s for s, r in zip(spans, reads) if r["kind"] != "stretched") <= 288
    for s in OUTLIER_SPANS + COMMON_SPANS:
        at = [r for r, sp in zip(reads, spans) if sp == s and r["kind"] == "stretched"]
        assert len(at) >= 3 and all(r["cigar"][0][1] % lane_bases == 0 for r in at)
        assert any(r["pos"] < CHUNK <= r["pos"] + s for r in at) and any(r["pos"] < TILE <= r["pos"] + s for r in at)
    thr = border_thresholds(baseq)
    oracle = c_oracle.pileup(thr, table, soa)
    assert oracle[0] == 0 and 10 * int(oracle[4][:, 1].sum()) >= 9 * len(reads)
    _same_on_both_paths(hip_ctx, thr, table, soa, max_len, oracle, (288, 4), request)


@pytest.mark.parametrize("mapid,aln_cov", [(100.0, 1.0), (0.0, 0.0), (-20000.0, 0.2)])
@pytest.mark.parametrize("baseq", [0, 30])
def test_filter_tables_of_16_bits_and_beyond(hip_ctx, request, mapid, aln_cov, baseq):
    """The long-overhang instantiation keeps the read filter's tables as 16-bit entries: the strictest and the loosest thresholds
    that fit them, and an identity threshold whose entry for 250 bases (-50 000 matches) does not -- that run takes the common
    instantiation tile by tile (batch.hip filt_fits16), the batch still reporting its chunks."""
    table, soa, reads = border_batch_of(32, 250, 288)
    thr = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, baseq=baseq, mapid=mapid, aln_cov=aln_cov, readq=0))
    oracle = c_oracle.pileup(thr, table, soa)
    assert oracle[0] == 0 and int(oracle[2].sum()) > 0
    kept = int(oracle[4][:, 1].sum())
    assert 0 < kept < len(reads) // 2 if mapid == 100.0 else kept > len(reads) * 9 // 10      # (exact, unclipped reads only / nearly all)
    kernel = None if mapid > -11000.0 else "pileup_direct_kernel<32, %s, 160> (tables beyond 16 bits)" % ("true" if baseq <= 0 else "false")
    _same_on_both_paths(hip_ctx, thr, table, soa, 250, oracle, (288, 4), request, kernel)


@pytest.mark.parametrize("max_len,want", [(160, (32, 5, 160, 4)), (161, (30, 6, 288, 4)), (288, (32, 9, 288, 4)), (289, (30, 10, 160, 1))])
@pytest.mark.parametrize("baseq", [0, 30])
def test_one_base_either_side_of_the_overhang_switch(hip_ctx, request, max_len, want, baseq):
    """160 bases keep the common overhang, 161 take the long one, 288 still do, 289 leave the chunks: the same seed and contigs."""
    lane_bases = H.direct_lane_shape(max_len)[0]
    table, soa, reads = H.border_batch(lane_bases, max_len, H.direct_overhang_shape(max_len)[0], seed=4242, lengths=H.border_contigs(288))
    thr = border_thresholds(baseq)
    oracle = c_oracle.pileup(thr, table, soa)
    assert oracle[0] == 0
    H.border_conditions(reads, lane_bases, max_len, oracle[2], oracle[4])
    info = _same_on_both_paths(hip_ctx, thr, table, soa, max_len, oracle, want[2:], request)
    assert (info.lane_bases, info.lanes_per_read, info.direct_overhang, info.direct_chunk_tiles) == want
