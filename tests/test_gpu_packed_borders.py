"""The packed path (pack_reads.hip -> index_reads.hip -> pileup_tiles.hip, planned by work_plan.h and batch_packed.hip) on small
batches aimed at its borders, each held to the C oracle at tolerance 0 -- counts, reference alleles, the counters of every species
-- on two runs with different thresholds, then to the direct and the long path on the same batch:

  A  stream shapes   a tile's virtual stream S, I, G ending on, before and behind a multiple of a wave's reads, with 1, 3, 4, 5 and
                     8 lanes per read; tiles t and t + grid are a workgroup's first two items, so the prefetch across the tile border
                     meets an empty successor, one with a single record, one that starts with its I or its G range, a long one, none
  B  hand-out        item counts around the grid and around 2 * grid + 8, a new species every five tiles
  C  split tiles     tiles that see 2048, 2049 and 5000 reads, split tiles at a contig's end, side by side, of two species, with
                     records reaching in and out
  D  far reach       records that reach 30, 31, 32 and 40 tiles on, position-sorted and shuffled
  E  refusals        a read the oracle refuses as the first, the last fast-path and the last class-0 record of a stream, as a record
                     reaching in and as another record: every path reports the oracle's status at the oracle's read

The batches come from tests/packed_cases.py with grid = 4 x the device's compute units; tests/test_packed_cases_host.py asserts
without a device that they are what they claim to be (here only for a grid the host test does not cover)."""
import numpy as np
import pytest

from midas_amd import abi
from oracle import c_oracle
from tests import packed_cases as P

pytestmark = pytest.mark.gpu


def _grid(ctx):
    return 4 * ctx.device_info()["compute_units"]


def _run(b, thr, oracle, what):
    """One run of the batch held to the oracle's result; where the oracle refuses the input, the same status at the same read."""
    st, er, oc, oa, os_ = oracle
    if st != 0:
        with pytest.raises(abi.MidasSnpsError) as ei:
            b.run(thr)
            b.fetch()
        assert (ei.value.status, ei.value.read_index) == (st, er), what
        return None
    b.run(thr)
    counts, allele, stats = b.fetch()
    bad = np.nonzero((counts != oc).any(axis=1))[0]
    assert bad.size == 0, "%s: counts differ at %d sites, first %s: hip %s oracle %s" % (
        what, bad.size, bad[:5], counts[bad[:5]].tolist(), oc[bad[:5]].tolist())
    assert np.array_equal(allele, oa), "%s: reference alleles differ at sites %s" % (what, np.nonzero(allele != oa)[0][:8])
    bad = np.nonzero((stats != os_).any(axis=1))[0]
    assert bad.size == 0, "%s: counters differ for %d species, first %s: hip %s oracle %s" % (
        what, bad.size, bad[:5], stats[bad[:5]].tolist(), os_[bad[:5]].tolist())
    return counts, allele, stats


def _assert_same(ctx, thr_default, table, soa, facts, n_work_items=None, repack=False):
    """The packed path twice against the oracle -- the second run with other thresholds, over whatever the first left in the
    tickets, the hand-out counters and the zeroed ranges -- then the direct and the long path against the packed result.
    repack: a third run over a layout packed again and a work plan made again (the same one: nothing is uploaded)."""
    runs = [(thr_default, c_oracle.pileup(thr_default, table, soa)), (P.thresholds(1), c_oracle.pileup(P.thresholds(1), table, soa))]
    b = ctx.batch(table, soa)
    try:
        b.select_path(abi.PATH_PACKED)
        info = b.info()
        assert info.path == abi.PATH_PACKED and (info.lane_bases, info.lanes_per_read) == (facts["lane_bases"], facts["lanes"])
        assert info.n_tiles == facts["n_tiles"] and info.n_reads == len(facts["reads"])
        assert info.n_work_items == (facts["n_tiles"] if n_work_items is None else n_work_items)
        for k, (thr, oracle) in enumerate(runs):
            packed = _run(b, thr, oracle, "packed, run %d" % k)
        if repack:
            b.pack()
            assert b.info().n_work_items == info.n_work_items
            packed = _run(b, runs[1][0], runs[1][1], "packed again")
        for path in (abi.PATH_DIRECT, abi.PATH_LONG):
            try:
                b.select_path(path)
            except abi.MidasSnpsError as e:          # (a path may refuse a batch; none may get it wrong)
                assert e.status == abi.ERR_UNSUPPORTED
                continue
            other = _run(b, runs[1][0], runs[1][1], abi.PATH_NAMES[path])
            if packed is not None:
                assert all(np.array_equal(x, y) for x, y in zip(packed, other))
    finally:
        b.close()
    print("info: lanes_per_read %d, lane_bases %d, tiles %d, work items %d, reads %d, compute units %d" % (
        info.lanes_per_read, info.lane_bases, info.n_tiles, info.n_work_items, info.n_reads, _grid(ctx) // 4))
    return info


def _checked(group, grid, batch):
    if grid not in P.HOST_GRIDS:          # (the host test holds the conditions for those)
        P.CONDITIONS[group](*batch)
    return batch


@pytest.mark.parametrize("lanes", sorted(P.READ_LEN))
def test_stream_shapes(hip_ctx, thr_default, lanes):
    grid = _grid(hip_ctx)
    table, soa, facts = _checked("A", grid, P.stream_batch(lanes, grid))
    info = _assert_same(hip_ctx, thr_default, table, soa, facts)
    assert info.lanes_per_read == lanes and info.n_tiles == 3 * grid > grid      # more whole tiles than workgroups, none split


@pytest.mark.parametrize("which", range(9), ids=["grid-1", "grid", "grid+1", "2grid", "2grid+1", "2grid+7", "2grid+8", "2grid+9", "3grid+5"])
def test_hand_out(hip_ctx, thr_default, which):
    grid = _grid(hip_ctx)
    n_tiles = P.handout_counts(grid)[which]
    table, soa, facts = _checked("B", grid, P.handout_batch(n_tiles))
    info = _assert_same(hip_ctx, thr_default, table, soa, facts)
    assert info.n_tiles == info.n_work_items == n_tiles and table.n_species == -(-n_tiles // 5)


@pytest.mark.parametrize("lanes", [1, 5])
def test_split_tiles(hip_ctx, thr_default, lanes):
    grid = _grid(hip_ctx)
    table, soa, facts = _checked("C", grid, P.split_batch(lanes, grid))
    # a workgroup's fair share of the reads, from the device's compute units: 2049 reads are split, into three parts
    fair = sum(t["sees"] for t in facts["tiles"]) // (4 * hip_ctx.device_info()["compute_units"]) + 1
    assert fair == facts["fair"] and 2 * fair <= 2048 and max(1024, fair) == 1024
    info = _assert_same(hip_ctx, thr_default, table, soa, facts, n_work_items=facts["n_work_items"], repack=True)
    assert info.lanes_per_read == lanes and info.n_work_items == info.n_tiles + 16


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_far_reach(hip_ctx, thr_default, shuffled):
    table, soa, facts = P.far_batch(shuffled)
    info = _assert_same(hip_ctx, thr_default, table, soa, facts)
    assert info.lanes_per_read == 5 and info.n_tiles == P.FAR_TILES + 6


@pytest.mark.parametrize("case", P.REFUSED_CASES, ids=["+".join("%s:%s" % x for x in c).replace(" ", "_") for c in P.REFUSED_CASES])
def test_a_refused_read_in_every_range_of_the_stream(hip_ctx, thr_default, case):
    table, soa, facts = P.refused_batch(case)
    assert c_oracle.pileup(thr_default, table, soa)[0] in P.REFUSED_STATUS.values()
    info = _assert_same(hip_ctx, thr_default, table, soa, facts)
    assert info.lanes_per_read == 5 and info.n_tiles == 7
