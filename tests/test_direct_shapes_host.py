"""The inputs of tests/test_gpu_direct_shapes.py, checked without a device: the cell table against the lane rule, and for every
border batch what keeps its case from passing for the wrong reason -- the oracle accepts it, every lane border carries a clip, an
insertion and a deletion, the oracle tallies something and keeps at least nine reads in ten."""
import pytest

from oracle import c_oracle
from tests import helpers as H
from tests import test_gpu_direct_shapes as S


def test_the_cell_table_follows_the_lane_rule():
    """Every longest read from 1 to 320 bases belongs to the cell the table names, or to the 38-base lanes."""
    seen = {}
    for max_len in range(1, 321):
        lb, lanes = H.direct_lane_shape(max_len)
        seen.setdefault((lb, lanes) + H.direct_overhang_shape(max_len), []).append(max_len)
    for lb, overhang, chunk_tiles, lanes, lengths in S.CELLS:
        got = seen.pop((lb, lanes, overhang, chunk_tiles))
        assert (got[0], got[-1]) == (1 if lanes == 1 and lb == 30 else lengths[0], lengths[-1]), (lb, lanes, got)
        assert got == list(range(got[0], got[-1] + 1))
    assert sorted(seen) == [(38, 3, 160, 4), (38, 4, 160, 4)] and seen[(38, 3, 160, 4)] == list(range(97, 115))
    assert seen[(38, 4, 160, 4)] == list(range(129, 151))


def test_every_threshold_class_meets_every_lane_width_and_overhang():
    met = set()
    for k, cell in enumerate(S.CELLS):
        met.add(("lb", cell[0], S.BASEQ_CLASSES[k % 3]))
        met.add(("ov", cell[1], S.BASEQ_CLASSES[k % 3]))
    assert len(met) == 2 * 3 + 2 * 3


@pytest.mark.parametrize("cell,max_len", [pytest.param(c, l, id=S._cell_id(c, l)) for c in S.CELLS for l in c[4]])
def test_border_batches_hold_their_conditions(cell, max_len):
    lane_bases, overhang, chunk_tiles, lanes, _ = cell
    table, soa, reads = S.border_batch_of(lane_bases, max_len, overhang)
    assert table.n_sites < 46000 and 4000 < len(reads) < 5000
    for k in range(len(table.length)):      # position-sorted inside every contig: the batch may run in chunks
        lo, hi = int(table.read_begin[k]), int(table.read_begin[k + 1])
        assert all(reads[i]["pos"] <= reads[i + 1]["pos"] for i in range(lo, hi - 1))
    assert all(H.cigar_span(r["cigar"]) <= overhang for r in reads) or chunk_tiles == 1
    walked = sum(1 for r in reads if len(r["cigar"]) > 4 or r["pos"] < 0 or r["cigar"][0][0] == 5)
    assert 0 < walked <= len(reads) // 8
    for baseq in (0,) + S.BASEQ_CLASSES:
        st, er, oc, _, os_ = c_oracle.pileup(S.border_thresholds(baseq), table, soa)
        assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
        H.border_conditions(reads, lane_bases, max_len, oc, os_)
