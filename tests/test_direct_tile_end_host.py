"""The inputs of tests/test_gpu_direct_tile_end.py, checked without a device: the contig sets hold every length the cases are
about within ten tiles, the read lengths select the lane shapes the cases name, and for every batch what keeps its case from
passing empty -- the oracle accepts it and keeps at least half of its reads, every tile has depth on its first site, its last
site and in each of its rows of 256 sites, a read starts on every full tile's last site and one ends on the next tile's first."""
import pytest

from oracle import c_oracle
from tests import helpers as H
from tests import test_gpu_direct_tile_end as T


def test_the_contig_sets_hold_every_length_and_the_species_border():
    seen = set(n for lengths, _ in T.CONTIG_SETS.values() for n in lengths)
    assert seen >= {2047, 2048, 2049, 4096, 4097, 2048 + 100, 100, 8192 + 3}
    for lengths, species in T.CONTIG_SETS.values():
        assert len(T.tiles_of(lengths)) <= 10 and len(species) == len(lengths)
    lengths, species = T.CONTIG_SETS["short"]      # tiles 0 and 1: full, of one chunk of four, of two species
    assert lengths[:2] == [T.TILE, T.TILE] and species[0] != species[1]
    lengths, _ = T.CONTIG_SETS["long"]             # a chunk of four full tiles, then one whose length is no multiple of 4
    assert [t[2] for t in T.tiles_of(lengths)[:5]] == [T.TILE] * 4 + [3]


def test_the_read_lengths_select_the_lane_shapes():
    assert [H.direct_lane_shape(l) for l in T.READ_LENGTHS] == [(38, 4), (32, 5), (38, 3), (30, 2), (30, 1)]
    assert all(H.direct_overhang_shape(l) == (H.OVERHANG, 4) for l in T.READ_LENGTHS)


@pytest.mark.parametrize("length", T.READ_LENGTHS)
@pytest.mark.parametrize("set_name", sorted(T.CONTIG_SETS))
def test_tile_end_batches_hold_their_conditions(set_name, length):
    table, soa, reads, lengths = T.tile_end_batch(set_name, length)
    for k in range(len(lengths)):
        lo, hi = int(table.read_begin[k]), int(table.read_begin[k + 1])
        assert all(reads[i]["pos"] <= reads[i + 1]["pos"] for i in range(lo, hi - 1))
    assert all(H.cigar_span(r["cigar"]) <= H.OVERHANG for r in reads)
    T.border_reads_present(lengths, table, reads, length)
    for baseq in T.BASEQS:
        T.tile_end_conditions(lengths, reads, c_oracle.pileup(T.tile_end_thresholds(baseq), table, soa))


def test_the_flagged_chunk_holds_its_conditions():
    table, soa, reads, lengths = T.tile_end_batch("long", 150, True)
    over = [r for r in reads if H.cigar_span(r["cigar"]) > H.OVERHANG]
    assert len(over) == 1 and over[0]["pos"] // T.TILE == 1 and H.cigar_span(over[0]["cigar"]) == 150 + T.OUTLIER_GAP
    for baseq in T.BASEQS:
        T.tile_end_conditions(lengths, reads, c_oracle.pileup(T.tile_end_thresholds(baseq), table, soa))
