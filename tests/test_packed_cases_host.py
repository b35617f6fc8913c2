"""The inputs of tests/test_gpu_packed_borders.py, checked without a device: every batch of tests/packed_cases.py is what it claims to
be, for a grid of 1024 workgroups (an MI355X: 256 compute units) and for a small one.  The packer's host mirror says which records
a tile's stream holds and how many reads it sees, the C oracle what is counted; the conditions (packed_cases.*_conditions) fail when
a builder is changed so that one of the borders it is aimed at disappears."""
import pytest

from tests import packed_cases as P


def test_the_lane_rule_gives_the_lane_counts():
    assert [P.packed_lane_shape(l) for l in (30, 90, 150, 240, 250, 125, 31, 32)] == \
        [(31, 1), (31, 3), (31, 5), (31, 8), (31, 9), (32, 4), (31, 1), (32, 1)]
    assert {k: P.packed_lane_shape(l)[1] for k, l in P.READ_LEN.items()} == {k: k for k in P.READ_LEN}
    assert sorted(P.READ_LEN) == [1, 3, 4, 5, 8] and P.packed_lane_shape(P.READ_LEN[4])[0] == 32      # (the others: lanes of 31 bases)
    # 3 and 5 lanes leave lanes of a wave unused
    assert [64 - k * (64 // k) for k in (1, 3, 4, 5, 8)] == [0, 1, 0, 4, 0]


def test_the_stream_order_deals_the_phases_round_robin():
    # first sites 8, 16, 24 (phase 0), 9 (phase 1), 15 (phase 7): ranks 0 of phases 0, 1, 7, then ranks 1 and 2 of phase 0
    assert P.stream_order([8, 9, 15, 16, 24]) == [0, 1, 2, 3, 4]
    assert P.stream_order([8, 16, 24, 9, 15]) == [0, 3, 4, 1, 2]


@pytest.mark.parametrize("grid", P.HOST_GRIDS)
@pytest.mark.parametrize("lanes", sorted(P.READ_LEN))
def test_stream_batches_hold_every_probe(lanes, grid):
    table, soa, facts = P.stream_batch(lanes, grid)
    assert facts["lanes"] == lanes and facts["max_len"] == P.READ_LEN[lanes]
    # the probes, written out: (class-0 records, records reaching in, other records that start in the tile)
    rpw = {1: 64, 3: 21, 4: 16, 5: 12, 8: 8}[lanes]
    step = 4 * rpw
    want = [(ns, 0, 0) for ns in (0, 1, rpw - 1, rpw, rpw + 1, step - 1, step, step + 1, 2 * step, 2 * step + 1, 3 * step + 1)]
    want += [(ns, ni, ng) for ns in (rpw - 1, rpw, step, step + 1) for ni, ng in ((1, 0), (0, 1), (1, 1))]
    want += [(0, 1, 0), (0, 0, 1), (0, rpw + 1, 0), (0, 0, step + 1)]
    want += [(2 * step + rpw, 0, 1), (2 * step + 3, 1, 0)]           # (beyond the list: long tiles that end on the general path)
    assert (facts["rpw"], facts["step"]) == (rpw, step) and len(set(want)) == 29
    for row in range(3):      # every probe in every row of `grid` tiles
        assert sorted(c["probe"] for c in facts["tiles"][row * grid:(row + 1) * grid] if c["kind"] == "probe") == sorted(want)
    assert len(facts["reads"]) < 40000
    P.stream_conditions(table, soa, facts)


@pytest.mark.parametrize("grid", P.HOST_GRIDS)
def test_handout_batches_show_a_tile_taken_twice_or_never(grid):
    counts = P.handout_counts(grid)
    assert counts == [grid - 1, grid, grid + 1, 2 * grid, 2 * grid + 1, 2 * grid + 7, 2 * grid + 8, 2 * grid + 9, 3 * grid + 5]
    for n_tiles in counts:
        table, soa, facts = P.handout_batch(n_tiles)
        assert facts["n_tiles"] == n_tiles == len(table.length) and table.n_species == -(-n_tiles // 5)
        P.handout_conditions(table, soa, facts)


@pytest.mark.parametrize("grid", P.HOST_GRIDS)
@pytest.mark.parametrize("lanes", [1, 5])
def test_split_batches_sit_on_the_split_rule(lanes, grid):
    table, soa, facts = P.split_batch(lanes, grid)
    assert facts["lanes"] == lanes and facts["max_len"] == P.READ_LEN[lanes]
    P.split_conditions(table, soa, facts)


def test_the_split_rule_in_python_is_the_one_of_work_plan_h():
    # tests/cpp/work_plan_check.cpp pins the C++; these are its corner values
    assert P.planned_items([2048, 2049, 5000, 1], 1024) == (9, [1, 3, 5, 1])
    assert P.planned_items([4096] * 1024, 1024) == (4097, [1] * 1024)          # 2 * fair above every tile: none is split
    assert P.planned_items([10000] + [100] * 99, 8)[1][0] == 5                 # fair 2488: 10000 reads in parts of 2488


@pytest.mark.parametrize("shuffled", [False, True])
def test_far_batch_reaches_30_tiles_and_more(shuffled):
    table, soa, facts = P.far_batch(shuffled)
    for k in range(len(table.length)):
        pos = [r["pos"] for r in facts["reads"][facts["read_begin"][k]:facts["read_begin"][k + 1]]]
        assert (pos == sorted(pos)) != shuffled
    P.far_conditions(table, soa, facts)


@pytest.mark.parametrize("case", P.REFUSED_CASES, ids=["+".join("%s:%s" % x for x in c).replace(" ", "_") for c in P.REFUSED_CASES])
def test_refused_batches_are_refused_at_the_intended_read(case):
    table, soa, facts = P.refused_batch(case)
    first = P.refused_conditions(table, soa, facts)
    assert first[1] in case
    # every place of the stream and every kind of refusal occurs
    assert set(x for c in P.REFUSED_CASES for x in c) == set([(p, "no_qual") for p in ("S first", "S last fast", "S tail")] +
                                                             [(p, k) for p in "IG" for k in ("no_nm", "no_qual", "overrun")])
