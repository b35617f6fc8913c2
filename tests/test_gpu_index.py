"""The index pass of the direct path (index_direct.hip: direct_facts_kernel once per batch, direct_ranges_kernel and
direct_outliers_kernel every pass; batch_direct.hip: what the host derives from the facts), looked at directly: every tile's
[tbegin, tend), the summed facts, the outlier list, tile_flag, chunk_ok and the batch's direct_* numbers come down through
midas_snps_batch_fetch_index and must equal tests/index_model.py word for word -- integers, no tolerance.

tend must be EXACT (a continuing tile of a chunk starts its stream at tend[t - 1]: one read too low tallies a read twice, one too
high drops it) and tbegin must be MINIMAL (a wide range costs time and no count: no parity test can see it), so every case is
aimed at a border of the pass: the 2048 reads of a workgroup, a contig change on and around that border, empty contigs there,
positions on tile borders and off the contig, position drops that do and do not make a batch unsorted, the two overhangs, reads
that span more than the overhang.  Every case asks three times -- both parities, and again behind a run -- and holds the batch's
counts to the C oracle, so that a wrong model cannot agree with a wrong kernel unnoticed."""
import numpy as np
import pytest

from midas_amd import abi
from oracle import c_oracle
from tests import helpers as H
from tests import index_model as M

pytestmark = pytest.mark.gpu

TILE = 2048
THR = abi.Thresholds.from_args(dict(abi.DEFAULT_ARGS, mapid=50.0, aln_cov=0.0))


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def R(pos, l=100, cigar=None, nm=0):
    return dict(pos=int(pos), l=int(l), cigar=cigar or [(0, int(l))], nm=nm)


def N(pos, span):
    """A two-base read that spans `span` sites: 1M (span - 2)N 1M."""
    return R(pos, 2, [(0, 1), (3, span - 2), (0, 1)])


def spread(rng, n, length, lo=30, hi=150):
    """n reads of lo..hi bases at sorted random starts on the whole contig."""
    return [R(p, rng.integers(lo, hi + 1)) for p in np.sort(rng.integers(0, length, n))]


def batch_of(lengths, reads_per_contig, seed=0):
    """-> (ContigTable, ReadsSoA) from one list of reads per contig, in the order given."""
    rng = np.random.default_rng(seed)
    reads = [r for rs in reads_per_contig for r in rs]
    begin = np.concatenate([[0], np.cumsum([len(rs) for rs in reads_per_contig])]).astype(np.int64)
    l = np.array([r["l"] for r in reads], np.int64)
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    seq_off = off((l + 1) // 2)
    codes = np.array([1, 2, 4, 8], np.uint8)
    seq4 = (codes[rng.integers(0, 4, int(seq_off[-1]))] << 4) | codes[rng.integers(0, 4, int(seq_off[-1]))]
    seq4[seq_off[1:][(l & 1) == 1] - 1] &= 0xF0                                     # (BAM pads an odd read's last byte with 0)
    soa = abi.ReadsSoA(pos=np.array([r["pos"] for r in reads], np.int32), mapq=np.full(len(reads), 42, np.uint8),
                       flag=np.zeros(len(reads), np.uint16), nm=np.array([r["nm"] for r in reads], np.int32), l_seq=l.astype(np.int32),
                       seq_off=seq_off, qual_off=off(l), cigar_off=off([len(r["cigar"]) for r in reads]), seq4=seq4,
                       qual=rng.choice(np.array([40, 35, 31, 29], np.uint8), int(l.sum())),
                       cigar=np.array([(n << 4) | op for r in reads for op, n in r["cigar"]], np.uint32))
    ref = rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), int(sum(lengths)))
    table = abi.ContigTable(length=lengths, species=[k % 2 for k in range(len(lengths))], read_begin=begin, ref=ref, n_species=2,
                            ids=["c%d" % k for k in range(len(lengths))], species_ids=["s0", "s1"])
    return table, soa


def model_of(table, soa):
    return M.index_model(table.length, table.read_begin, soa.pos, soa.l_seq, M.cigars_of(soa.cigar, soa.cigar_off), soa.nm, soa.mapq)


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def words_equal(b, m, table, when):
    got, info = b.fetch_index(), b.info()
    assert got["facts"] == m["facts"], when
    for k in ("tend", "tbegin", "tile_flag", "chunk_ok"):
        bad = np.nonzero(got[k] != m[k])[0] if got[k].shape == m[k].shape else None
        assert bad is not None and bad.size == 0, "%s: %s differs (device %s, model %s) at %s: device %s model %s" % (
            when, k, got[k].shape, m[k].shape, None if bad is None else bad[:8], None if bad is None else got[k][bad[:8]],
            None if bad is None else m[k][bad[:8]])
    assert sorted(tuple(int(x) for x in o) for o in got["outliers"]) == m["outliers"], when
    f = m["facts"]
    assert (info.n_tiles, info.direct_general_reads, info.direct_reach, info.direct_stream_reads, info.direct_max_tile_reads,
            info.direct_chunk_tiles, info.direct_overhang, info.algorithmic_bytes) == (
        m["n_tiles"], f["n_general"], f["direct_reach"], m["stream_reads"], m["max_tile_reads"], m["chunk_tiles"], m["info_overhang"],
        f["alg"] + 17 * table.n_sites), when
    return got


def check(ctx, table, soa, reads=None):
    """The batch over (table, soa) -- or over `reads`, the same records resident -- against the model and the oracle."""
    m = model_of(table, soa)
    st, er, oc, oa, os_ = c_oracle.pileup(THR, table, soa)
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    b = ctx.batch(table, soa if reads is None else reads)
    try:
        if b.info().path != abi.PATH_DIRECT:
            b.select_path(abi.PATH_DIRECT)
        words_equal(b, m, table, "first pass")
        words_equal(b, m, table, "other parity")
        b.run(THR)
        counts, allele, stats = b.fetch()
        bad = np.nonzero((counts != oc).any(axis=1))[0]
        assert bad.size == 0, "counts differ at %d sites, first %s: hip %s oracle %s" % (
            bad.size, bad[:5], counts[bad[:5]].tolist(), oc[bad[:5]].tolist())
        np.testing.assert_array_equal(allele, oa)
        np.testing.assert_array_equal(stats, os_)
        got = words_equal(b, m, table, "behind a run")
    finally:
        b.close()
    return m, got


# ---- the workgroup's run of 2048 reads ----------------------------------------------------------------------------------------------
SIX_TILES = 6 * TILE - 5


@pytest.mark.parametrize("n_reads", [1, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_one_contig_around_the_workgroup_run(ctx, n_reads):
    rng = np.random.default_rng(n_reads)
    m, _ = check(ctx, *batch_of([SIX_TILES], [spread(rng, n_reads, SIX_TILES)], seed=n_reads))
    assert m["facts"]["unsorted"] == 0 and m["facts"]["direct_chunks"] == 1 and m["n_tiles"] == 6


def contig_change(first, n_empty, seed):
    """A contig of `first` reads, n_empty read-less contigs, a contig of 300 reads whose first is read `first`, a contig with one read."""
    rng = np.random.default_rng(seed)
    one = n_empty < 3                            # (two to five contigs)
    lengths = [9000] + [3000] * n_empty + [7000] + [TILE] * one
    a = spread(rng, first, 9000)
    a[-1] = R(8999, 60)                          # the last read of the run's contig starts on its last site ...
    b = spread(rng, 300, 7000)
    b[0] = R(0, 60)                              # ... and the first of the next one on its first: a drop across the border alone
    return batch_of(lengths, [a] + [[]] * n_empty + [b] + [[R(TILE - 1, 31)]] * one, seed=seed)


@pytest.mark.parametrize("n_empty", [0, 1, 3])
@pytest.mark.parametrize("first", [2047, 2048, 2049, 4096])
def test_a_contig_change_against_the_workgroup_run(ctx, first, n_empty):
    table, soa = contig_change(first, n_empty, 100 * first + n_empty)
    m, _ = check(ctx, table, soa)
    assert m["facts"]["unsorted"] == 0 and m["facts"]["direct_chunks"] == 1      # the drop across the border is no disorder
    t0 = m["tile_base"][1 + n_empty]
    assert m["tend"][m["tile_base"][1] - 1] == first and m["tbegin"][t0] == first      # the border lies where the case wants it


def test_empty_contigs_in_front_and_behind_and_the_smallest_contigs(ctx):
    rng = np.random.default_rng(5)
    lengths = [500, 1, 2047, 2048, 2049, 5000, 300, 400]
    reads = [[], [R(0, 30), R(0, 40), R(0, 31)], spread(rng, 50, 2047), spread(rng, 50, 2048), spread(rng, 50, 2049), [R(4000, 90)], [], []]
    m, _ = check(ctx, *batch_of(lengths, reads, seed=5))
    assert m["n_tiles"] == 1 + 1 + 1 + 1 + 2 + 3 + 1 + 1
    assert (m["tbegin"][0], m["tend"][0]) == (M.NONE, 0) and (m["tbegin"][-1], m["tend"][-1]) == (M.NONE, 0)


# ---- positions ------------------------------------------------------------------------------------------------------------------------
def test_positions_on_the_borders_of_tiles_and_contigs(ctx):
    """The batch's reach is 150 (its longest read, all of it aligned): starts of 2048 k - 151 and 2048 k - 150 put start + reach
    on the last site of a tile and on the first of the next."""
    rng = np.random.default_rng(7)
    L = 5 * TILE + 100
    edges = [R(-1, 40), R(-1, 150), R(0, 50), R(2047, 33), R(2047, 150), R(2048, 150), R(2 * TILE - 151, 100), R(2 * TILE - 150, 100),
             R(3 * TILE - 151, 30), R(3 * TILE - 150, 30), R(L - 1, 75), R(L, 75), R(L + 4000, 75)]
    far = [R(100, 120), R(40 * TILE + 100, 120)]                       # 40 tiles apart: one thread fills every tile in between
    one_tile = [R(p, 100) for p in np.sort(rng.integers(TILE, 2 * TILE - 200, 300))]
    first_tile_only = [R(p, 100) for p in np.sort(rng.integers(0, TILE, 40))]
    wide = [R(5, 100), R(299 * TILE + 1, 100)]                         # more tiles than a workgroup has threads
    m, _ = check(ctx, *batch_of([L, 45 * TILE, 3 * TILE, 6 * TILE, 300 * TILE], [edges, far, one_tile, first_tile_only, wide], seed=7))
    f = m["facts"]
    assert (f["direct_reach"], f["direct_reach_ranges"], f["unsorted"], f["n_general"]) == (150, 150, 0, 4)      # (the four starts off the contig)
    assert m["tbegin"][:6].tolist() == [0, 3, 7, 9, 10, 10] and m["tend"][:6].tolist() == [5, 8, 10, 10, 10, 13]
    t1 = m["tile_base"][1]
    assert m["tend"][t1:t1 + 45].tolist() == [14] * 40 + [15] * 5 and m["tbegin"][t1:t1 + 42].tolist() == [13] + [14] * 40 + [M.NONE]
    t3 = m["tile_base"][3]
    assert m["tend"][t3:t3 + 6].tolist() == [355] * 6 and m["tbegin"][t3] == 315 and m["tbegin"][t3 + 2] == M.NONE      # the fill reaches tile_end
    assert m["tend"][t3 + 6:].tolist() == [356] * 299 + [357] and m["tbegin"][t3 + 6:].tolist() == [355] + [356] * 299


# ---- sortedness --------------------------------------------------------------------------------------------------------------------------
def _sorted_case(kind):
    rng = np.random.default_rng(11)
    L = SIX_TILES
    if kind == "drop_across_a_border":
        return [L, L], [[R(p, 100) for p in range(6000, 12000, 20)], [R(p, 100) for p in range(0, 6000, 20)]], 0
    if kind == "zero_then_minus_one":
        return [L], [[R(0, 100), R(-1, 100)] + spread(rng, 200, L)], 0
    if kind == "swapped_pair":
        rs = spread(rng, 500, L)
        rs[250], rs[251] = R(6001, 100), R(6000, 100)
        return [L], [rs], 1
    if kind == "swapped_pair_across_the_run":
        rs = [R(p, 100) for p in np.linspace(0, L - 1, 3000).astype(int)]
        rs[2047], rs[2048] = rs[2048], rs[2047]
        assert rs[2047]["pos"] > rs[2048]["pos"]
        return [L], [rs], 1
    # shuffled in pieces of 100 reads: runs of equal tile keys that cross lanes 63 | 0 and the steps of 256 reads
    rs = spread(rng, 3000, L) + [N(3 * TILE + 7, 3002)]                 # (unsorted: an outlier is not listed, the reach is the full one)
    pieces = [rs[k:k + 100] for k in range(0, 3001, 100)]
    return [L], [[r for k in rng.permutation(len(pieces)) for r in pieces[k]]], 1


@pytest.mark.parametrize("kind", ["drop_across_a_border", "zero_then_minus_one", "swapped_pair", "swapped_pair_across_the_run",
                                  "shuffled_in_pieces"])
def test_sortedness(ctx, kind):
    lengths, reads, unsorted = _sorted_case(kind)
    m, _ = check(ctx, *batch_of(lengths, reads, seed=11))
    assert (m["facts"]["unsorted"], m["facts"]["direct_chunks"], m["chunk_tiles"]) == (unsorted, 1 - unsorted, 1 if unsorted else 4)


# ---- the overhang ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_l", [160, 161, 288, 289])
def test_the_overhang_follows_the_longest_read(ctx, max_l):
    rng = np.random.default_rng(max_l)
    rs = spread(rng, 400, SIX_TILES)
    rs[200] = R(rs[200]["pos"], max_l)
    m, got = check(ctx, *batch_of([SIX_TILES], [rs], seed=max_l))
    assert (m["info_overhang"], m["chunk_tiles"]) == H.direct_overhang_shape(max_l)
    assert got["facts"]["direct_overhang"] == (288 if 160 < max_l <= 288 else 160) and got["facts"]["n_outliers"] == (max_l == 289)


# ---- reads that span more than the overhang ---------------------------------------------------------------------------------------------------
TWENTY = 20 * TILE          # 20 tiles: the first 16 in chunks of four, the last four (the tail eighth, rounded to chunks) one by one


def _with(rng, outliers):
    rs = spread(rng, 500, TWENTY) + outliers
    rs.sort(key=lambda r: min(max(r["pos"], 0), TWENTY - 1))
    return rs


def test_one_long_skip_is_listed_and_the_common_reach_kept(ctx):
    rs = _with(np.random.default_rng(21), [N(5 * TILE + 100, 3002)])
    m, got = check(ctx, *batch_of([TWENTY], [rs], seed=21))
    f = got["facts"]
    assert (f["n_outliers"], f["n_outliers_listed"], f["direct_chunks"], f["direct_reach"], f["max_span"]) == (1, 1, 1, 3002, 3002)
    assert f["direct_reach_ranges"] == f["max_l"] == f["max_common"] <= 150
    assert [tuple(o[1:]) for o in got["outliers"].tolist()] == [(6, 6)]
    assert got["tile_flag"].tolist() == [0] * 5 + [1, 1] + [0] * 13 and got["chunk_ok"].tolist() == [1, 0, 1, 1]


def test_the_border_of_the_tile_flag(ctx):
    """From a tile's first site a span of 2048 + 160 ends on the last site of the next tile's overhang: the flag rises one site on."""
    spans = [161, 2048 + 160 - 1, 2048 + 160, 2048 + 160 + 1]
    rs = _with(np.random.default_rng(22), [N(4 * k * TILE, s) for k, s in enumerate(spans)])
    m, got = check(ctx, *batch_of([TWENTY], [rs], seed=22))
    assert got["facts"]["n_outliers"] == 4 and got["facts"]["n_outliers_listed"] == 3           # (161 sites stay inside the tile)
    assert got["tile_flag"].tolist() == [0] * 12 + [1, 1] + [0] * 6 and got["chunk_ok"].tolist() == [1, 1, 1, 0]


def test_outliers_off_the_contig_and_in_the_tail(ctx):
    outliers = [N(-5000, 3000),                     # wholly in front of the contig: reaches nothing
                N(-100, 2400),                      # begins in front of it: sites 0 .. 2299
                N(17 * TILE + 5, 3000),             # in the tail eighth: flagged, but no chunk's word
                N(TWENTY - TILE - 10, 3000)]        # over the contig's end
    rs = _with(np.random.default_rng(23), outliers)
    m, got = check(ctx, *batch_of([TWENTY], [rs], seed=23))
    assert got["facts"]["n_outliers"] == 4 and sorted(tuple(o[1:]) for o in got["outliers"].tolist()) == [(1, 1), (18, 18), (19, 19)]
    assert got["tile_flag"].tolist() == [1, 1] + [0] * 15 + [1, 1, 1] and got["chunk_ok"].tolist() == [0, 1, 1, 1]


@pytest.mark.parametrize("n_listed", [4096, 4097])
def test_the_outlier_list_overflows(ctx, n_listed):
    """5000 reads have a list of 4096: with one more listed read the batch gives up its chunks and takes the full reach."""
    rng = np.random.default_rng(n_listed)
    L = 10 * TILE
    rs = spread(rng, 5000 - n_listed, L) + [N(p, 2102) for p in rng.integers(0, L - 2200, n_listed)]      # (2102 sites cross a border)
    rs.sort(key=lambda r: r["pos"])
    m, got = check(ctx, *batch_of([L], [rs], seed=n_listed))
    f, over = got["facts"], n_listed > 4096
    assert (f["n_outliers"], f["outlier_cap"], f["direct_chunks"], m["chunk_tiles"]) == (n_listed, 4096, 0 if over else 1, 1 if over else 4)
    assert f["direct_reach"] == 2102 and f["direct_reach_ranges"] == (2102 if over else f["max_l"])
    assert len(got["outliers"]) == (0 if over else 4096) and got["chunk_ok"].size == (0 if over else 2)


# ---- small random batches: the generator of the model's own brute-force test ------------------------------------------------------------------
@pytest.mark.parametrize("block", range(3))
def test_random_small_batches(ctx, block):
    """Sorted and shuffled, with and without outliers, long reads, empty contigs, starts off the contig: 16 batches a case."""
    from tests.test_index_model_host import random_batch
    seen = set()
    for seed in range(1000 + 16 * block, 1016 + 16 * block):
        length, begin, pos, l_seq, cigars, nm = random_batch(seed, oracle_ok=True)
        if not pos:
            continue
        reads = [[R(pos[i], l_seq[i], cigars[i], nm[i]) for i in range(begin[c], begin[c + 1])] for c in range(len(length))]
        m, _ = check(ctx, *batch_of(length, reads, seed=seed))
        seen.add((m["facts"]["unsorted"], m["facts"]["direct_chunks"], m["facts"]["direct_overhang"], m["facts"]["n_outliers_listed"] > 0))
    assert len(seen) >= 4, seen


# ---- a resident batch: the facts pass reads the CIGARs in the payload ------------------------------------------------------------------------
def test_a_resident_batch_has_the_same_words(ctx, tmp_path):
    table, soa = contig_change(2048, 1, 31)
    path = str(tmp_path / "index.bam")
    refid = np.repeat(np.arange(table.n_contigs, dtype=np.int32), np.diff(table.read_begin))
    abi.write_bam(path, table.ids, [int(x) for x in table.length], refid, soa)
    _, _, refid_r, res = abi.read_bam(path, ctx, resident=True)
    assert isinstance(res, abi.ResidentReads) and res.n_reads == soa.n_reads
    np.testing.assert_array_equal(refid, refid_r)
    _, got_resident = check(ctx, table, soa, reads=res)
    _, got_columns = check(ctx, table, soa)
    assert got_resident["facts"] == got_columns["facts"]
    for k in ("tbegin", "tend", "tile_flag", "chunk_ok"):
        np.testing.assert_array_equal(got_resident[k], got_columns[k])


# ---- what the aid refuses, and the facts' status ------------------------------------------------------------------------------------------------
def test_reads_without_nm_or_off_the_contig_are_walked(ctx):
    """n_general counts what the kernel walks op by op: a read without NM is one (and raises in the run, as in the oracle)."""
    rs = spread(np.random.default_rng(41), 300, SIX_TILES)
    rs[7]["nm"] = rs[290]["nm"] = -1
    rs[100] = R(rs[100]["pos"], 60, [(5, 3), (0, 60)])                  # a hard clip: walked
    table, soa = batch_of([SIX_TILES], [rs], seed=41)
    m = model_of(table, soa)
    assert m["facts"]["n_general"] == 3
    st, er, *_ = c_oracle.pileup(THR, table, soa)
    assert (st, er) == (abi.ERR_READ_NO_NM, 7)
    b = ctx.batch(table, soa)
    try:
        words_equal(b, m, table, "first pass")
        b.run(THR)
        with pytest.raises(abi.MidasSnpsError) as ei:
            b.fetch()
        assert (ei.value.status, ei.value.read_index) == (st, er)
        words_equal(b, m, table, "behind a run that raised")
    finally:
        b.close()


def test_a_batch_on_the_long_path_has_no_index(ctx):
    table, soa = batch_of([SIX_TILES], [[R(10, 100), R(500, 1025), R(900, 100)]])
    b = ctx.batch(table, soa)
    try:
        assert b.info().path == abi.PATH_LONG
        with pytest.raises(abi.MidasSnpsError) as ei:
            b.fetch_index()
        assert ei.value.status == abi.ERR_UNSUPPORTED
    finally:
        b.close()
    lib = abi.load_library()
    assert lib.midas_snps_batch_fetch_index(None, None, None, None, None, None, None, None) == abi.ERR_INVALID_ARG


def test_the_lowest_malformed_read_is_reported(ctx):
    """Reads 300 and 2050 -- two workgroups, two fact slots -- both have a QUAL extent one byte short: the lower one is named."""
    table, soa = batch_of([SIX_TILES], [spread(np.random.default_rng(51), 3000, SIX_TILES)], seed=51)
    short = np.zeros(soa.n_reads, np.int64)
    short[[300, 2050]] = 1
    qual_off = np.concatenate([[0], np.cumsum(soa.l_seq.astype(np.int64) - short)]).astype(np.int64)
    bad = abi.ReadsSoA(**{**soa.as_dict(), "qual_off": qual_off, "qual": soa.qual[:int(qual_off[-1])]})
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.batch(table, bad)
    assert (ei.value.status, ei.value.read_index) == (abi.ERR_BAD_LAYOUT, 300)
