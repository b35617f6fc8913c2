"""Batches aimed at the borders of the packed path (pack_reads.hip -> index_reads.hip -> pileup_tiles.hip, planned by work_plan.h and
batch_packed.hip), and the conditions that keep them from passing for the wrong reason.  Pure numpy / Python; the conditions use
the packer's host mirror (tests/mirror) and the C oracle, never a device.

Every builder takes `grid`, the number of workgroups the pileup kernel is launched with (4 x compute units), and returns
(ContigTable, ReadsSoA, facts): facts["tiles"][t] says what tile t claims to be, facts["reads"] are the reads as dicts in input order.

  stream_batch    A  tiles whose virtual stream S, I, G ends on, before and behind a multiple of a wave's reads, three rows of
                     `grid` tiles, so that tiles t and t + grid are one workgroup's first two items
  handout_batch   B  filler tiles only, a new species every five tiles: the item count relative to the grid
  split_batch     C  tiles that see 2048, 2049 and more reads: whole or cut into parts
  far_batch       D  records that reach 30, 31, 32 and 40 tiles on
  refused_batch   E  a read the oracle refuses at a chosen place of a tile's stream

tests/test_packed_cases_host.py asserts the conditions for grid 1024 and SMALL_GRID; tests/test_gpu_packed_borders.py runs the
batches on the device."""
import functools

import numpy as np

from midas_amd import abi

TILE = 2048
NWAVES = 4                       # waves of the pileup kernel's workgroup
SMALL_GRID = 64                  # the second grid of the host test (a multiple of 8, small enough to read a failure)
HOST_GRIDS = (1024, SMALL_GRID)
OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P = 0, 1, 2, 3, 4, 5, 6
N_CODE = 15
ACGT = np.array([1, 2, 4, 8], np.uint8)
# at, above and below the base thresholds of both runs (30 and 0), and beyond what the layouts keep exactly (50, 62)
QUALS = np.array([0, 1, 12, 29, 30, 31, 40, 41, 50, 63], np.uint8)
FILLER_QUALS = np.array([12, 29, 30, 31, 40, 41], np.uint8)
MAPQS = np.array([42, 42, 42, 35, 30, 19], np.uint8)
# the two runs of every GPU case: the second drops other reads (mapq 30) and keeps what the first dropped (identity 80 .. 94 %,
# an aligned part of 50 .. 75 %), with every A/C/G/T base counted
THRESHOLDS = (dict(abi.DEFAULT_ARGS), dict(abi.DEFAULT_ARGS, baseq=0, mapid=80.0, aln_cov=0.5, mapq=31))
READ_LEN = {1: 30, 3: 90, 4: 128, 5: 150, 8: 240}   # lanes per read -> read length of the batch (four lanes: of 32 bases)


def packed_lane_shape(max_len):
    """(lane_bases, lanes_per_read) of the packed layout for a batch's longest read: layout.h lane_bases_for."""
    n32, n31 = (max_len + 31) // 32, (max_len + 30) // 31
    lb = 32 if n32 < n31 and n32 <= 5 else 31
    return lb, max(1, -(-max_len // lb))


def thresholds(k):
    return abi.Thresholds.from_args(THRESHOLDS[k])


# ---- reads -----------------------------------------------------------------------------------------------------------------------

def _read(pos, cigar, seq, qual, nm=0, mapq=42, tag="plain"):
    return dict(pos=int(pos), cigar=cigar, seq=seq, qual=qual, nm=int(nm), mapq=int(mapq), tag=tag)


class _Draw:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def seqs(self, n, l, n_frac=0.03):
        s = ACGT[self.rng.integers(0, 4, size=(n, l))]
        if n_frac:
            s[self.rng.random((n, l)) < n_frac] = N_CODE
        return s

    def good(self, pos, l, cigar=None, tag="good"):
        """Kept by both runs, every base counted by both."""
        return _read(pos, cigar or [(OP_M, l)], self.seqs(1, l, 0)[0], np.full(l, 40, np.uint8), tag=tag)

    def noisy(self, positions, l, tag="noisy", quals=QUALS):
        """One read of l bases per position: one match op, or (one in ten of 20 bases and more) a soft clip at either end; mapq,
        NM and qualities on both sides of both runs' thresholds."""
        n = len(positions)
        seqs, qs = self.seqs(n, l), quals[self.rng.integers(0, quals.size, size=(n, l))]
        mapq = MAPQS[self.rng.integers(0, MAPQS.size, n)]
        nmk, u = self.rng.integers(0, 4, n), self.rng.random(n)
        out = []
        for k, pos in enumerate(positions):
            cigar = [(OP_M, l)]
            if l >= 20 and u[k] < 0.1:
                s = 1 + int(u[k] * 10 * (l // 3))               # up to a third: below aln_cov 0.75 now and then, never below 0.5
                cigar = [(OP_S, s), (OP_M, l - s)] if k & 1 else [(OP_M, l - s), (OP_S, s)]
            out.append(_read(pos, cigar, seqs[k], qs[k], (0, 0, 1, l // 12 + 1)[nmk[k]], mapq[k], tag))
        return out

    def kept_cigar(self, pos, l, k, good=False, tag="general"):
        """A read that keeps its CIGAR in the packed layout (plan_read refuses it): a pad op between two matches (k even), or a
        hard clip behind the leading soft clip (k odd; the clip loops of kRecClipGeneric).  Its aligned bases start at pos."""
        if k & 1:
            cigar = [(OP_S, 2), (OP_H, 3), (OP_M, l - 2)]
        else:
            a = 1 + (7 * k) % (l - 1)
            cigar = [(OP_M, a), (OP_P, 1 + k % 3), (OP_M, l - a)]
        r = self.good(pos, l, cigar, tag) if good else self.noisy([pos], l, tag)[0]
        r["cigar"] = cigar
        return r


def stream_order(positions):
    """Order of a tile's class-0 records in the device layout, from their first sites in input order: sorted by (first site mod 8,
    input order), then dealt round-robin over those eight phases (pack_reads.hip pack_dest_kernel)."""
    rank, seen = [], {}
    for p in positions:
        ph = p & 7
        rank.append((seen.get(ph, 0), ph))
        seen[ph] = seen.get(ph, 0) + 1
    return sorted(range(len(positions)), key=lambda i: rank[i])


def soa_of(reads):
    l_seq = np.array([r["seq"].size for r in reads], dtype=np.int32)
    seq4, cigar = [], []
    for r in reads:
        c = r["seq"]
        if c.size & 1:
            c = np.append(c, np.uint8(0))
        seq4.append((c[0::2] << 4) | c[1::2])
        cigar += [(ln << 4) | op for op, ln in r["cigar"]]
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    cat = lambda parts: np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)
    return abi.ReadsSoA(pos=np.array([r["pos"] for r in reads], dtype=np.int32), mapq=np.array([r["mapq"] for r in reads], dtype=np.uint8),
                        flag=np.zeros(len(reads), dtype=np.uint16), nm=np.array([r["nm"] for r in reads], dtype=np.int32), l_seq=l_seq,
                        seq_off=off([s.size for s in seq4]), qual_off=off(l_seq), cigar_off=off([len(r["cigar"]) for r in reads]),
                        seq4=cat(seq4), qual=cat([r["qual"] for r in reads]), cigar=np.array(cigar, dtype=np.uint32))


# ---- units: one contig each -------------------------------------------------------------------------------------------------------

def _unit(length, reads, tiles, species=None, sort=True):
    assert len(tiles) == -(-length // TILE)
    if sort:
        reads = sorted(reads, key=lambda r: r["pos"])         # (stable)
    return dict(length=length, reads=reads, tiles=tiles, species=species)


def filler_unit(d, n_sites, n_reads, hang=None):
    """A tile that is its own contig of 1 to 7 sites: a good read over all of it, then reads of 1 to 7 bases that may hang over
    its end; hang: the length of a full-size read that may take the second read's place."""
    reads = [d.good(0, n_sites)]
    for _ in range(n_reads - 1):
        l = int(d.rng.integers(1, 8))
        if hang and d.rng.random() < 0.3:
            l = hang
        reads += d.noisy([int(d.rng.integers(0, n_sites))], l, "filler", FILLER_QUALS)
    return _unit(n_sites, reads, [dict(kind="filler", ns=n_reads, ni=0, ng=0, sees=n_reads)])


def assemble(units, facts):
    """-> (ContigTable, ReadsSoA, facts).  A unit's species is a key; the keys are numbered in order of appearance.  The reference
    has lower case and N; a filler's last letter is lower case."""
    rng = np.random.default_rng(len(units))
    names, species, begin, reads, tiles, ref = {}, [], [0], [], [], []
    for k, u in enumerate(units):
        species.append(names.setdefault(u["species"], len(names)))
        reads += u["reads"]
        begin.append(len(reads))
        letters = np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, size=u["length"])]
        if u["tiles"][0]["kind"] == "filler":
            letters[-1] = b"acgt"[k & 3]
        ref.append(letters)
        for j, t in enumerate(u["tiles"]):
            tiles.append(dict(t, contig=k, species=species[-1], start=j * TILE, len=min(TILE, u["length"] - j * TILE)))
    table = abi.ContigTable(length=[u["length"] for u in units], species=species, read_begin=begin, ref=np.concatenate(ref),
                            n_species=len(names), ids=["c%d" % k for k in range(len(units))], species_ids=["s%d" % k for k in range(len(names))])
    site_base = np.concatenate([[0], np.cumsum([t["len"] for t in tiles])])
    for t, b in zip(tiles, site_base):
        t["site_base"] = int(b)
    facts = dict(facts, tiles=tiles, reads=reads, read_begin=begin, n_tiles=len(tiles), max_len=max(r["seq"].size for r in reads))
    facts["lane_bases"], facts["lanes"] = packed_lane_shape(facts["max_len"])
    return table, soa_of(reads), facts


def without(table, facts, drop):
    """The batch without the reads whose input-order index is in `drop`."""
    drop = set(int(i) for i in drop)
    keep = [i for i in range(len(facts["reads"])) if i not in drop]
    kept_before = np.concatenate([[0], np.cumsum([0 if i in drop else 1 for i in range(len(facts["reads"]))])])
    t2 = abi.ContigTable(length=table.length, species=table.species, read_begin=kept_before[np.asarray(facts["read_begin"])],
                         ref=table.ref, n_species=table.n_species, ids=table.ids, species_ids=table.species_ids)
    return t2, soa_of([facts["reads"][i] for i in keep])


def tile_table(table, soa):
    """What the packer makes of a batch, from its host mirror's index keys (tile << 7 | reach << 2 | class): per tile the numbers
    of class-0 records (ns), of class-2 records of earlier tiles that reach it (ni), of other records that start in it (ng) and of
    reads it sees (pack_keys_kernel's tile_reads: the records that start in it and those that reach in, a reach counted up to 31);
    per record its tile, class, reach field and read."""
    from tests import mirror
    _, _, orig, key = mirror.pack_reads_tiled(soa, table)
    n_tiles = int(sum(-(-int(n) // TILE) for n in table.length))
    tile, reach, cls = (key >> 7).astype(np.int64), ((key >> 2) & 31).astype(np.int64), (key & 3).astype(np.int64)
    ns = np.bincount(tile[cls == 0], minlength=n_tiles)
    ng = np.bincount(tile[cls != 0], minlength=n_tiles)
    ni = np.zeros(n_tiles + 64, np.int64)
    for t, r in zip(tile[reach > 0], reach[reach > 0]):
        ni[t + 1:t + 1 + r] += 1
    assert not ni[n_tiles:].any()                              # (a reach never leaves its contig)
    ni = ni[:n_tiles]
    return dict(ns=ns, ni=ni, ng=ng, sees=ns + ng + ni, tile=tile, reach=reach, cls=cls, orig=orig.astype(np.int64), n_tiles=n_tiles)


def planned_items(sees, grid):
    """work_plan.h plan_work_items: (fair, [parts per tile]); a tile is one item unless it sees more than max(2048, 2 * fair) reads,
    then it is cut into parts of max(1024, fair)."""
    fair = int(np.sum(sees)) // grid + 1
    split, part = max(2048, 2 * fair), max(1024, fair)
    return fair, [1 if int(s) <= split else min(-(-int(s) // part), 4096) for s in sees]


# ---- A: stream shapes -------------------------------------------------------------------------------------------------------------

def stream_probes(rpw):
    step = NWAVES * rpw
    out = [(ns, 0, 0) for ns in (0, 1, rpw - 1, rpw, rpw + 1, step - 1, step, step + 1, 2 * step, 2 * step + 1, 3 * step + 1)]
    out += [(ns, ni, ng) for ns in (rpw - 1, rpw, step, step + 1) for ni, ng in ((1, 0), (0, 1), (1, 1))]
    out += [(0, 1, 0), (0, 0, 1), (0, rpw + 1, 0), (0, 0, step + 1)]
    out += [(2 * step + rpw, 0, 1), (2 * step + 3, 1, 0)]           # long tiles whose last iterations take the general path
    return out


def probe_unit(d, l, probe):
    """A probe tile with exactly ns class-0 records, ni records reaching in from the tile in front and ng other records that start in
    it.  With ni > 0 the unit is a contig of two tiles, the probe the second.  The first reaching and the first other record, and
    the read behind the last class-0 record of the tile's stream, are good reads: no part of the stream can be skipped unseen."""
    ns, ni, ng = probe
    length = l + 301 + int(d.rng.integers(0, 8)) if ns + ni + ng else 11
    base = TILE if ni else 0
    s_pos = sorted(base + int(p) for p in d.rng.integers(0, length - l + 1, ns))
    s_reads = d.noisy(s_pos, l, "S")
    if ns:
        last = stream_order(s_pos)[-1]
        s_reads[last] = d.good(s_pos[last], l, tag="S")
    reads = list(s_reads)
    for k in range(ng):
        reads.append(d.kept_cigar(base + int(d.rng.integers(0, length - l + 1)), l, k, good=k == 0, tag="G"))
    tiles = [dict(kind="probe", probe=probe, ns=ns, ni=ni, ng=ng, sees=ns + ni + ng)]
    if ni:
        front = [d.good(0, l)] + d.noisy([int(p) for p in d.rng.integers(0, 1500, int(d.rng.integers(0, 3)))], l, "front")
        for k in range(ni):       # (at least one aligned base on either side of the border)
            x = l // 2 if k == 0 else int(d.rng.integers(1, l - 3))
            front.append(d.kept_cigar(TILE - x, l, k, good=k == 0, tag="I"))
        tiles.insert(0, dict(kind="front", ns=len(front) - ni, ni=0, ng=ni, sees=len(front)))
        reads += front
    return _unit(base + length, reads, tiles)


@functools.lru_cache(maxsize=2)
def stream_batch(lanes, grid):
    """Three rows of `grid` tiles; every probe of stream_probes once in every row, at seeded columns, fillers in between.  No tile is
    split, so the item list is the identity and tiles t and t + grid are the first two items of workgroup t."""
    l = READ_LEN[lanes]
    assert packed_lane_shape(l)[1] == lanes
    rpw = 64 // lanes
    step = NWAVES * rpw
    d = _Draw(1000 * lanes + grid)
    probes = stream_probes(rpw)
    long_probes = [p for p in probes if sum(p) >= 2 * step]
    # what row 1 holds behind row 0's long tiles: an empty tile, one record, a long tile, a tile whose stream starts with a record
    # of its I range, one whose stream starts with its G range (row 2's long tiles have no successor)
    successors = [(0, 0, 0), (1, 0, 0), long_probes[0], (0, 1, 0), (0, 0, 1)]
    assert len(long_probes) == len(successors)
    # row 0's long tiles sit in even columns: the tile in front of each stays free for the front tile of a successor of two tiles
    long_cols = [2 + 2 * int(c) for c in d.rng.choice(grid // 2 - 1, len(long_probes), replace=False)]
    units = []
    for row in range(3):
        slots = [None] * grid
        forced = dict(zip(long_probes if row == 0 else successors if row == 1 else [], long_cols))       # probe -> column of its tile
        rest = [p for p in probes if p not in forced]
        for probe in list(forced) + [rest[i] for i in d.rng.permutation(len(rest))]:
            width = 2 if probe[1] else 1
            free = [c for c in range(grid - width + 1) if all(slots[c + j] is None for j in range(width))]
            col = forced[probe] - (width - 1) if probe in forced else free[int(d.rng.integers(0, len(free)))]
            assert all(slots[col + j] is None for j in range(width))
            slots[col] = probe_unit(d, l, probe)
            if width == 2:
                slots[col + 1] = "second tile"
        for col in range(grid):
            if slots[col] is None:
                slots[col] = filler_unit(d, 1 + (col + row) % 7, 1 + int(d.rng.integers(0, 3)), hang=l)
            if isinstance(slots[col], dict):
                # a new species every 37 columns; the blocks of columns take turns in keeping it over the rows
                block = col // 37
                slots[col]["species"] = (block,) if block % 2 == 0 else (block, row)
                units.append(slots[col])
    return assemble(units, dict(group="A", grid=grid, rpw=rpw, step=step, read_len=l))


# ---- B: hand-out --------------------------------------------------------------------------------------------------------------------

def handout_counts(grid):
    return [grid - 1, grid, grid + 1, 2 * grid, 2 * grid + 1, 2 * grid + 7, 2 * grid + 8, 2 * grid + 9, 3 * grid + 5]


@functools.lru_cache(maxsize=2)
def handout_batch(n_tiles):
    """Filler tiles only, a new species every five tiles.  Neighbouring species hold different numbers of reads, so a tile taken twice
    or never shows in its species' counters."""
    d = _Draw(n_tiles)
    units, prev = [], -1
    for first in range(0, n_tiles, 5):
        k = min(5, n_tiles - first)
        total = int(d.rng.choice([t for t in range(k, 3 * k + 1) if t != prev]))
        prev = total
        per = [1] * k
        while sum(per) < total:
            j = int(d.rng.integers(0, k))
            per[j] += 1 if per[j] < 3 else 0
        for j in range(k):
            u = filler_unit(d, 1 + (first + j + first // 5) % 7, per[j])
            u["species"] = first // 5
            units.append(u)
    return assemble(units, dict(group="B"))


# ---- C: split tiles -----------------------------------------------------------------------------------------------------------------

N_HOT = 1100        # reads of a hot tile that start within eight sites: a depth above 255 at either run


def _hot_reads(d, base, l, n, lo, hi, hot_at=50):
    """n reads that start in the tile at contig position base: N_HOT within eight sites of hot_at, the others over [lo, hi]."""
    pos = [base + hot_at + int(p) for p in d.rng.integers(0, 8, min(n, N_HOT))]
    pos += [base + int(p) for p in d.rng.integers(lo, hi + 1, n - len(pos))]
    return d.noisy(pos, l, "hot")


def _split_tile(n, **more):
    return dict(kind="hot", ns=n, ni=0, ng=0, sees=n, **more)


@functools.lru_cache(maxsize=2)
def split_batch(lanes, grid):
    l = READ_LEN[lanes]
    d = _Draw(77 * lanes + grid)
    few = lambda base, n=3, room=TILE: [d.good(base, l)] + d.noisy([base + int(p) for p in d.rng.integers(0, room - l - 1, n - 1)], l, "few")
    plain = lambda positions, tag: [dict(r, cigar=[(OP_M, l)]) for r in d.noisy(positions, l, tag)]
    one = lambda length, n, name: _unit(length, _hot_reads(d, 0, l, n, 58, length - l - 40), [_split_tile(n, name=name)])
    specials = [one(1600, 2048, "2048"), one(TILE, 2049, "2049"), one(2000, 5000, "5000")]
    for tail, name in ((1002, "last+2"), (803, "last+3")):          # a contig's short last tile, 2 and 3 sites beyond a multiple of 4
        assert tail % 4 == int(name[-1])
        specials.append(_unit(TILE + tail, few(0) + _hot_reads(d, TILE, l, 2100, 58, tail - l - 40),
                              [dict(kind="few", ns=3, ni=0, ng=0, sees=3), _split_tile(2100, name=name)]))
    specials.append(_unit(TILE + 1500, _hot_reads(d, 0, l, 2100, 58, TILE - l - 40) + _hot_reads(d, TILE, l, 2300, 58, 1500 - l - 40),
                          [_split_tile(2100, name="adjacent 0"), _split_tile(2300, name="adjacent 1")]))
    # a split tile between two tiles of its contig: records that keep their CIGAR reach in and out (class 2), plain reads over either
    # border are cut into class-0 pieces
    cross = lambda border, k: border - 1 - (k * 7) % (l - 4)
    reads = few(0) + _hot_reads(d, TILE, l, 2200, 300, 1400, hot_at=200) + few(2 * TILE, 2, 700)
    reads += [d.kept_cigar(cross(TILE, k), l, k, good=k == 0, tag="in") for k in range(6)]
    reads += plain([cross(TILE, k) for k in range(6, 11)], "in plain")
    reads += [d.kept_cigar(cross(2 * TILE, k), l, k, good=k == 0, tag="out") for k in range(6)]
    reads += plain([cross(2 * TILE, k) for k in range(6, 11)], "out plain")
    specials.append(_unit(2 * TILE + 700, reads, [
        dict(kind="few", ns=3 + 5, ni=0, ng=6, sees=3 + 5 + 6),
        dict(kind="hot", name="in and out", ns=2200 + 5 + 5, ni=6, ng=6, sees=2200 + 5 + 5 + 6 + 6),
        dict(kind="few", ns=2 + 5, ni=6, ng=0, sees=2 + 5 + 6)]))
    n_fillers = grid + 40 - sum(len(u["tiles"]) for u in specials)
    at = sorted(int(x) for x in d.rng.choice(n_fillers, len(specials), replace=False))
    units = []
    for k in range(n_fillers + 1):
        while at and at[0] == k:
            at.pop(0)
            u = specials[len(specials) - len(at) - 1]
            u["species"] = ("special", len(units))
            units.append(u)
        if k < n_fillers:
            u = filler_unit(d, 1 + k % 7, 1 + int(d.rng.integers(0, 3)), hang=l)
            u["species"] = ("filler", k // 10)
            units.append(u)
    table, soa, facts = assemble(units, dict(group="C", grid=grid, read_len=l))
    facts["fair"], facts["parts"] = planned_items([t["sees"] for t in facts["tiles"]], grid)
    facts["n_work_items"] = sum(facts["parts"])
    return table, soa, facts


# ---- D: far reach -------------------------------------------------------------------------------------------------------------------

FAR_REACH = (30, 31, 32, 40)
FAR_TILES = 45
FAR_A = 75              # matched bases in front of the skip (and behind it: reads of 150 bases)


@functools.lru_cache(maxsize=2)
def far_batch(shuffled):
    """One contig of 45 tiles between two-tile contigs.  Reads of 150 bases with one N or D op reach exactly 30, 31, 32 and 40 tiles
    on, each as a read that keeps its CIGAR (a pad op in front of the skip: ONE record with a reach field) and as a plain one (two
    match segments, cut at the tile borders); facts["far"] lists them.  One read's skip runs past the contig's end."""
    l, d = 2 * FAR_A, _Draw(4545)
    length = FAR_TILES * TILE

    def ordinary(size):       # 22 reads that start in every tile; those of a tile that is not the contig's last may cross into the next
        out = []
        for start in range(0, size, TILE):
            n_sites = min(TILE, size - start)
            room = TILE if start + TILE < size else n_sites - l
            out += [d.good(start + 5, l), d.good(start + n_sites - l - 5, l)] + d.noisy([start + int(p) for p in d.rng.integers(0, room, 20)], l)
        return out
    reads, n = ordinary(length), 0
    for reach in FAR_REACH:
        for place in ("first site", "last site", "ends on a last site", "ends on a first site"):
            for op in (OP_N, OP_D):
                for kept in (True, False):
                    s = n % 5
                    n += 1
                    pos, end = {"first site": (s * TILE, (s + reach) * TILE + 700), "last site": (s * TILE + TILE - 1, (s + reach) * TILE + 300),
                                "ends on a last site": (s * TILE + 400, (s + reach + 1) * TILE - 1),
                                "ends on a first site": (s * TILE + 900, (s + reach) * TILE)}[place]
                    skip = end + 1 - pos - l
                    cigar = [(OP_M, FAR_A)] + ([(OP_P, 1)] if kept else []) + [(op, skip), (OP_M, l - FAR_A)]
                    r = d.good(pos, l, cigar, tag="far")
                    r.update(reach=reach, place=place, kept=kept, behind=pos + FAR_A + skip)
                    assert (end // TILE) - (pos // TILE) == reach and end < length
                    reads.append(r)
    over = d.good(10 * TILE + 77, l, [(OP_M, FAR_A), (OP_P, 1), (OP_N, length), (OP_M, l - FAR_A)], tag="past the end")
    reads.append(over)
    small = lambda k: _unit(TILE + 300 + k, ordinary(TILE + 300 + k) + [d.good(100, l, [(OP_M, FAR_A), (OP_P, 1), (OP_D, 3 * TILE), (OP_M, l - FAR_A)], "past the end")],
                            [dict(kind="small"), dict(kind="small")])
    units = [small(1), small(2), _unit(length, reads, [dict(kind="far")] * FAR_TILES), small(3)]
    for k, u in enumerate(units):
        u["species"] = k % 2
        if shuffled:
            u["reads"] = [u["reads"][i] for i in d.rng.permutation(len(u["reads"]))]
    return assemble(units, dict(group="D", read_len=l))


# ---- E: a refused read in every range of the stream ------------------------------------------------------------------------------------

REFUSED_CASES = ((("S first", "no_qual"),), (("S last fast", "no_qual"),), (("S tail", "no_qual"),),
                 (("I", "no_nm"),), (("I", "no_qual"),), (("I", "overrun"),), (("G", "no_nm"),), (("G", "no_qual"),), (("G", "overrun"),),
                 (("S tail", "no_qual"), ("G", "no_nm")), (("I", "overrun"), ("S first", "no_qual")))
REFUSED_STATUS = {"no_nm": abi.ERR_READ_NO_NM, "no_qual": abi.ERR_READ_NO_QUAL, "overrun": abi.ERR_READ_CIGAR_OVERRUN}


@functools.lru_cache(maxsize=2)
def refused_batch(case):
    """A probe tile (the second tile of its contig, among fillers) with step + 5 class-0 records, two records reaching in and two
    other records, all of good reads but the class-0 ones; the reads at the places of `case` are ones the oracle refuses: without
    NM, without QUAL, or with a match op that runs two bases past SEQ inside the contig.  The place says where the read's record
    sits in the stream: the first class-0 record, the last one of the fast iterations, the last one of all (an iteration on the
    general path), a record reaching in (reported by the tile it starts in), another record.  Only a read without QUAL can be
    refused as a class-0 record: the other two kinds keep their CIGAR."""
    l, lanes = READ_LEN[5], 5
    rpw = 64 // lanes
    step, d = NWAVES * rpw, _Draw(5150)
    ns, length = step + 5, l + 350
    s_pos = sorted(TILE + int(p) for p in d.rng.integers(0, length - l + 1, ns))
    s_reads = d.noisy(s_pos, l, "S")
    order = stream_order(s_pos)
    at = {"S first": order[0], "S last fast": order[step - 1], "S tail": order[ns - 1]}
    others = {"I": [d.kept_cigar(TILE - l // 2 - k, l, 0, good=True, tag="I") for k in range(2)],
              "G": [d.kept_cigar(TILE + 40 + 90 * k, l, 0, good=True, tag="G") for k in range(2)]}
    for place, kind in case:
        if place in at:
            s_reads[at[place]] = r = d.good(s_pos[at[place]], l, tag="S")
        else:
            r = others[place][0]
        if kind == "no_nm":
            r["nm"] = -1
        elif kind == "no_qual":
            r["qual"] = np.full(l, 0xFF, np.uint8)
        else:
            r["cigar"] = r["cigar"][:-1] + [(OP_M, r["cigar"][-1][1] + 2)]
        r["refused"] = (place, kind)
    probe = _unit(TILE + length, [d.good(0, l)] + d.noisy([300, 900], l, "front") + others["I"] + s_reads + others["G"],
                  [dict(kind="front", ns=3, ni=0, ng=2, sees=5), dict(kind="probe", ns=ns, ni=2, ng=2, sees=ns + 4)])
    units = [filler_unit(d, 1 + k, 2) for k in range(3)] + [probe] + [filler_unit(d, 7 - k, 3) for k in range(2)]
    for k, u in enumerate(units):
        u["species"] = k // 2
    return assemble(units, dict(group="E", case=case, rpw=rpw, step=step))


# ---- the conditions ----------------------------------------------------------------------------------------------------------------

def _oracle(table, soa, k=0):
    from oracle import c_oracle
    st, er, counts, allele, stats = c_oracle.pileup(thresholds(k), table, soa)
    assert st == 0, "oracle refused the input (%d at read %d)" % (st, er)
    return counts, stats


def _claims_hold(facts, tt, what=("ns", "ni", "ng", "sees")):
    assert tt["n_tiles"] == facts["n_tiles"]
    for t, claim in enumerate(facts["tiles"]):
        got = {k: int(tt[k][t]) for k in what}
        assert got == {k: claim[k] for k in what}, "tile %d (%s): the packer makes %s of it" % (t, claim, got)


def _tile_sites(facts, t):
    b = facts["tiles"][t]["site_base"]
    return slice(b, b + facts["tiles"][t]["len"])


def stream_conditions(table, soa, facts):
    grid, rpw, step = facts["grid"], facts["rpw"], facts["step"]
    tiles = facts["tiles"]
    tt = tile_table(table, soa)
    assert facts["n_tiles"] == 3 * grid and rpw == 64 // facts["lanes"]
    _claims_hold(facts, tt)
    probes = [t for t, c in enumerate(tiles) if c["kind"] == "probe"]
    assert sorted(tiles[t]["probe"] for t in probes) == sorted(3 * stream_probes(rpw))
    assert set(c["len"] for c in tiles if c["kind"] == "filler") == set(range(1, 8))
    assert all(1 <= c["ns"] <= 3 for c in tiles if c["kind"] == "filler")
    assert max(tt["sees"]) <= 2048                                   # no tile is split: the prefetch across the tile border is on
    # behind a tile with at least 2 * step records (the prefetch across the tile border is on in every wave): an empty tile, a
    # single record, another such tile, nothing; and a stream that starts with a record of its I range, of its G range
    total = tt["ns"] + tt["ni"] + tt["ng"]
    behind = set()
    for t in np.nonzero(total >= 2 * step)[0]:
        if t + grid >= facts["n_tiles"]:
            behind.add("none")
            continue
        ns, ni, ng = (int(tt[k][t + grid]) for k in ("ns", "ni", "ng"))
        behind.add("empty" if ns + ni + ng == 0 else "one" if (ns, ni, ng) == (1, 0, 0) else "long" if ns + ni + ng >= 2 * step else
                   "I first" if ns == 0 and ni else "G first" if ns == 0 else "other")
    assert behind >= {"none", "empty", "one", "long", "I first", "G first"}, behind
    # a successor of the same and of another species behind tiles that end on the fast path and on the general one
    seen = set((c["ni"] + c["ng"] > 0, tiles[t + grid]["species"] == c["species"])
               for t, c in enumerate(tiles[:2 * grid]) if c["kind"] == "probe" and c["sees"])
    assert len(seen) == 4, seen
    counts, stats = _oracle(table, soa)
    assert 2 * int(stats[:, 1].sum()) >= int(stats[:, 0].sum()) == len(facts["reads"])
    assert 2 * int(_oracle(table, soa, 1)[1][:, 1].sum()) >= len(facts["reads"])
    # no part of a probe's stream can be skipped unseen: without its I records, its G records, or the S records of its last,
    # partial wave-iteration the oracle counts something else in that tile
    rec_of = lambda t, cls0: np.nonzero((tt["tile"] == t) & ((tt["cls"] == 0) == cls0))[0]
    parts = {"I": {}, "G": {}, "S tail": {}}
    for t in probes:
        ns, ni, ng = tiles[t]["probe"]
        if ni:
            front = rec_of(t - 1, False)
            parts["I"][t] = tt["orig"][front[tt["reach"][front] > 0]]
            assert len(parts["I"][t]) == ni
        if ng:
            parts["G"][t] = tt["orig"][rec_of(t, False)]
        if ns % rpw:
            parts["S tail"][t] = tt["orig"][rec_of(t, True)[ns - ns % rpw:]]
    for name, drop in parts.items():
        assert len(drop) >= 3 * 8
        c2, _ = _oracle(*without(table, facts, np.concatenate(list(drop.values()))))
        same = [t for t in drop if np.array_equal(c2[_tile_sites(facts, t)], counts[_tile_sites(facts, t)])]
        assert not same, "without their %s records the oracle counts the same in tiles %s" % (name, same[:8])


def handout_conditions(table, soa, facts):
    tt = tile_table(table, soa)
    _claims_hold(facts, tt)
    assert all(c["kind"] == "filler" for c in facts["tiles"]) and facts["lanes"] == 1
    assert [c["species"] for c in facts["tiles"]] == [t // 5 for t in range(facts["n_tiles"])]
    for k in (0, 1):
        counts, stats = _oracle(table, soa, k)
        depth = counts.sum(axis=1)
        first = np.array([c["site_base"] for c in facts["tiles"]])
        last = first + np.array([c["len"] for c in facts["tiles"]]) - 1
        assert (depth[first] > 0).all() and (depth[last] > 0).all()
        assert (stats > 0).all()
        assert (stats[1:] != stats[:-1]).any(axis=1).all()


def split_conditions(table, soa, facts):
    grid, tiles = facts["grid"], facts["tiles"]
    tt = tile_table(table, soa)
    assert facts["n_tiles"] == grid + 40
    _claims_hold(facts, tt)
    fair, parts = planned_items(tt["sees"], grid)
    assert (fair, parts) == (facts["fair"], facts["parts"]) and 2 * fair <= 2048 and len(facts["reads"]) < 1000000
    by_name = {c["name"]: t for t, c in enumerate(tiles) if c["kind"] == "hot"}
    want = {"2048": 1, "2049": 3, "5000": 5, "last+2": 3, "last+3": 3, "adjacent 0": 3, "adjacent 1": 3, "in and out": 3}
    assert {n: parts[t] for n, t in by_name.items()} == want and sum(parts) == facts["n_work_items"] == facts["n_tiles"] + 16
    assert tt["sees"][by_name["2048"]] == 2048 and tt["sees"][by_name["2049"]] == 2049
    assert tiles[by_name["last+2"]]["len"] % 4 == 2 and tiles[by_name["last+3"]]["len"] % 4 == 3
    for n in ("last+2", "last+3"):
        t = by_name[n]
        assert tiles[t]["start"] > 0 and (t + 1 == len(tiles) or tiles[t + 1]["contig"] != tiles[t]["contig"])
    a0, a1 = by_name["adjacent 0"], by_name["adjacent 1"]
    assert a1 == a0 + 1 and tiles[a0]["contig"] == tiles[a1]["contig"]
    split = [t for t in range(len(tiles)) if parts[t] > 1]
    pairs = set(tiles[a]["species"] == tiles[b]["species"] for a, b in zip(split, split[1:]))
    assert pairs == {True, False}                                   # neighbours in the item list: of one species, of two
    t = by_name["in and out"]
    assert tt["ni"][t] == 6 and tt["ni"][t + 1] == 6 and tiles[t - 1]["contig"] == tiles[t + 1]["contig"]
    assert grid < sum(1 for p in parts if p == 1)                   # more whole tiles than workgroups: the item list is read
    quals = np.concatenate([r["qual"] for r in facts["reads"] if r["tag"] == "hot"])
    assert set(QUALS.tolist()) <= set(np.unique(quals).tolist())
    assert any((r["seq"] == N_CODE).any() for r in facts["reads"] if r["tag"] == "hot")
    pos = np.array([r["pos"] for r in facts["reads"]])
    contig = np.repeat(np.arange(len(table.length)), np.diff(facts["read_begin"]))
    for k in (0, 1):
        counts, _ = _oracle(table, soa, k)
        depth = counts.sum(axis=1)
        for t in split:
            d = depth[_tile_sites(facts, t)]
            assert d.min() == 0 and d.max() > 255, (tiles[t]["name"], int(d.min()), int(d.max()))
            mine = (contig == tiles[t]["contig"]) & (pos // TILE == tiles[t]["start"] // TILE)
            _, stats = _oracle(*without(table, facts, np.nonzero(~mine)[0]), k)
            aligned, mapped = int(stats[:, 0].sum()), int(stats[:, 1].sum())
            assert aligned == int(mine.sum()) and 0 < mapped < aligned


def far_conditions(table, soa, facts):
    from oracle import c_oracle
    tt = tile_table(table, soa)
    assert facts["n_tiles"] == 3 * 2 + FAR_TILES and facts["lanes"] == 5
    assert (tt["ns"] + tt["ng"] >= 20).all()                        # every tile has reads of its own
    far = [i for i, r in enumerate(facts["reads"]) if r["tag"] == "far"]
    assert len(far) == 4 * 4 * 2 * 2
    rec_of = {}
    for j, i in enumerate(tt["orig"]):
        rec_of.setdefault(int(i), []).append(j)
    for reach in FAR_REACH:
        for i in far:
            r = facts["reads"][i]
            if r["reach"] != reach:
                continue
            recs = rec_of[i]
            if r["kept"]:                 # one record, class 2, the reach field capped at 31
                assert len(recs) == 1 and tt["cls"][recs[0]] == 2 and tt["reach"][recs[0]] == min(reach, 31), (r["place"], reach)
            else:                         # match segments: class 0, cut at a tile border where they cross one
                assert len(recs) in (2, 3) and all(tt["cls"][j] == 0 for j in recs)
    fields = sorted(int(tt["reach"][rec_of[i][0]]) for i in far if facts["reads"][i]["kept"])
    assert fields == [30] * 8 + [31] * 24
    places = set((r["reach"], r["place"], r["kept"]) for r in (facts["reads"][i] for i in far))
    assert len(places) == 4 * 4 * 2
    for r in (facts["reads"][i] for i in far):
        end = r["behind"] + FAR_A - 1
        want = {"first site": r["pos"] % TILE == 0, "last site": r["pos"] % TILE == TILE - 1,
                "ends on a last site": end % TILE == TILE - 1, "ends on a first site": end % TILE == 0}
        assert want[r["place"]]
    st, er, counts, _, stats = c_oracle.pileup(thresholds(0), table, soa)
    assert st == 0 and 2 * int(stats[:, 1].sum()) >= len(facts["reads"])
    # the oracle counts bases of every far read on both sides of its skip
    base = int(table.site_offsets()[2])
    for i in far:
        r = facts["reads"][i]
        c2, _ = _oracle(*without(table, facts, [i]))
        front, behind = slice(base + r["pos"], base + r["pos"] + FAR_A), slice(base + r["behind"], base + r["behind"] + FAR_A)
        assert (counts[front].sum(axis=1) - c2[front].sum(axis=1) == 1).all(), (r["reach"], r["place"])
        assert (counts[behind].sum(axis=1) - c2[behind].sum(axis=1) == 1).all(), (r["reach"], r["place"])
    # the reads whose skip runs past their contig's end: the reach is cut at the contig, the bases in front of the skip count
    past = [i for i, r in enumerate(facts["reads"]) if r["tag"] == "past the end"]
    assert len(past) == 4
    for i in past:
        j, = rec_of[i]
        t = int(tt["tile"][j])
        last = max(k for k, c in enumerate(facts["tiles"]) if c["contig"] == facts["tiles"][t]["contig"])
        assert tt["cls"][j] == 2 and tt["reach"][j] == min(31, last - t)
    assert sorted(int(tt["reach"][rec_of[i][0]]) for i in past) == [1, 1, 1, 31]


def refused_conditions(table, soa, facts):
    from oracle import c_oracle
    tt = tile_table(table, soa)
    _claims_hold(facts, tt)
    rpw, step = facts["rpw"], facts["step"]
    bad = [(i, r["refused"]) for i, r in enumerate(facts["reads"]) if "refused" in r]
    assert sorted(x for _, x in bad) == sorted(facts["case"]) and facts["lanes"] == 5
    probe, = [t for t, c in enumerate(facts["tiles"]) if c["kind"] == "probe"]
    ns = facts["tiles"][probe]["ns"]
    assert step < ns and ns % rpw and (ns - 1) // rpw > (step - 1) // rpw
    for i, (place, kind) in bad:
        j, = np.nonzero(tt["orig"] == i)[0]
        if place in ("I", "G"):       # one record that keeps its CIGAR: it starts in the tile in front and reaches in / in the probe
            assert (tt["tile"][j], tt["cls"][j]) == ((probe - 1, 2) if place == "I" else (probe, 1))
        else:                         # a class-0 record at its place of the probe's stream
            mine = np.nonzero((tt["tile"] == probe) & (tt["cls"] == 0))[0]
            assert j == mine[{"S first": 0, "S last fast": step - 1, "S tail": ns - 1}[place]]
    first = min(bad)
    for k in (0, 1):
        st, er, *_ = c_oracle.pileup(thresholds(k), table, soa)
        assert (st, er) == (REFUSED_STATUS[first[1][1]], first[0])
    return first


CONDITIONS = {"A": stream_conditions, "B": handout_conditions, "C": split_conditions, "D": far_conditions, "E": refused_conditions}
