"""The row kernel (rows_deflate.hip) on inputs of the tests' choosing, through midas_snps_rows_code -- the launch of
Batch.write_part with the members, the arena and the grid handed in.  The reference of every test is the text a Python
"%s\\t%d\\t%c\\t%d\\t%d\\t%d\\t%d\\t%d\\n" loop writes for the same numbers; zlib inflates each member's stream and
tests/deflate_tokens.py takes it apart, so that a case can say that the match it was built for is in the stream: the 258 cap,
the distances 32767 / 32768 / 32769, code lengths cut back to 15 and 7 bits, members that share a workgroup, a full arena."""
import zlib

import numpy as np
import pytest

from midas_amd import abi
from tests import deflate_tokens as DT

pytestmark = pytest.mark.gpu

ROWS_MAX = 16384
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


# ---- the reference and the checks every coded member has to pass --------------------------------------------------------------------

def member_text(counts, allele, member):
    site0, pos0, n_rows, cid = member
    rows = counts[site0:site0 + n_rows].tolist()
    al = allele[site0:site0 + n_rows].tolist()
    return b"".join(b"%s\t%d\t%c\t%d\t%d\t%d\t%d\t%d\n" % (cid, pos0 + i, al[i], sum(c), *c) for i, c in enumerate(rows))


def check_member(res, text, what=""):
    """A member the kernel coded (status 0) against its text -> the parsed stream."""
    assert res["status"] == 0, (what, res["status"])
    raw = res["stream"]
    d = zlib.decompressobj(-15)
    got = d.decompress(raw) + d.flush()
    assert d.eof and d.unused_data == b"", what
    if got != text:
        la, lb = got.split(b"\n"), text.split(b"\n")
        bad = next((i for i in range(min(len(la), len(lb))) if la[i] != lb[i]), min(len(la), len(lb)))
        raise AssertionError("%s: text differs at line %d of %d/%d: %r vs %r" % (what, bad, len(la), len(lb), la[bad:bad + 2], lb[bad:bad + 2]))
    assert res["crc"] == zlib.crc32(text), what
    assert res["text_len"] == len(text), what
    assert res["n_bytes"] == len(raw), what
    p = DT.parse(raw)
    assert p.text == text and p.n_bytes == len(raw), what
    for length, dist in p.matches:
        assert 3 <= length <= 258 and 1 <= dist <= 32768, (what, length, dist)
    assert len(p.blocks) == 1 and p.blocks[0].kind == 2, what
    b = p.blocks[0]
    for lens, limit in ((b.ll_lens, 15), (b.d_lens, 15), (b.cl_lens, 7)):
        k, used = DT.kraft(lens)
        assert max(lens) <= limit and (k == 32768 or used == 1), (what, limit, k, used)
    return p


def check_all(counts, allele, members, results, what=""):
    assert len(results) == len(members)
    return [check_member(r, member_text(counts, allele, m), "%s member %d" % (what, k)) for k, (m, r) in enumerate(zip(members, results))]


def tokens_at(parsed):
    """{offset in the text: token} of a parsed stream"""
    at, out = 0, {}
    for t in parsed.tokens:
        out[at] = t
        at += t[0] if type(t) is tuple else 1
    return out


def tail_hash(allele, c):
    """rows_deflate.hip, tail_hash: the 18 bits two rows have to share for the one to be looked at as the other's match"""
    h = 0x9E3779B97F4A7C15 ^ allele
    h = ((h ^ c[0]) * 0xFF51AFD7ED558CCD) & M64
    h = ((h ^ c[1]) * 0xFF51AFD7ED558CCD) & M64
    h = ((h ^ (h >> 29) ^ c[2]) * 0xFF51AFD7ED558CCD) & M64
    h = ((h ^ c[3]) * 0xC4CEB9FE1A85EC53) & M64
    return h >> 46


def common_digits(a, b):
    a, b = str(a), str(b)
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def pool_sites(rng, n, depth=12.0, n_tails=40):
    """n sites whose (allele, counts) come from a small pool: tails that repeat, as a table's do"""
    pc = np.zeros((n_tails, 4), np.uint32)
    pc[np.arange(n_tails), rng.integers(0, 4, n_tails)] = rng.poisson(depth, n_tails)
    pa = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n_tails)
    pick = rng.integers(0, n_tails, n)
    return pc[pick], pa[pick]


# ---- digits ---------------------------------------------------------------------------------------------------------------------------

BORDERS = [0] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [4294967295]


def test_digit_borders(ctx):
    """Every count of member 0 is one of 0, 9, 10, 99, 100, ... 999999999, 1000000000, 2^32 - 1 (each of them in each column);
    member 1 has the depths on both sides of nd64's two borders, 2^32 and 10^10, and the largest there is; members 2-10 start
    at 8, 98, ... 999999998 and walk over a digit border with tails that repeat (the match that runs into the next head meets a
    head one digit longer than the one behind the matched tail); the last member ends at position 2^31 - 1."""
    rng = np.random.default_rng(101)
    n_a = 400
    ca = np.array(BORDERS, np.uint64)[rng.integers(0, len(BORDERS), (n_a, 4))]
    for col in range(4):
        ca[:len(BORDERS), col] = np.roll(BORDERS, col)
    m32 = 4294967295
    cb = np.array([[m32, 0, 0, 0], [m32, 1, 0, 0], [0, m32, 0, 1], [m32, m32, 1410065409, 0], [m32, m32, 1410065410, 0], [m32, m32, 0, 1410065409],
                   [m32, m32, m32, m32], [m32, 0, 0, 0], [m32, m32, 1410065410, 0], [1, 2, 3, 4]], np.uint64)
    assert [int(r.sum()) for r in cb[:5]] == [4294967295, 4294967296, 4294967296, 9999999999, 10000000000]
    cp, ap = pool_sites(rng, 64, n_tails=3)
    counts = np.concatenate([ca, cb, cp.astype(np.uint64)]).astype(np.uint32)
    allele = np.concatenate([rng.choice(np.frombuffer(b"ACGTN", np.uint8), n_a + len(cb)), ap])
    at_b, at_p = n_a, n_a + len(cb)
    members = [(0, 1, n_a, b"digits"), (at_b, 7, len(cb), b"deep")]
    members += [(at_p + k, 10 ** k - 2, 9, b"border%d" % k) for k in range(1, 10)]
    members += [(at_p, 2147483647 - 63, 64, b"end"), (0, 2147483647 - n_a + 1, n_a, b"")]
    res = ctx.rows_code(counts, allele, members)
    parsed = check_all(counts, allele, members, res, "digits")
    assert b"\t17179869180\t4294967295\t4294967295\t4294967295\t4294967295\n" in parsed[1].text
    assert parsed[-1].text.endswith(b"\t2147483647" + member_text(counts, allele, (n_a - 1, 0, 1, b""))[2:])
    for k in range(1, 10):       # (the pool's three tails do repeat: the border is crossed by matches, not by literals alone)
        assert len(parsed[1 + k].matches) >= 6


@pytest.mark.parametrize("grid_blocks", [0, 2])
def test_id_lengths(ctx, grid_blocks):
    """Ids of 0, 1, 191, 192 and 193 bytes in one launch: the last is not taken (status 1, no bytes), its neighbours -- in the same
    workgroup's loop when there are two workgroups -- are right."""
    rng = np.random.default_rng(102)
    counts, allele = pool_sites(rng, 200)
    ids = [b"", b"i", bytes(rng.integers(33, 127, 191).astype(np.uint8)), b"x" * 192, b"y" * 193, b"after", bytes(rng.integers(33, 127, 192).astype(np.uint8))]
    members = [(3 * k, 95 + k, 150, cid) for k, cid in enumerate(ids)]
    res = ctx.rows_code(counts, allele, members, grid_blocks=grid_blocks)
    for k, (m, r) in enumerate(zip(members, res)):
        if len(m[3]) > 192:
            assert (r["status"], r["n_bytes"], r["text_len"], r["stream"], r["arena_off"]) == (1, 0, 0, None, -1)
        else:
            check_member(r, member_text(counts, allele, m), "id of %d bytes" % len(m[3]))


def test_row_counts(ctx):
    """1, 2, 31, 32, 33 (a thread's 32 rows and one more), 63, 64, 65 (the sort's smallest size), 16383 and 16384 rows in one
    launch; no rows and 16385 rows are not taken (status 1)."""
    rng = np.random.default_rng(103)
    counts, allele = pool_sites(rng, ROWS_MAX + 8)
    sizes = [1, 2, 31, 32, 33, 0, 63, 64, 65, 16385, 16383, 16384, -1, 1]
    members = [(k % 8, 1 + 1000 * k, n, b"contig_%d" % k) for k, n in enumerate(sizes)]
    res = ctx.rows_code(counts, allele, members)
    for m, r in zip(members, res):
        if 1 <= m[2] <= ROWS_MAX:
            check_member(r, member_text(counts, allele, m), "%d rows" % m[2])
        else:
            assert (r["status"], r["n_bytes"], r["stream"]) == (1, 0, None), m[2]


# ---- the format's limits --------------------------------------------------------------------------------------------------------------

def test_match_length_is_capped_at_258(ctx):
    """A 192-byte id, ten-digit positions and one 59-byte tail (four ten-digit counts, an eleven-digit depth) for 300 rows: tail +
    next head is 59 + 193 + 9 = 261 bytes that agree, the match may take 258 of them = 199 of the head's 203, and the row behind
    such a match starts with its position's last 4 digits as literals.  Member 1, the same rows under a 5-byte id: the matches
    are 59 + 5 + 1 + the digits two consecutive positions share, nowhere near the cap."""
    n = 300
    counts = np.tile(np.array([[3000000000, 3000000001, 3000000002, 3000000003]], np.uint32), (n, 1))
    allele = np.full(n, ord("G"), np.uint8)
    long_id, short_id = bytes(range(33, 33 + 96)) * 2, b"short"
    pos0 = 1234567801
    members = [(0, pos0, n, long_id), (0, pos0, n, short_id)]
    assert len(member_text(counts, allele, (0, pos0, 1, long_id))) == 203 + 59
    res = ctx.rows_code(counts, allele, members)
    p_long, p_short = check_all(counts, allele, members, res, "cap")
    # row 0: its tail as literals, then the next head against its own; rows 1 .. n - 2: one match each, tail + next head
    want_long, want_short = [], []
    for r in range(n - 1):
        c = common_digits(pos0 + r, pos0 + r + 1)
        want_long.append((min(59 * (r > 0) + 193 + c, 258), 262))
        want_short.append((59 * (r > 0) + 6 + c, 75))
    assert p_long.matches == want_long + [(59, 262)] and p_short.matches == want_short + [(59, 75)]
    assert p_long.matches.count((258, 262)) == n - 2 and max(m[0] for m in p_short.matches) == 59 + 6 + 9
    toks = p_long.tokens
    seen = 0
    for i, t in enumerate(toks):
        if t == (258, 262):
            seen += 1            # the match of row `seen` (row 0 has none of 258): behind it row seen + 1 starts, 199 bytes into its head
            assert bytes(toks[i + 1:i + 5]) == b"%d" % ((pos0 + seen + 1) % 10000) and type(toks[i + 5]) is tuple
    assert seen == n - 2


def test_match_distances_up_to_32768(ctx):
    """64-byte rows (a 34-byte id, five-digit positions, a four-digit depth, four three-digit counts).  Tail T sits in rows 3, 515,
    1027 and 1539; the 512 rows between the first two are 64 bytes each: T repeats 32768 bytes back.  Between the second and the
    third one row is a byte shorter (a two-digit count): 32767.  Between the third and the fourth one is a byte longer (a
    four-digit count): 32769, out of reach, so the fourth T goes out as literals.  All other tails are distinct and none shares
    T's hash, so the kernel's "nearest earlier row with this hash" is the T before."""
    rng = np.random.default_rng(104)
    n = 1600
    t_rows = [3, 515, 1027, 1539]
    T = (ord("C"), (777, 888, 999, 666))
    counts = np.zeros((n, 4), np.uint32)
    allele = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    seen = {T[1]}
    for r in range(n):
        while True:
            c = tuple(int(v) for v in rng.integers(250, 1000, 4))
            if c not in seen:
                break
        seen.add(c)
        counts[r] = c
    counts[700], counts[1300] = (900, 99, 901, 902), (400, 401, 1000, 402)       # the shorter and the longer row (depths stay four digits)
    for r in t_rows:
        counts[r], allele[r] = T[1], T[0]
    cid = b"contig_with_a_name_of_34_bytes_abc"
    member = (0, 10000, n, cid)
    # the construction, checked on the host: row lengths, where the tails are, and that T's hash is T's alone
    lines = member_text(counts, allele, member).split(b"\n")[:-1]
    assert len(cid) == 34 and [len(x) + 1 for x in lines] == [64 + (r == 1300) - (r == 700) for r in range(n)]
    begin = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])
    tail_at = [int(begin[r]) + 34 + 1 + 5 for r in t_rows]
    assert [b - a for a, b in zip(tail_at, tail_at[1:])] == [32768, 32767, 32769]
    hashes = [tail_hash(int(allele[r]), [int(v) for v in counts[r]]) for r in range(n)]
    assert all((hashes[r] == hashes[3]) == (r in t_rows) for r in range(n)) and 0 <= hashes[3] < 1 << 18
    assert all(int(counts[r].sum()) in range(1000, 10000) for r in range(n))
    res = ctx.rows_code(counts, allele, [member])
    p = check_member(res[0], member_text(counts, allele, member), "distances")
    at = tokens_at(p)
    for k, dist in ((1, 32768), (2, 32767)):
        t = at[tail_at[k]]
        assert type(t) is tuple and t[1] == dist and t[0] >= 24, (k, t)
    for i in range(24):          # the fourth T: 24 literals
        assert type(at[tail_at[3] + i]) is int, i
    assert max(d for _, d in p.matches) == 32768


def deep_litlen_input():
    """Allele bytes with 1, 1, 2, 4, ... 4096 rows each, shuffled, no two rows with the same counts: as literals they are a comb
    under the digits, tabs and newlines of 8192 rows."""
    rng = np.random.default_rng(105)
    values = [v for v in range(128, 256)][:14]
    reps = [1] + [1 << k for k in range(13)]
    allele = np.repeat(np.array(values, np.uint8), reps)
    rng.shuffle(allele)
    n = allele.size
    counts = np.zeros((n, 4), np.uint32)
    counts[:, 0] = rng.permutation(n) + 1
    counts[:, 1:] = rng.integers(0, 100000, (n, 3))
    return counts, allele, [(0, 1, n, b"deep_tree")]


def deep_codelen_input():
    """Allele bytes in groups of 1, 2, 4, ... symbols, a symbol of the next group half as frequent: the literal/length code then
    has 1, 2, 4, ... codes of lengths that grow by one, and the 19-symbol histogram of those lengths is itself a comb."""
    rng = np.random.default_rng(106)
    free = [v for v in range(256) if v not in b"\t\n0123456789"]
    values, reps, at = [], [], 0
    for g in range(8):
        size = min(1 << g, len(free) - at)
        values += free[at:at + size]
        reps += [256 >> g] * size
        at += size
    allele = np.repeat(np.array(values, np.uint8), reps)
    rng.shuffle(allele)
    n = allele.size
    counts = np.zeros((n, 4), np.uint32)
    counts[:, 0] = rng.permutation(n) + 1
    counts[:, 1:] = rng.integers(0, 1000, (n, 3))
    return counts, allele, [(0, 1, n, b"c")]


def test_code_lengths_are_cut_back_to_15_and_7_bits(ctx):
    """build_lengths' repair loops.  Precondition of each half, taken from the tokens the kernel itself chose: Huffman's tree for
    the block's symbol counts is deeper than the format allows; then the lengths sent must be within 15 / 7 bits and complete
    (check_member) and the stream must inflate.
    On the MI355X: deep_litlen_input's symbol counts give a tree 18 deep (15 sent, the code length code stays within 7 without
    repair); deep_codelen_input's code lengths give the 19 code length symbols the histogram 8 2 1 1 8 2 2 0 0 4 4 9 16 31 62 120,
    whose tree is 8 deep (7 sent): the first input reaches the 15-bit limit, the second the 7-bit one."""
    counts, allele, members = deep_litlen_input()
    p = check_all(counts, allele, members, ctx.rows_code(counts, allele, members, arena_bytes=64 * len(allele)), "deep literal/length tree")[0]
    ll, _ = DT.frequencies(p.tokens)
    depth_ll = max(DT.huffman_depths(ll).values())
    print("literal/length code: unconstrained depth %d, sent %d" % (depth_ll, max(p.blocks[0].ll_lens)))
    assert depth_ll > 15
    assert max(p.blocks[0].ll_lens) == 15

    counts, allele, members = deep_codelen_input()
    p = check_all(counts, allele, members, ctx.rows_code(counts, allele, members, arena_bytes=64 * len(allele)), "deep code length tree")[0]
    b = p.blocks[0]
    cl = [0] * 19
    for s in b.cl_symbols:
        cl[s] += 1
    depth_cl = max(DT.huffman_depths(cl).values())
    print("code length code: histogram %s, unconstrained depth %d, sent %d" % (cl, depth_cl, max(b.cl_lens)))
    assert depth_cl > 7
    assert max(b.cl_lens) == 7


# ---- members that share a workgroup, and the arena ----------------------------------------------------------------------------------------

def mixed_sites(rng, n):
    """pool tails, Poisson depths and full-range counts side by side; alleles ACGTN and any byte"""
    counts, allele = pool_sites(rng, n)
    kind = rng.random(n)
    some = kind < 0.10
    counts[some] = rng.poisson(30, (int(some.sum()), 4))
    wide = kind > 0.97
    counts[wide] = rng.integers(0, 1 << 32, (int(wide.sum()), 4), dtype=np.uint64).astype(np.uint32)
    odd = rng.random(n) < 0.02
    allele[odd] = rng.integers(0, 256, int(odd.sum()))
    return counts, allele


def test_members_that_share_a_workgroup(ctx):
    """Seven members of 16384, 1, 65, 16384, 33, 2, 16384 rows over one workgroup, over two, and over one each: a workgroup's
    shared memory (keys, offsets, histograms, codes, the ok flag) is whatever the member before left there.  Every member's
    stream is the same bytes in all three launches."""
    rng = np.random.default_rng(107)
    sizes = [16384, 1, 65, 16384, 33, 2, 16384]
    counts, allele = mixed_sites(rng, ROWS_MAX + 4000)
    members = [(int(rng.integers(0, 4000)), int(rng.integers(1, 10 ** (k + 2))), n, b"member_%d" % k * (k + 1)) for k, n in enumerate(sizes)]
    runs = [ctx.rows_code(counts, allele, members, grid_blocks=g) for g in (1, 2, len(sizes))]
    check_all(counts, allele, members, runs[0], "one workgroup")
    for other in runs[1:]:
        for k, (a, b) in enumerate(zip(runs[0], other)):
            assert {**a, "arena_off": 0} == {**b, "arena_off": 0}, k
    offs = sorted((r["arena_off"], (r["n_bytes"] + 3) & ~3) for r in runs[0])
    assert offs[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(offs, offs[1:]))      # one workgroup: in order, back to back
    assert [r["arena_off"] for r in runs[0]] == [o for o, _ in offs]


def test_arena_exactly_full_and_four_bytes_short(ctx):
    rng = np.random.default_rng(108)
    counts, allele = mixed_sites(rng, 3000)
    members = [(0, 1, 700, b"a"), (100, 5000, 1, b"bb"), (200, 77, 65, b"ccc"), (300, 123456, 2500, b"dddd")]
    ample = ctx.rows_code(counts, allele, members, arena_bytes=1 << 20, grid_blocks=1)
    check_all(counts, allele, members, ample, "ample arena")
    need = sum((r["n_bytes"] + 3) & ~3 for r in ample)
    exact = ctx.rows_code(counts, allele, members, arena_bytes=need, grid_blocks=1)
    assert exact == ample
    short = ctx.rows_code(counts, allele, members, arena_bytes=need - 4, grid_blocks=1)
    assert short[:-1] == ample[:-1]
    last = short[-1]
    assert (last["status"], last["stream"], last["n_bytes"]) == (2, None, 0)
    assert last["text_len"] == len(member_text(counts, allele, members[-1]))


def test_the_products_arena_rule_declines_an_incompressible_member(ctx):
    """16384 rows of four distinct random ten-digit counts: nothing matches but the heads, and 10 bytes a row + 5 KiB is not room
    enough: status 2 under the product's rule (Batch.write_part then takes the host's formatter), coded with ample room."""
    rng = np.random.default_rng(109)
    counts = rng.integers(1000000000, 1 << 32, (ROWS_MAX, 4), dtype=np.uint64).astype(np.uint32)
    allele = rng.choice(np.frombuffer(b"ACGT", np.uint8), ROWS_MAX)
    member = (0, 1, ROWS_MAX, b"incompressible")
    res = ctx.rows_code(counts, allele, [member])[0]
    text = member_text(counts, allele, member)
    assert (res["status"], res["text_len"]) == (2, len(text))
    res = ctx.rows_code(counts, allele, [member], arena_bytes=64 * ROWS_MAX)[0]
    check_member(res, text, "incompressible")
    print("incompressible member: %.2f bytes a row (the rule gives %.2f)" % (res["n_bytes"] / ROWS_MAX, (10 * ROWS_MAX + 5120) / ROWS_MAX))


def test_random_members(ctx):
    """40 members in one launch: 1 to 16384 rows, ids of 0 to 192 bytes, first positions anywhere below 2^31 - 16384, counts
    from a small pool, Poisson and the full 32-bit range, alleles ACGTN and any byte."""
    rng = np.random.default_rng(110)
    n_sites = 3 * ROWS_MAX
    counts, allele = mixed_sites(rng, n_sites)
    sizes = [ROWS_MAX, 1] + [int(2 ** rng.uniform(0, 14)) for _ in range(38)]
    members = []
    for k, n in enumerate(sizes):
        cid = bytes(rng.integers(33, 127, int(rng.choice([0, 1, 192, int(rng.integers(0, 193))]))).astype(np.uint8))
        members.append((int(rng.integers(0, n_sites - n + 1)), int(rng.integers(0, (1 << 31) - ROWS_MAX)), n, cid))
    res = ctx.rows_code(counts, allele, members)
    check_all(counts, allele, members, res, "random")
