"""The case table of the device inflater's format tests: raw DEFLATE streams built token by token with tests/deflate_writer.py, each
aimed at one piece of bgzf_inflate.hip and each with a CLAIM -- a predicate over the stream as tests/deflate_tokens.py parses it --
that proves the stream contains the edge it is named after.  tests/test_deflate_writer_host.py holds every stream to zlib and to
the reader and asserts every claim; tests/test_gpu_inflate_format.py runs the same table on the device.

The groups, by the name's prefix, and the code each aims at:
  shape/   limits_from_counts, Limits::pack / length, decode<>: the 1..15,15 chain in both alphabets (15-bit codes on the most used
           symbols; the end-of-block code deepest), equal lengths, codes of three and of four symbols, HLIT 286 + HDIST 30 with every
           length and distance code at its least and most extra bits, 258 as code 285 and as 284 + 31, distance 32768, HLIT 257 +
           HDIST 1 without a distance code, one and two one-bit distance codes, blocks whose only code is a one-bit end of block
  header/  ClCode, lengths_pass, dynamic_tables and its seek: HCLEN 5 (the least that spells an end of block) and 19, a 7-bit code
           length code, 16 / 17 / 18 across the border of the two alphabets, an 18 of 138, 16 behind 17 and 18, the last repeat ending
           on the last length, the header at every bit 0..7 of a byte at every offset 0..3 mod 4 behind a fixed block, behind stored blocks
  bits/    refill_fast, short_of_words, emergency, top_up: 220 matches of 15 + 5 + 15 + 13 bits in a row, also all of length 258
  tokens/  TokenOut::step, finish, kEscape: literal runs of 0, 1, 3, 4, 5, 510, 511, 512, 1022 in front of a match and behind the last
           one, no match at all, one literal and then matches of distance 1 only
  stored/  kStored, skip(n & 7): LEN 0 (between, final, first, twice), 1, 65535, behind a block that ends at each bit 0..7, matches that
           reach into stored bytes and over two block borders
  room/    TokenOut::fits, kMatchRoom, inflate_again: the last stream that fits the first-pass room, one with a dword to spare and the
           first that overflows it, by one dword -- found out by finish()'s partial literal dword, and by a token's push (1000 and 65000
           bytes; 400 bytes of which 5 are literals); the densest legal stream
  placer/  make_window, place_literals, the dependency masks, periodic8: 1 / 63 / 64 / 65 / 127 / 128 / 129 tokens, literal runs of
           1..9 / 63 / 64 / 65, every distance 1..16 with every length of PAIR_LENGTHS, sources inside the token's own literals, chains of
           150 matches, a source across the window border, random streams under random codes, a last match whose load passes the end
  valid/   a stream with garbage behind its final block

cases()      -> [(name, raw, text, claim)]          valid streams
spec(name)   -> [(kind, tokens, ll_lens, d_lens)]   what the writer was asked for, block by block
malformed()  -> [(name, raw, ulen, refused_by, zlib_says)]   one broken rule each; refused_by: the ONE line of bgzf_decode_kernel that
                                                    refuses it and the status it sets (status_code()); zlib_says: zlib's error for it (None: zlib inflates it, to another size
                                                    or not to its end)
"""
import functools
import random

from tests import deflate_tokens as DT
from tests import deflate_writer as DW
from tests.deflate_tokens import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA


# ---- the kernel's bookkeeping, modelled from the code -----------------------------------------------------------------------------
def kernel_counts(tokens):
    """(tokens as TokenOut counts them, literal dwords, literals): one token per match, one escape token in front of a match whose
    literal run is 511 or more, one for the literals behind the last match; four literals to a dword"""
    toks = lits = run = 0
    for t in tokens:
        if type(t) is tuple:
            toks += 2 if run >= 511 else 1
            run = 0
        else:
            run += 1
            lits += 1
    return toks + (1 if run else 0), (lits + 3) // 4, lits


def first_pass_dwords(ulen):
    """decode_plan.h first_pass_room, in dwords"""
    return 2 * (ulen // 8 + 16)


def room_needed(tokens):
    """The least room (dwords) in which TokenOut takes the stream.  fits() -- 2 + tw + lw + 2 <= room -- is asked BEFORE every token
    and every literal dword is added (push; the dword paths of literal, step and finish), the counts only grow, so the last
    addition decides: 4 + (tokens + literal dwords - 1) <= room."""
    t, lw, _ = kernel_counts(tokens)
    return 3 + t + lw


def token_out_takes(tokens, room):
    """TokenOut (bgzf_inflate.hip) step by step, its counters only: does a room of `room` dwords take the stream, or is `full` set?"""
    tw = lw = na = run = 0
    for t in list(tokens) + [None]:
        if t is None:                       # finish(): the escape token of the last literals, then the partly filled dword
            adds = (["token"] if run else []) + (["dword"] if na else [])
        elif type(t) is tuple:              # step(mat): an escape token in front of a run of 511 or more, the match's token
            adds, run = (["token", "token"] if run >= 511 else ["token"]), 0
        else:                               # step(lit): a dword with every fourth literal
            na, run = na + 1, run + 1
            adds, na = (["dword"], 0) if na == 4 else ([], na)
        for a in adds:
            if not 2 + tw + lw + 2 <= room:     # fits()
                return False
            tw, lw = tw + (a == "token"), lw + (a == "dword")
    return True


def last_addition(tokens):
    """what TokenOut adds last, and so where a stream that misses its room by one dword finds out: finish() pushes the escape token
    of the literals behind the last match first and adds the partly filled literal dword after it; without such a dword the last
    addition is the last token (step's push of a match, or finish's escape token)"""
    return "finish: literal dword" if kernel_counts(tokens)[2] % 4 else "push: token"


def literal_runs(tokens):
    """([literals in front of every match], literals behind the last match)"""
    runs, run = [], 0
    for t in tokens:
        if type(t) is tuple:
            runs.append(run)
            run = 0
        else:
            run += 1
    return runs, run


def match_bits(p):
    """per token of the parsed stream: the bits its match took (code + extra + code + extra), 0 for a literal"""
    out, m = [], 0
    for blk in p.blocks:
        ll, d = (blk.ll_lens, blk.d_lens) if blk.kind == 2 else (DT.FIXED_LL, DT.FIXED_D)
        for t in p.tokens[blk.first_token:blk.end_token]:
            if type(t) is tuple:
                c, dc = p.length_codes[m], DT.distance_code(t[1])
                m += 1
                out.append(ll[257 + c] + LEN_EXTRA[c] + d[dc] + DIST_EXTRA[dc])
            else:
                out.append(0)
    return out


def longest_streak(values, want):
    best = cur = 0
    for v in values:
        cur = cur + 1 if v == want else 0
        best = max(best, cur)
    return best


def first_fixed_block_bits(p):
    """the bits of the stream's first block, a fixed block of literals: where the second block begins"""
    b = p.blocks[0]
    assert b.kind == 1 and b.first_token == 0
    return 3 + sum(DT.FIXED_LL[t] for t in p.tokens[:b.end_token]) + 7


# ---- building ----------------------------------------------------------------------------------------------------------------------
class _Table:
    def __init__(self):
        self.cases, self.specs = [], {}

    def add(self, name, w, claim, tail=b""):
        assert name not in self.specs, name
        tokens = [t for b in w.blocks for t in b[1]]
        self.cases.append((name, w.getvalue() + tail, DW.expected_text(tokens), claim))
        self.specs[name] = w.blocks


def _rand_lits(rng, n, lo=0, hi=256):
    return [rng.randrange(lo, hi) for _ in range(n)]


def random_tokens(rng, ll_lens, d_lens, n, have=0, p_match=0.3, favor=(), favor_len=(), favor_d=(), max_text=40000):
    """n random tokens that the two codes can spell and that are valid behind `have` bytes of text; matches carry their length code.
    favor*: symbols chosen four times out of five where they can be."""
    lits = [s for s in range(min(256, len(ll_lens))) if ll_lens[s]]
    lcs = [c for c in range(29) if 257 + c < len(ll_lens) and ll_lens[257 + c]]
    dcs = [c for c in range(len(d_lens)) if d_lens[c]]

    def pick(fav, pool):
        fav = [x for x in fav if x in pool]
        return rng.choice(fav) if fav and rng.random() < 0.8 else rng.choice(pool)
    out, size = [], have
    for _ in range(n):
        ok_d = [c for c in dcs if DIST_BASE[c] <= size]
        if lcs and ok_d and (not lits or rng.random() < p_match):
            c, dc = pick(favor_len, lcs), pick(favor_d, ok_d)
            length = LEN_BASE[c] + rng.randrange(1 << LEN_EXTRA[c])
            dist = min(size, DIST_BASE[dc] + rng.randrange(1 << DIST_EXTRA[dc]))
            out.append((length, dist, c))
            size += length
        else:
            out.append(pick(favor, lits))
            size += 1
        if size > max_text:
            break
    return out


def _uses(p, blk_i, lens_attr, sym_of, depth):
    """how many tokens of block blk_i use a symbol whose code in that alphabet is `depth` bits long"""
    blk = p.blocks[blk_i]
    lens = getattr(blk, lens_attr)
    n, m = 0, sum(1 for t in p.tokens[:blk.first_token] if type(t) is tuple)
    for t in p.tokens[blk.first_token:blk.end_token]:
        s = sym_of(t, p.length_codes[m] if type(t) is tuple else None)
        if type(t) is tuple:
            m += 1
        if s is not None and lens[s] == depth:
            n += 1
    return n


_ll_sym = lambda t, c: 257 + c if type(t) is tuple else t
_d_sym = lambda t, c: DT.distance_code(t[1]) if type(t) is tuple else None


def _fixed_to_bit(w, phase, align, rng):
    """A non-final fixed block behind which the next block begins at bit `phase` of a byte whose offset is `align` mod 4.  (A fixed
    block is 3 + 7 bits around literals of 8 bits, or 9 from 144 up.)"""
    at = w.bit_length
    for n9 in range(8):
        for n8 in range(4):
            end = at + 10 + 9 * n9 + 8 * n8
            if end % 8 == phase and (end // 8) % 4 == align:
                toks = _rand_lits(rng, n9, 144, 256) + _rand_lits(rng, n8, 32, 127)
                rng.shuffle(toks)
                w.fixed(toks, False)
                assert w.bit_length == end
                return toks
    raise AssertionError((phase, align))


def _code_shapes(T, rng):
    # the deepest code in both alphabets; A: the 15-bit codes on the most used symbols, B: the end-of-block code deepest
    for tag, ll_order, d_order, fav, fav_len, fav_d in (
            ("deep_codes_on_the_most_used", [256, 260, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 258, 76, 257], [15, 14, 13, 12, 11, 10,
                    9, 8, 7, 6, 5, 4, 3, 2, 0, 1],
             [76], [0], [0, 1]),
            ("end_of_block_deepest", [65, 257, 66, 67, 258, 68, 69, 70, 71, 72, 73, 74, 75, 260, 76, 256], list(range(16)), [76], [3], [14, 15])):
        ll_lens, d_lens = DW.chain_lens(ll_order, 286)[:261], DW.chain_lens(d_order, 30)[:16]
        toks = _rand_lits(rng, 300, 65, 77) + random_tokens(rng, ll_lens, d_lens, 900, 300, 0.4, fav, fav_len, fav_d)
        w = DW.Writer().dynamic(toks, ll_lens, d_lens, True)
        eob = 15 if ll_order[-1] == 256 else 1
        T.add("shape/chain/" + tag, w, lambda p, eob=eob: max(p.blocks[0].ll_lens) == 15 and max(p.blocks[0].d_lens) == 15
                and p.blocks[0].ll_lens[256] == eob
              and sorted(l for l in p.blocks[0].ll_lens if l) == list(range(1, 16)) + [15]
                      and sorted(l for l in p.blocks[0].d_lens if l) == list(range(1, 16)) + [15]
              and _uses(p, 0, "ll_lens", _ll_sym, 15) >= 100 and _uses(p, 0, "d_lens", _d_sym, 15) >= 50)
    # complete codes of equal lengths: 256 x 8 bits (254 literals, end of block, length 3) and 16 x 4 bits
    ll_lens, d_lens = DW.equal_lens(list(range(254)) + [256, 257], 286)[:258], DW.equal_lens(list(range(16)), 30)[:16]
    toks = _rand_lits(rng, 260, 0, 254) + random_tokens(rng, ll_lens, d_lens, 600, 260, 0.5)
    T.add("shape/equal_lengths_8_and_4", DW.Writer().dynamic(toks, ll_lens, d_lens, True),
          lambda p: set(p.blocks[0].ll_lens) == {0, 8} and set(p.blocks[0].d_lens) == {4} and len(p.matches) > 100)
    for k in (1, 2):       # two literals and the end of block: 1 + 2 + 2 bits; 4 symbols of 2 bits
        syms = [65, 66, 256] if k == 1 else [65, 66, 67, 256]
        ll_lens = [0] * 257
        for i, s in enumerate(syms):
            ll_lens[s] = 2 if k == 2 or i else 1
        T.add("shape/tiny_code_%d" % k, DW.Writer().dynamic(_rand_lits(rng, 700, 65, 65 + len(syms) - 1), ll_lens, [0], True),
              lambda p, n=len(syms): sum(1 for l in p.blocks[0].ll_lens if l) == n and DT.kraft(p.blocks[0].ll_lens)[0] == 32768)
    # every symbol of both alphabets in use (HLIT 286, HDIST 30) behind 32 768 stored bytes: every length code and every distance code
    # at its smallest and its largest extra bits, 258 spelt both ways, distance 32768
    hist = bytes(rng.randrange(256) for _ in range(32768))
    ll_lens, d_lens = DW.full_lens(286, short=[256] + list(range(257, 286))), DW.full_lens(30, short=[29, 28])
    toks = []
    for c in range(29):
        for extra in {0, (1 << LEN_EXTRA[c]) - 1}:
            toks += [rng.randrange(256), (LEN_BASE[c] + extra, rng.randrange(1, 32769), c)]
    for dc in range(30):
        for extra in {0, (1 << DIST_EXTRA[dc]) - 1}:
            toks += [rng.randrange(256), (rng.randrange(3, 12), DIST_BASE[dc] + extra)]
    toks += [(258, 32768, 28), (258, 32768, 27), (258, 1, 27), (3, 32768)]
    toks += random_tokens(rng, ll_lens, d_lens, 400, 40000, 0.3)

    def every_code(p):
        seen_l = {(c, t[0] - LEN_BASE[c]) for c, t in zip(p.length_codes, p.matches)}
        seen_d = {(DT.distance_code(t[1]), t[1] - DIST_BASE[DT.distance_code(t[1])]) for t in p.matches}
        b = p.blocks[1]
        return (len(b.ll_lens) == 286 and all(b.ll_lens) and len(b.d_lens) == 30 and all(b.d_lens)
                and all((c, e) in seen_l for c in range(29) for e in (0, (1 << LEN_EXTRA[c]) - 1))
                and all((c, e) in seen_d for c in range(30) for e in (0, (1 << DIST_EXTRA[c]) - 1))
                and (27, 31) in seen_l and (28, 0) in seen_l and max(t[1] for t in p.matches) == 32768)
    T.add("shape/all_286_and_30_every_code_258_both_ways_distance_32768", DW.Writer().stored(hist).dynamic(toks, ll_lens, d_lens, True), every_code)
    # HLIT 257 and HDIST 1 with no distance code at all: a literal-only block
    toks = _rand_lits(rng, 900, 0, 256)
    ll_lens, _ = DW.lens_for(toks)
    T.add("shape/hlit_257_hdist_1_no_distance_code", DW.Writer().dynamic(toks, ll_lens[:257], [0], True),
          lambda p: len(p.blocks[0].ll_lens) == 257 and p.blocks[0].d_lens == [0] and not p.matches)
    # one distance code of one bit, used (HDIST 1: distance 1; and as the fourth of four: distance 4); two distance codes of one bit
    for tag, d_lens in (("one_distance_code_of_one_bit", [1]), ("one_distance_code_of_one_bit_dist4", [0, 0, 0, 1]),
            ("two_distance_codes_of_one_bit", [1, 1])):
        toks = _rand_lits(rng, 9, 97, 105)
        for _ in range(120):
            toks += _rand_lits(rng, rng.randrange(0, 3), 97, 105) + [(rng.randrange(3, 40), rng.choice([i + 1 for i, l in enumerate(d_lens) if l]))]
        ll_lens, _ = DW.lens_for(toks)
        T.add("shape/" + tag, DW.Writer().dynamic(toks, ll_lens, d_lens, True),
              lambda p, d=d_lens: p.blocks[0].d_lens == d and len(p.matches) == 120 and {t[1] for t in p.matches} == {i + 1 for i,
                      l in enumerate(d) if l})
    # a block whose only code is a one-bit end of block: an empty non-final block, in front of, between and behind normal blocks
    only_eob = [0] * 256 + [1]
    a, b = _rand_lits(rng, 40, 97, 123), [(5, 7), 98, (30, 40), 99]
    w = DW.Writer().dynamic([], only_eob, [0]).auto(a).dynamic([], only_eob, [0]).dynamic([], only_eob, [0]).fixed(b).dynamic([], only_eob, [0], True)
    T.add("shape/blocks_of_one_code_the_end_of_block", w, lambda p: [bl.end_token - bl.first_token for bl in p.blocks] == [0, 40, 0, 0, 4, 0]
          and all(sum(bl.ll_lens) == 1 and bl.ll_lens[256] == 1 for bl in (p.blocks[0], p.blocks[2], p.blocks[3], p.blocks[5])))


def distance_32769_cannot_be_spelt():
    """Code 29 is 24577 + 13 extra bits: 32768 at most.  No token spells 32769, so no stream can ask the device for it."""
    return DIST_BASE[29] + (1 << DIST_EXTRA[29]) - 1 == 32768 and len(DIST_BASE) == 30


def _header_spellings(T, rng):
    # HCLEN 5 (the least that can spell an end-of-block code: with 4, only 16 / 17 / 18 / 0 have codes and every length is zero -- see
    # malformed()): lengths 8 and 0 only.  255 literals and the end of block, 8 bits each
    ll_lens = [8] * 255 + [0, 8]
    cl = [0] * 19
    cl[0] = cl[8] = 1
    T.add("header/hclen_5", DW.Writer().dynamic(_rand_lits(rng, 500, 0, 255), ll_lens, [0], True, cl_lens=cl, cl_symbols=[(l,
            1) for l in ll_lens + [0]]),
          lambda p: sum(1 for i, s in enumerate(DT.CL_ORDER) if p.blocks[0].cl_lens[s] and i >= 5) == 0 and p.blocks[0].cl_lens[8] == 1
                  and len(p.blocks[0].cl_symbols) == 258)
    # HCLEN 19: the last of the nineteen, the length of symbol 15, is in use (the deepest chain again, spelt length by length)
    ll_lens, d_lens = DW.chain_lens([256, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 257, 258, 259, 97, 98],
            286)[:260], DW.chain_lens(list(range(16)), 30)[:16]
    toks = _rand_lits(rng, 200, 48, 58) + random_tokens(rng, ll_lens, d_lens, 300, 200)
    T.add("header/hclen_19", DW.Writer().dynamic(toks, ll_lens, d_lens, True), lambda p: p.blocks[0].cl_lens[15] > 0 and 15 in p.blocks[0].cl_symbols)
    # a code length code with 7-bit codes: 1, 2, 3, 4, 5, 6, 7, 7 over eight symbols.  Lengths 6..9: 32 + 32 + 32 + 64 symbols
    order = [s for s in range(20, 200) if s not in (50, 60, 61, 62, 63, 64, 70, 90, 91, 92, 100, 130)]      # (gaps: zeros spelt 0 and 17)
    ll_lens = [0] * 257
    for i, s in enumerate(order[:159] + [256]):
        ll_lens[s] = 6 if i < 32 else 7 if i < 64 else 8 if i < 96 else 9
    cl = [0] * 19
    for l, s in zip((1, 2, 3, 4, 5, 6, 7, 7), (9, 8, 16, 7, 6, 18, 17, 0)):
        cl[s] = l
    T.add("header/code_length_code_of_7_bits", DW.Writer().dynamic([rng.choice(order[:159]) for _ in range(800)], ll_lens, [0], True, cl_lens=cl),
          lambda p: sorted(l for l in p.blocks[0].cl_lens if l) == [1, 2, 3, 4, 5, 6, 7, 7]
                  and sum(1 for s in p.blocks[0].cl_symbols if p.blocks[0].cl_lens[s] == 7) >= 2)

    def crosses(p, sym):     # a repeat `sym` whose lengths lie on both sides of the border between the two alphabets
        b, at = p.blocks[0], 0
        for s, run in zip(b.cl_symbols, b.cl_runs):
            if s == sym and at < len(b.ll_lens) < at + run:
                return True
            at += run
        return False
    # 16 across the border: the last length codes and the first distance codes all 4 bits
    ll_lens, d_lens = DW.equal_lens([256, 257, 258, 259] + list(range(100, 112)), 286)[:260], DW.equal_lens(list(range(16)), 30)[:16]
    toks = _rand_lits(rng, 300, 100, 112) + random_tokens(rng, ll_lens, d_lens, 300, 300)
    sp = DW.spell(ll_lens[:256]) + [(4, 1), (16, 6), (16, 6), (16, 4), (16, 3)]       # (and the last repeat ends exactly on the last length)
    T.add("header/repeat_16_across_the_border", DW.Writer().dynamic(toks, ll_lens, d_lens, True, cl_symbols=_respell_tail(sp, ll_lens + d_lens)),
          lambda p: crosses(p, 16) and p.blocks[0].cl_symbols[-1] == 16 and sum(p.blocks[0].cl_runs) == 260 + 16)
    # 17 and 18 across it: the last length symbols and the first distance symbols unused
    for sym, n_ll, d0 in ((17, 260, 3), (18, 270, 20)):
        toks = _rand_lits(rng, 30000 if d0 == 20 else 40, 97, 123)
        for _ in range(200):
            toks += _rand_lits(rng, rng.randrange(0, 4), 97, 123) + [(3, DIST_BASE[d0] + rng.randrange(0, 3))]
        ll_lens, d_lens = DW.lens_for(toks, n_ll=n_ll)
        T.add("header/repeat_%d_across_the_border" % sym, DW.Writer().dynamic(toks, ll_lens, d_lens, True), lambda p, sym=sym: crosses(p, sym))
    # an 18 of 138; a 16 directly behind an 18 and behind a 17 (it repeats a zero); the last repeat ends exactly on the last length
    toks = _rand_lits(rng, 600, 200, 256)
    ll_lens, _ = DW.lens_for(toks)
    T.add("header/repeat_18_of_138", DW.Writer().dynamic(toks, ll_lens, [0], True), lambda p: (18, 138) in zip(p.blocks[0].cl_symbols,
            p.blocks[0].cl_runs))
    toks = _rand_lits(rng, 600, 40, 60) + _rand_lits(rng, 100, 120, 126)
    ll_lens, _ = DW.lens_for(toks)
    sp = [(18, 37), (16, 3)] + DW.spell(ll_lens[40:60]) + [(17, 10), (16, 6), (16, 6), (16, 6), (16, 6), (18,
            26)] + DW.spell(ll_lens[120:]) + [(17, 3), (16, 3)]
    T.add("header/repeat_16_behind_17_and_18", DW.Writer().dynamic(toks, ll_lens, [0, 0, 0, 0, 0, 0], True, cl_symbols=_respell_tail(sp,
            ll_lens + [0] * 6)),
          lambda p: any(a in (17, 18) and b == 16 for a, b in zip(p.blocks[0].cl_symbols, p.blocks[0].cl_symbols[1:]))
                  and p.blocks[0].cl_symbols[-1] == 16
          and not any(p.blocks[0].d_lens))
    # the dynamic header at every bit phase and byte alignment, as a later block (behind a fixed block) ...
    for phase in range(8):
        for align in range(4):
            w = DW.Writer()
            front = _fixed_to_bit(w, phase, align, rng)
            toks = _rand_lits(rng, 30, 97, 110)
            for _ in range(60):
                toks += _rand_lits(rng, rng.randrange(0, 3), 97, 110) + [(rng.randrange(3, 20), rng.randrange(1, len(front) + 20))]
            w.auto(toks, True)
            T.add("header/at_bit_%d_of_byte_%d_mod_4" % (phase, align), w, lambda p, phase=phase,
                    align=align: [b.kind for b in p.blocks] == [1, 2] and len(p.matches) == 60
                  and first_fixed_block_bits(p) % 8 == phase and first_fixed_block_bits(p) // 8 % 4 == align)
    # ... behind a stored block (bit 0, every alignment) ...
    for align in range(4):
        data = bytes(_rand_lits(rng, 7 + align, 0, 256))       # 1 + 4 + n bytes in front of the header
        w = DW.Writer().stored(data)
        toks = [(6, 3), 97, (100, 5), 98, 99, (3, 1)]
        T.add("header/behind_a_stored_block_byte_%d_mod_4" % ((12 + align) % 4), w.auto(toks, True), lambda p,
                align=align: [b.kind for b in p.blocks] == [0, 2] and (5 + p.blocks[0].end_token) % 4 == align)
    # ... and as the first block with a second dynamic block behind it (the first header is at bit 0: the byte alignment is the stream's)
    a = _rand_lits(rng, 200, 97, 123)
    b = random_tokens(rng, *DW.lens_for(_rand_lits(rng, 300, 97, 123) + [(3, 1), (20, 100), (258, 150)]), 200, 200)
    T.add("header/two_dynamic_blocks", DW.Writer().auto(a).auto(b, True), lambda p: [bl.kind for bl in p.blocks] == [2, 2])


def _respell_tail(spelling, lens):
    """the hand-made spelling must spell exactly `lens`: checked here, where it is made"""
    got = []
    for s, run in spelling:
        if s < 16:
            got.append(s)
        elif s == 16:
            got += [got[-1]] * run
        else:
            got += [0] * run
    assert got == list(lens), (len(got), len(lens), [i for i, (x, y) in enumerate(zip(got, lens)) if x != y][:5])
    return spelling


def slow_matches(rng, n, length):
    """Matches of 15 + 5 + 15 + 13 = 48 bits each, n in a row, behind 16 500 stored bytes: the length code 24 (131..162) or 27 (227..258)
    and the distance codes 28 / 29 (from 16385) on the two 15-bit codes of the deepest chain."""
    ll_lens = DW.chain_lens([97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 256, 257 + 24, 257 + 27], 286)[:285]
    d_lens = DW.chain_lens(list(range(14)) + [28, 29], 30)
    hist = bytes(rng.randrange(256) for _ in range(16500))
    toks, size = [97, 98], 16502
    for _ in range(n):
        ln = length if length else 131 + rng.randrange(32)
        toks.append((ln, rng.randrange(16385, min(size, 32768) + 1), 27 if length == 258 else DT.length_code(ln)))
        size += ln
    toks += [99, 100]
    return DW.Writer().stored(hist).dynamic(toks, ll_lens, d_lens, True)


def one_bit_literals(n):
    """n literals of one bit each (and an end-of-block code of one bit): what a lane next to a slow one decodes meanwhile"""
    ll_lens = [0] * 257
    ll_lens[97] = ll_lens[256] = 1
    return DW.Writer().dynamic([97] * n, ll_lens, [0], True)


def _bit_budget(T, rng):
    T.add("bits/220_matches_of_48_bits", slow_matches(rng, 220, 0), lambda p: longest_streak(match_bits(p), 48) >= 200)
    T.add("bits/220_matches_of_48_bits_length_258", slow_matches(rng, 220, 258),
          lambda p: longest_streak(match_bits(p), 48) >= 200 and all(t[0] == 258 for t in p.matches) and set(p.length_codes) == {27})
    T.add("bits/one_bit_literals", one_bit_literals(12000), lambda p: p.blocks[0].ll_lens[97] == 1 and p.blocks[0].ll_lens[256] == 1
            and len(p.tokens) == 12000)


RUNS = (0, 1, 3, 4, 5, 510, 511, 512, 1022)


def _token_edges(T, rng):
    for r in RUNS:
        toks = _rand_lits(rng, max(r, 1), 0, 256) + [(4, 1)] + _rand_lits(rng, r, 0, 256) + [(rng.randrange(3, 9), rng.randrange(1,
                5))] + _rand_lits(rng, r, 0, 256)
        for kind in ("fixed", "dynamic"):
            w = DW.Writer().fixed(toks, True) if kind == "fixed" else DW.Writer().auto(toks, True)
            T.add("tokens/run_of_%d_%s" % (r, kind), w, lambda p, r=r: literal_runs(p.tokens) == ([max(r, 1), r], r)
                  and kernel_counts(p.tokens)[0] == 2 + (2 if r >= 511 else 0) + (1 if r else 0))
    T.add("tokens/no_match_300_literals", DW.Writer().auto(_rand_lits(rng, 300, 0, 256), True), lambda p: not p.matches
            and kernel_counts(p.tokens) == (1, 75, 300))
    T.add("tokens/no_match_2000_literals", DW.Writer().auto(_rand_lits(rng, 2000, 0, 256), True), lambda p: not p.matches
            and kernel_counts(p.tokens) == (1, 500, 2000))
    T.add("tokens/one_literal_then_matches_of_distance_1", DW.Writer().auto([7] + [(rng.randrange(3, 259), 1) for _ in range(90)], True),
          lambda p: literal_runs(p.tokens) == ([1] + [0] * 89, 0) and {t[1] for t in p.matches} == {1})


def _stored(T, rng):
    a, b = _rand_lits(rng, 50, 97, 123), [(10, 20), 65, (4, 1)]
    T.add("stored/len_0_between_two_huffman_blocks", DW.Writer().auto(a).stored(b"").fixed(b, True),
          lambda p: [bl.kind for bl in p.blocks] == [2, 0, 1] and p.blocks[1].first_token == p.blocks[1].end_token and not p.blocks[1].final)
    T.add("stored/len_0_final", DW.Writer().auto(a).stored(b"", True), lambda p: [bl.kind for bl in p.blocks] == [2, 0]
            and p.blocks[1].first_token == p.blocks[1].end_token)
    T.add("stored/len_0_first_and_twice", DW.Writer().stored(b"").stored(b"").fixed(a).stored(b"").stored(b"", True),
            lambda p: [bl.kind for bl in p.blocks] == [0, 0, 1, 0, 0])
    T.add("stored/len_1", DW.Writer().stored(b"x", True), lambda p: p.text == b"x")
    T.add("stored/len_1_between", DW.Writer().fixed(a).stored(b"y").fixed([(3, 1)], True),
            lambda p: p.blocks[1].end_token - p.blocks[1].first_token == 1)
    T.add("stored/len_65535", DW.Writer().stored(bytes(rng.randrange(256) for _ in range(65535)), True), lambda p: len(p.text) == 65535
            and len(p.blocks) == 1)
    # behind a Huffman block that ended at each of the eight bit phases; then matches that reach back into the stored bytes and over both borders
    for phase in range(8):
        w = DW.Writer()
        front = _fixed_to_bit(w, phase, phase % 4, rng)
        n0, data = len(front), bytes(_rand_lits(rng, 5 + phase, 0, 256))
        w.stored(data)
        toks = [(4, 3), (3, len(data)), (len(data) + 2, len(data) + 7 + 1), 66, (3, n0 + len(data) + 4 + 3 + len(data) + 2 + 1 - 1)]
        w.fixed(toks, True)
        T.add("stored/behind_a_block_that_ends_at_bit_%d" % phase, w, lambda p, n0=n0, nd=len(data),
                phase=phase: [b.kind for b in p.blocks] == [1, 0, 1] and first_fixed_block_bits(p) % 8 == phase
              and p.matches[2][1] > nd + 7 and p.matches[3][1] >= nd + 4 + 3 + nd + 2 + 1)


def room_stream(rng, ulen, delta, lits):
    """A stream of `ulen` bytes that needs the first-pass room of that size + delta dwords (room_needed): `lits` literals, then matches only"""
    need = first_pass_dwords(ulen) + delta
    n = need - 3 - (lits + 3) // 4 - (1 if lits >= 511 else 0)
    spare = ulen - lits - 3 * n
    assert n > 0 and 0 <= spare <= 255 * n, (ulen, delta, lits, n, spare)
    toks, size = _rand_lits(rng, lits, 0, 256), lits
    for k in range(n):
        ln = 3 + min(255, spare) if k % 3 == 2 or spare > 255 * (n - 1 - k) or k == n - 1 else 3 + min(spare, rng.randrange(0, 3))
        ln = min(ln, 3 + spare)
        spare -= ln - 3
        toks.append((ln, rng.randrange(1, min(size, 32768) + 1)))
        size += ln
    assert spare == 0 and size == ulen
    return toks


def _room(T, rng):
    # around the border of the first-pass room: the last stream that fits, one with a dword to spare, the first that does not (it is
    # decoded again); what is added last, and so finds the room full, is finish()'s partly filled literal dword (literals not a
    # multiple of four) or a match's token (a multiple of four)
    def at_the_border(ulen, delta, lits, last):
        def claim(p):
            room = first_pass_dwords(ulen)
            return (len(p.text) == ulen and room_needed(p.tokens) == room + delta and kernel_counts(p.tokens)[2] == lits
                    and last_addition(p.tokens) == last and type(p.tokens[-1]) is tuple
                    and token_out_takes(p.tokens, room) == (delta <= 0) and token_out_takes(p.tokens, room + delta)
                    and not token_out_takes(p.tokens, room + delta - 1))
        return claim
    for ulen, lits, tag in ((1000, 41, "small"), (1000, 40, "small_literals_in_whole_dwords"), (65000, 17001, "near_64k"),
                            (65000, 17000, "near_64k_literals_in_whole_dwords"), (400, 5, "fewer_than_8_literals")):
        last = "finish: literal dword" if lits % 4 else "push: token"
        for delta, what in ((0, "last_that_fits"), (-1, "one_dword_to_spare"), (1, "first_that_overflows")):
            toks = room_stream(rng, ulen, delta, lits)
            T.add("room/%s_%s" % (tag, what), DW.Writer().auto(toks, True), at_the_border(ulen, delta, lits, last))
    for n in (2000, 21000):      # the densest legal stream: more tokens than any first-pass room holds
        T.add("room/densest_%d" % n, DW.Writer().fixed([9] + [(3, 1)] * n, True), lambda p, n=n: len(p.matches) == n
                and len(p.text) == 1 + 3 * n and room_needed(p.tokens) > first_pass_dwords(1 + 3 * n))


PAIR_LENGTHS = (3, 4, 7, 8, 9, 15, 16, 17, 257, 258)


def _placer(T, rng):
    for n in (1, 63, 64, 65, 127, 128, 129):
        toks = []
        for _ in range(n):
            toks += _rand_lits(rng, rng.randrange(1, 4), 0, 256) + [(rng.randrange(3, 12), rng.randrange(1, len(toks) + 2))]
        T.add("placer/%d_tokens" % n, DW.Writer().auto(toks, True), lambda p, n=n: kernel_counts(p.tokens)[0] == n == len(p.matches))
        T.add("placer/%d_tokens_the_last_an_escape" % n, DW.Writer().auto(toks[:-1] + [5, 6], True), lambda p,
                n=n: kernel_counts(p.tokens)[0] == n == len(p.matches) + 1)
    runs = list(range(1, 10)) + [63, 64, 65]
    toks = []
    for r in runs * 2:
        toks += _rand_lits(rng, r, 0, 256) + [(rng.randrange(3, 10), rng.randrange(1, len(toks) + r + 1))]
    T.add("placer/literal_runs_1_to_9_63_64_65", DW.Writer().auto(toks, True), lambda p: literal_runs(p.tokens) == (runs * 2, 0))
    # every distance 1..16 with every length: behind 17 fresh literals (the source begins inside the token's own literals), and behind
    # 2 (it reaches into the matches in front)
    for lits in (17, 2):
        toks = _rand_lits(rng, 20, 0, 256)
        pairs = [(ln, d) for d in range(1, 17) for ln in PAIR_LENGTHS]
        rng.shuffle(pairs)
        for pr in pairs:
            toks += _rand_lits(rng, lits, 0, 256) + [pr]
        T.add("placer/every_distance_1_to_16_with_every_length_behind_%d_literals" % lits, DW.Writer().auto(toks, True),
              lambda p, lits=lits: set(p.matches) == {(ln, d) for d in range(1, 17) for ln in PAIR_LENGTHS}
                      and literal_runs(p.tokens)[0][1:] == [lits] * 159
              and (lits == 2 or all(m[1] <= lits for m in p.matches)))
    # chains: every match copies the output of the match in front of it, through whole windows of 64 tokens and over their borders
    for ln, d in ((8, 8), (5, 5), (9, 3), (3, 3), (20, 7), (258, 258)):
        toks = _rand_lits(rng, d, 0, 256) + [(ln, d)] * 150
        T.add("placer/chain_of_150_matches_%d_%d" % (ln, d), DW.Writer().auto(toks, True), lambda p, ln=ln, d=d: p.matches == [(ln,
                d)] * 150 and literal_runs(p.tokens) == ([d] + [0] * 149, 0))
    # a match whose source straddles the border of the previous window: token 64 (the second window's first) reads the last bytes of
    # token 63's match, its own two literals in between
    toks = [1]
    for _ in range(64):
        toks += [rng.randrange(256), (3, 1)]
    toks += [200, 201, (10, 6)] + [rng.randrange(256), (4, 9)] * 10

    def straddles(p):
        starts, at = [], 0          # the first byte of every token (its literals), as the placer's windows have it
        for r, m in zip(literal_runs(p.tokens)[0], p.matches):
            starts.append(at)
            at += r + m[0]
        o = starts[64] + 2
        return p.matches[64] == (10, 6) and o - 6 < starts[64] < o - 6 + 6
    T.add("placer/source_straddles_the_window_border", DW.Writer().auto(toks, True), straddles)
    # random streams under random codes: what nobody thought of
    for k in range(24):
        base = _rand_lits(rng, 400, 0, 256) + [(rng.randrange(3, 259), rng.randrange(1, 300)) for _ in range(60)]
        ll_lens, d_lens = DW.lens_for(base + [(3, 20000), (100, 9000)], max_len=rng.choice((9, 11, 15)))
        toks = random_tokens(rng, ll_lens, d_lens, 1 + 40 * (k % 5), 0, 0.0)
        toks += random_tokens(rng, ll_lens, d_lens, rng.randrange(900, 2500), len(toks), rng.choice((0.1, 0.5, 0.9)), max_text=64000)
        # (more than one of the placer's windows, and matches that reach behind their own token)
        T.add("placer/random_%02d" % k, DW.Writer().dynamic(toks, ll_lens, d_lens, True),
              lambda p: kernel_counts(p.tokens)[0] >= 65 and len(p.matches) >= 64 and any(m[1] > r for m, r in zip(p.matches,
                      literal_runs(p.tokens)[0])))
    # (the table's last stream, and so the last of a launch: its match's 8-byte load reaches past its own bytes)
    T.add("placer/length_3_distance_3_as_the_last_bytes", DW.Writer().fixed([1, 2, 3, (3, 3)], True), lambda p: p.tokens[-1] == (3, 3)
            and len(p.text) == 6)


def _garbage(T, rng):
    toks = _rand_lits(rng, 40, 97, 123) + [(9, 30), 98]
    w = DW.Writer().auto(toks, True)
    T.add("valid/trailing_garbage_behind_the_final_block", w, lambda p, n=len(w.getvalue()): p.n_bytes == n and p.blocks[-1].final,
          tail=bytes([0xFF, 0x07, 0xA5, 0xFF, 0xFF, 0x00, 0x13, 0xFF, 0xEE]))


@functools.lru_cache(maxsize=None)
def _table():
    T, rng = _Table(), random.Random(1951)
    for part in (_code_shapes, _header_spellings, _bit_budget, _token_edges, _stored, _room, _garbage, _placer):
        part(T, rng)
    return T


def cases():
    return list(_table().cases)


def spec(name):
    return _table().specs[name]


# ---- malformed streams: one broken rule each -------------------------------------------------------------------------------------
def good_stream():
    toks = list(b"a good stream in front, ") + [(12, 24), 33]
    return DW.Writer().fixed(toks, True).getvalue(), DW.expected_text(toks)


STATUS = {"kBadBlockType": 1, "kBadStored": 2, "kBadCodeLengths": 3, "kBadSymbol": 4, "kBadDistance": 5, "kOutputOverrun": 6,
          "kInputOverrun": 7, "kShortOutput": 8}        # bgzf_inflate.hip; the C ABI's message names it: "code %u"


def status_code(refused_by):
    """the status the refusing line ends in ('... -> kName')"""
    return STATUS[refused_by.rsplit("-> ", 1)[1]]


ZLIB_SAYS = {
    "block_type_3": "invalid block type", "stored_len_nlen_mismatch": "invalid stored block lengths",
    "hlit_287": "too many length or distance symbols", "hlit_288": "too many length or distance symbols",
    "hdist_31": "too many length or distance symbols", "hdist_32": "too many length or distance symbols",
    "code_length_code_over_subscribed": "invalid code lengths set", "code_length_code_incomplete": "invalid code lengths set",
    "code_length_code_of_one_code": "invalid code lengths set", "repeat_16_first": "invalid bit length repeat",
    "repeat_past_the_last_length": "invalid bit length repeat", "no_end_of_block_code": "missing end-of-block",
    "hclen_4_spells_no_end_of_block": "missing end-of-block", "literal_length_code_over_subscribed": "invalid literal/lengths set",
    "literal_length_code_incomplete": "invalid literal/lengths set", "distance_code_over_subscribed": "invalid distances set",
    "distance_code_incomplete": "invalid distances set", "distance_code_single_of_two_bits": "invalid distances set",
    "match_without_any_distance_code": "invalid distance code", "the_other_bit_of_a_single_distance_code": "invalid distance code",
    "fixed_symbol_286": "invalid literal/length code", "fixed_symbol_287": "invalid literal/length code",
    "fixed_distance_code_30": "invalid distance code", "fixed_distance_code_31": "invalid distance code",
    "distance_beyond_the_text_first_block": "invalid distance too far back", "distance_beyond_the_text_second_block": "invalid distance too far back",
}


def malformed():
    """[(name, raw, ulen, refused_by, zlib_says)]: refused_by is the line of bgzf_decode_kernel (or of what it calls) that was found,
    by reading, to refuse the stream before anything is indexed with what the stream says."""
    rng = random.Random(3)
    out = []
    add = lambda name, raw, ulen, line: out.append((name, bytes(raw), ulen, line, ZLIB_SAYS.get(name)))
    lits = list(b"malformed? no: ")
    ll_ok, d_ok = DW.lens_for(lits + [(3, 1), (3, 2)])
    assert len(ll_ok) == 258 and len(d_ok) == 2 and DT.kraft(ll_ok)[0] == 32768
    W = DW.Writer

    add("block_type_3", W().bits(1, 1).bits(3, 2).bits(0, 29).getvalue(), 10, "type == 3u -> kBadBlockType")
    add("stored_len_nlen_mismatch", W().stored(b"0123456789", True, nlength=(10 ^ 0xFFFF) ^ 0x0100).getvalue(), 10,
            "(len ^ 0xFFFFu) != nlen -> kBadStored")
    add("stored_longer_than_the_input", W().stored(b"0123456789", True, length=100).getvalue(), 100, "kStored: in.overrun() -> kInputOverrun")
    add("stored_longer_than_ulen", W().stored(b"0123456789" * 2, True).getvalue(), 10, "out.o + len > ulen -> kOutputOverrun")
    add("stored_longer_than_ulen_left", W().fixed(lits).stored(b"0123456789", True).getvalue(), len(lits) + 9, "out.o + len > ulen -> kOutputOverrun")
    for hlit in (287, 288):
        add("hlit_%d" % hlit, W().header(DT.FIXED_LL[:hlit], [5] * 30, True).symbols(lits, DT.FIXED_LL, [5] * 30).getvalue(), len(lits),
                "dynamic_tables: hlit > 286 -> kBadCodeLengths")
    for hdist in (31, 32):
        add("hdist_%d" % hdist, W().header(DT.FIXED_LL[:286], [5] * hdist, True).symbols(lits, DT.FIXED_LL, [5] * 30).getvalue(), len(lits),
                "dynamic_tables: hdist > 30 -> kBadCodeLengths")
    sp = DW.spell(ll_ok + d_ok)
    used = sorted({s for s, _ in sp})

    good_cl = DW.limited_lens([sum(1 for s, _ in sp if s == k) for k in range(19)], 7)
    over = list(good_cl)
    over[used[0]] = max(1, min(l for l in good_cl if l) - 1) if good_cl[used[0]] > 1 else 1
    over[used[1]] = 1
    over[used[2]] = 1
    add("code_length_code_over_subscribed", W().header(ll_ok, d_ok, True, cl_lens=over).symbols(lits, ll_ok, d_ok).getvalue(), len(lits),
            "ClCode::build: left < 0 -> kBadCodeLengths")
    under = [l + 1 if l else 0 for l in good_cl]
    add("code_length_code_incomplete", W().header(ll_ok, d_ok, True, cl_lens=under).symbols(lits, ll_ok, d_ok).getvalue(), len(lits),
            "ClCode::build: left != 0 and not one code -> kBadCodeLengths")
    cl8 = [0] * 19
    cl8[8] = 1
    add("code_length_code_of_one_code", W().header([8] * 257, [8], True, cl_lens=cl8, cl_symbols=[(8, 1)] * 258).bits(0, 64).getvalue(), 5,
        "limits_from_counts (literal/length): left < 0 (257 codes of 8 bits: one code length symbol cannot spell a complete pair of codes) -> kBadCodeLengths")
    add("repeat_16_first", W().header(ll_ok, d_ok, True, cl_lens=[1 if s in (16, 0) else 0 for s in range(19)], cl_symbols=[(16, 3)] + [(0,
            1)] * 257).bits(0, 64).getvalue(), 5,
        "lengths_pass: s == 16 and i == 0 -> kBadCodeLengths")
    long_sp = sp[:-1] + [(18, 11)] if sp[-1][0] != 18 else sp[:-1] + [(18, sp[-1][1] + 1)]
    cl_long = DW.limited_lens([sum(1 for s, _ in long_sp if s == k) + (1 if k in used else 0) for k in range(19)], 7)
    add("repeat_past_the_last_length", W().header(ll_ok, d_ok, True, cl_lens=cl_long, cl_symbols=long_sp).symbols(lits, ll_ok,
            d_ok).getvalue(), len(lits),
        "lengths_pass: i + rep > total -> kBadCodeLengths")
    no_eob = list(ll_ok[:256]) + [0, ll_ok[256]]
    add("no_end_of_block_code", W().header(no_eob, d_ok, True).symbols(lits, no_eob, d_ok, eob=False).bits(0, 32).getvalue(), len(lits),
            "dynamic_tables: !has_eob -> kBadCodeLengths")
    cl4 = [0] * 19
    cl4[0] = cl4[18] = 1
    add("hclen_4_spells_no_end_of_block", W().header([0] * 257, [0], True, cl_lens=cl4, cl_symbols=[(18, 138), (18, 120)], hclen=4).bits(0,
            32).getvalue(), 5,
        "dynamic_tables: !has_eob (with HCLEN 4 only 16 / 17 / 18 / 0 have codes: every length is zero) -> kBadCodeLengths")

    def with_lens(name, ll, d, line, toks=lits):
        add(name, W().header(ll, d, True).symbols(toks, ll, d).getvalue(), len(toks), line)
    ll_over = list(ll_ok)
    ll_over[1] = min(l for l in ll_ok if l)
    with_lens("literal_length_code_over_subscribed", ll_over, d_ok, "limits_from_counts (literal/length): left < 0 -> kBadCodeLengths")
    ll_under = [0] * 257
    ll_under[109] = ll_under[256] = 2
    with_lens("literal_length_code_incomplete", ll_under, [0],
            "limits_from_counts (literal/length): left != 0, two codes -> kBadCodeLengths", [109, 109])
    with_lens("distance_code_over_subscribed", ll_ok, [1, 1, 1], "limits_from_counts (distance): left < 0 -> kBadCodeLengths")
    with_lens("distance_code_incomplete", ll_ok, [2, 2], "limits_from_counts (distance): left != 0, two codes -> kBadCodeLengths")
    with_lens("distance_code_single_of_two_bits", ll_ok, [2], "limits_from_counts (distance): one code, but lim[1] != 1 << 14 -> kBadCodeLengths")
    ll = DW.canonical_codes(ll_ok)
    add("match_without_any_distance_code", W().header(ll_ok, [0], True).symbols(lits, ll_ok, [0], eob=False).code(*ll[257]).bits(0,
            40).getvalue(), len(lits) + 3,
        "symbol loop: dl0 == 0 (no limit of an empty alphabet is below the value: length 16) -> kBadDistance")
    add("the_other_bit_of_a_single_distance_code", W().header(ll_ok, [1], True).symbols(lits, ll_ok, [1], eob=False).code(*ll[257]).bits(1,
            1).bits(0, 40).getvalue(), len(lits) + 3,
        "symbol loop: dl0 == 0 (every limit of a one-code alphabet is 1 << 14: length 16) -> kBadDistance")
    for s in (286, 287):
        add("fixed_symbol_%d" % s, W().bits(1, 1).bits(1, 2).symbols(lits, DT.FIXED_LL, DT.FIXED_D, eob=False).code(0xC0 + s - 280,
                8).bits(0, 40).getvalue(), len(lits) + 3,
            "symbol loop: is_len && !sl_ok (s - 257 >= 29) -> kBadSymbol")
    for dc in (30, 31):
        add("fixed_distance_code_%d" % dc, W().bits(1, 1).bits(1, 2).symbols(lits, DT.FIXED_LL, DT.FIXED_D, eob=False).code(1, 7).code(dc,
                5).bits(0, 40).getvalue(), len(lits) + 3,
            "symbol loop: dl0 == 0 (fixed_tables counts 30 codes of 5 bits: 30 << 10 is the last limit) -> kBadDistance")
    n = len(lits)
    add("distance_beyond_the_text_first_block", W().fixed(lits + [(3, n + 1)], True).getvalue(), n + 3, "symbol loop: dist > out.o -> kBadDistance")
    add("distance_beyond_the_text_second_block", W().fixed(lits).stored(b"xy").auto([65, (5, n + 2 + 1 + 1)], True).getvalue(),
            n + 2 + 1 + 5, "symbol loop: dist > out.o -> kBadDistance")
    add("one_literal_more_than_ulen", W().fixed(lits + [(4, 2), 65], True).getvalue(), n + 4,
            "symbol loop: is_lit && out.o >= ulen -> kOutputOverrun")
    add("one_match_more_than_ulen", W().fixed(lits + [65, (4, 2)], True).getvalue(), n + 1 + 3,
            "symbol loop: is_len && out.o + len > ulen -> kOutputOverrun")
    add("final_end_of_block_before_ulen", W().fixed(lits + [65, (4, 2)], True).getvalue(), n + 6, "behind the loop: out.o != ulen -> kShortOutput")
    # The stream cut.  These are traced with ZERO bits behind the cut: the test puts the stream last in its buffer, in front of the 512
    # zero bytes the host keeps behind the streams.
    first = W().stored(b"abc")                       # ends on a byte: the next block's three header bits are missing altogether
    add("cut_inside_the_header_bits", first.getvalue(), 10,
        "header: the zero bits are a stored block of LEN 0 and NLEN 0, refused before the header's in.overrun(): (len ^ 0xFFFFu) != nlen -> kBadStored")
    # 24 bits: the 17 of the header, the lengths of 16 and 17 and one bit of 18's; every other length reads as zero
    whole = W().header(ll_ok, d_ok, True, cl_lens=good_cl).getvalue()
    seen = [good_cl[16], good_cl[17], good_cl[18] & 1]
    assert sum(128 >> l for l in seen if l) != 128 and [l for l in seen if l] != [1]      # neither a complete code nor one code of one bit
    add("cut_inside_the_hclen_lengths", whole[:3], n, "ClCode::build: left != 0 and not one code (before lengths_pass asks in.overrun()) -> kBadCodeLengths")
    # two whole bytes of the length vector are kept: its first symbols are read as they were written, the one across the cut is whatever
    # its bits and the zeros spell -- a repeat of 138 at most, far from the 260th length -- and the check behind it finds the end passed
    ends = [W().header(ll_ok, d_ok, True, cl_lens=good_cl, cl_symbols=sp[:k]).bit_length for k in range(len(sp) + 1)]
    cut = (ends[0] + 7) // 8 + 2
    assert ends[1] <= 8 * cut and sum(run for (_, run), e in zip(sp,
            ends[1:]) if e <= 8 * cut) + 138 <= len(ll_ok) + len(d_ok) and 8 * cut + 24 < ends[-1]
    add("cut_inside_the_length_vector", whole[:cut], n, "lengths_pass: in.overrun() -> kInputOverrun")
    deep_ll = DW.chain_lens([97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 256, 257, 110, 109], 286)[:258]
    deep_d = DW.chain_lens(list(range(14)) + [28, 29], 30)
    hist = bytes(rng.randrange(256) for _ in range(16400))
    w = W().stored(hist).header(deep_ll, deep_d, True).symbols([97, 98, 97], deep_ll, deep_d, eob=False)
    at = w.bit_length
    w.symbols([109], deep_ll, deep_d, eob=False)       # 15 bits
    # (literal 109 is fourteen ones and a zero: the one to eight ones in front of the cut and a zero behind it are a shorter literal, which
    # still fits ulen, and whose last bit lies behind the cut)
    add("cut_inside_a_symbol", w.getvalue()[:at // 8 + 1], 16400 + 4, "symbol loop: in.overrun() -> kInputOverrun")
    hist = bytes(rng.randrange(256) for _ in range(30000))      # (enough text for any distance of code 29 with its low eight extra bits)
    w = W().stored(hist).header(deep_ll, deep_d, True).symbols([97, 98, 97], deep_ll, deep_d, eob=False)
    dd = DW.canonical_codes(deep_d)
    w.code(*DW.canonical_codes(deep_ll)[257]).code(*dd[29])
    at = w.bit_length
    w.bits(0x1ABC & 0x1FFF, 13)
    add("cut_inside_the_extra_bits", w.getvalue()[:at // 8 + 1], 30000 + 6, "symbol loop: in.overrun() -> kInputOverrun")
    return out
