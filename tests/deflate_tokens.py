"""A token-level reader of raw DEFLATE streams (RFC 1951) for the tests of the two row coders: what zlib only inflates, this
takes apart -- the text, the tokens (a literal is an int, a match a (length, distance) pair) and, per dynamic block, the three
vectors of code lengths -- so that a test can say WHICH match a coder chose and how deep its codes are.  Plain Python, no
dependencies; tests/test_deflate_tokens_host.py holds it against zlib's own streams before it judges anybody."""
import heapq

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


class DeflateError(ValueError):
    pass


class Block:
    """One block of a stream: kind 0 stored, 1 fixed, 2 dynamic; tokens[first_token:end_token] are its own; for a dynamic block the
    code lengths as sent (cl_lens by symbol 0..18, ll_lens [HLIT + 257], d_lens [HDIST + 1]) and the code length symbols
    that spelt them (cl_symbols: 0..15 a length, 16 / 17 / 18 the repeats; cl_runs: how many lengths each of them stood for)."""

    def __init__(self, kind, final):
        self.kind, self.final = kind, final
        self.first_token = self.end_token = 0
        self.cl_lens = self.ll_lens = self.d_lens = self.cl_symbols = self.cl_runs = None


class Parsed:
    """length_codes: per match, in order, the length code 0..28 that spelt it (258 can be code 28, or code 27 with 31 extra)"""

    def __init__(self, text, tokens, blocks, n_bytes, length_codes=None):
        self.text, self.tokens, self.blocks, self.n_bytes, self.length_codes = text, tokens, blocks, n_bytes, length_codes

    @property
    def matches(self):
        return [t for t in self.tokens if type(t) is tuple]


def kraft(lens):
    """(sum of 2^-len over the symbols in use as a fraction of 2^15: complete = 32768, symbols in use)"""
    used = [l for l in lens if l]
    return sum(32768 >> l for l in used), len(used)


def _table(lens, what):
    """Decoding table of the canonical code (RFC 1951 3.2.2), indexed by the next max_len bits of the stream (first bit lowest):
    entry = symbol << 4 | length, 0 where no code word begins so."""
    max_len = max(lens) if lens else 0
    if max_len == 0:
        return [0], 0
    if max_len > 15:
        raise DeflateError("%s: a code length above 15" % what)
    k, _ = kraft(lens)
    if k > 32768:
        raise DeflateError("%s: over-subscribed code" % what)
    count = [0] * (max_len + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (max_len + 2)
    for b in range(1, max_len + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [0] * (1 << max_len)
    for sym, l in enumerate(lens):
        if l:
            c = nxt[l]
            nxt[l] += 1
            r = int(format(c, "0%db" % l)[::-1], 2)
            n = 1 << (max_len - l)
            table[r::1 << l] = [(sym << 4) | l] * n
    return table, max_len


def parse(raw):
    """raw: a raw DEFLATE stream (anything behind its final block is left alone) -> Parsed(text, tokens, blocks, n_bytes it took)."""
    raw = bytes(raw)
    n_raw = len(raw)
    pos = acc = fill = 0           # next byte of raw; the bits read but not used, lowest first

    def need(n):
        nonlocal pos, acc, fill
        while fill < n:
            if pos >= n_raw:
                raise DeflateError("the stream ends inside a block")
            acc |= raw[pos] << fill
            pos += 1
            fill += 8

    def bits(n):
        nonlocal acc, fill
        if n == 0:
            return 0
        need(n)
        v = acc & ((1 << n) - 1)
        acc >>= n
        fill -= n
        return v

    def symbol(table, max_len, what):
        nonlocal pos, acc, fill
        while fill < max_len and pos < n_raw:
            acc |= raw[pos] << fill
            pos += 1
            fill += 8
        e = table[acc & ((1 << max_len) - 1)]
        l = e & 15
        if e == 0 or l > fill:
            raise DeflateError("%s: no such code word (or the stream ends inside one)" % what)
        acc >>= l
        fill -= l
        return e >> 4

    out, tokens, blocks, length_codes = bytearray(), [], [], []
    while True:
        final, kind = bits(1), bits(2)
        blk = Block(kind, bool(final))
        blk.first_token = len(tokens)
        if kind == 0:
            pos -= fill // 8       # (whole bytes were read, some of them ahead: what is left of the current one is padding)
            acc, fill = 0, 0
            if pos + 4 > n_raw:
                raise DeflateError("the stream ends inside a stored block's header")
            ln, nln = raw[pos] | raw[pos + 1] << 8, raw[pos + 2] | raw[pos + 3] << 8
            if ln ^ nln != 0xFFFF or pos + 4 + ln > n_raw:
                raise DeflateError("stored block: bad length")
            out += raw[pos + 4:pos + 4 + ln]
            tokens.extend(raw[pos + 4:pos + 4 + ln])
            pos += 4 + ln
        elif kind in (1, 2):
            if kind == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise DeflateError("dynamic block: HLIT / HDIST out of range")
                cl_lens = [0] * 19
                for i in range(hclen):
                    cl_lens[CL_ORDER[i]] = bits(3)
                cl_table, cl_max = _table(cl_lens, "code length code")
                lens, syms, runs = [], [], []
                while len(lens) < hlit + hdist:
                    s, before = symbol(cl_table, cl_max, "code length code"), len(lens)
                    syms.append(s)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise DeflateError("dynamic block: repeat with nothing before it")
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
                    runs.append(len(lens) - before)
                if len(lens) != hlit + hdist:
                    raise DeflateError("dynamic block: a repeat runs past the code lengths")
                ll_lens, d_lens = lens[:hlit], lens[hlit:]
                if ll_lens[256] == 0:
                    raise DeflateError("dynamic block: no end-of-block code")
                blk.cl_lens, blk.ll_lens, blk.d_lens, blk.cl_symbols, blk.cl_runs = cl_lens, ll_lens, d_lens, syms, runs
            ll_table, ll_max = _table(ll_lens, "literal/length code")
            d_table, d_max = _table(d_lens, "distance code")
            while True:
                s = symbol(ll_table, ll_max, "literal/length code")
                if s < 256:
                    out.append(s)
                    tokens.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise DeflateError("length code %d" % (s - 257))
                    length = LEN_BASE[s - 257] + bits(LEN_EXTRA[s - 257])
                    d = symbol(d_table, d_max, "distance code")
                    if d > 29:
                        raise DeflateError("distance code %d" % d)
                    dist = DIST_BASE[d] + bits(DIST_EXTRA[d])
                    if dist > len(out):
                        raise DeflateError("a match reaches %d bytes back in a text of %d" % (dist, len(out)))
                    tokens.append((length, dist))
                    length_codes.append(s - 257)
                    at = len(out) - dist
                    if dist >= length:
                        out += out[at:at + length]
                    else:
                        for i in range(length):
                            out.append(out[at + i])
        else:
            raise DeflateError("block type 3")
        blk.end_token = len(tokens)
        blocks.append(blk)
        if final:
            break
    return Parsed(bytes(out), tokens, blocks, pos - fill // 8, length_codes)


def length_code(length):
    """the length code 0..28 (symbol 257 + code) of a match length 3..258, from the RFC's table"""
    assert 3 <= length <= 258, length
    c = 28
    while LEN_BASE[c] > length:
        c -= 1
    return c


def distance_code(dist):
    assert 1 <= dist <= 32768, dist
    c = 29
    while DIST_BASE[c] > dist:
        c -= 1
    return c


def frequencies(tokens):
    """(literal/length symbol counts [286], end of block included once; distance symbol counts [30]) of one block's tokens"""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if type(t) is tuple:
            ll[257 + length_code(t[0])] += 1
            d[distance_code(t[1])] += 1
        else:
            ll[t] += 1
    return ll, d


def huffman_depths(freq):
    """Depths of Huffman's tree for the symbols with freq > 0, with no limit on the depth: the two lightest nodes are merged, the
    older node first among equals (a leaf before any merged node, leaves by symbol).  One symbol: depth 1.  -> {symbol: depth}"""
    heap = [(f, s, (s,)) for s, f in enumerate(freq) if f]
    if len(heap) == 1:
        return {heap[0][1]: 1}
    depth = {s: 0 for _, s, _ in heap}
    heapq.heapify(heap)
    age = len(freq)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, age, a + b))
        age += 1
    return depth
