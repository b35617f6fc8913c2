"""A token-level WRITER of raw DEFLATE streams (RFC 1951), the inverse of tests/deflate_tokens.py: it emits exactly the tokens, code
lengths, header spelling and block sequence a test asks for, so that an inflater can be held to the format and not to one encoder's
habits.  Same convention as the reader: a literal is an int, a match a (length, distance) pair; a third element forces the length
code (0..28), so that 258 can be spelt as code 27 plus 31 extra bits.  Plain Python, no dependencies.  Nothing here refuses a wrong
stream on purpose: `bits` is public, and the header and the symbols of a dynamic block can be written separately, so that a test can
break one rule at a time."""
from tests.deflate_tokens import (CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, distance_code, huffman_depths,
                                  length_code)


def canonical_codes(lens):
    """[(code, length)] per symbol of the canonical code (RFC 1951 3.2.2); (0, 0) for a symbol not in use"""
    max_len = max(lens) if lens else 0
    count = [0] * (max_len + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (max_len + 2)
    for b in range(1, max_len + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append((nxt[l], l))
            nxt[l] += 1
        else:
            out.append((0, 0))
    return out


# ---- code lengths -----------------------------------------------------------------------------------------------------------------
def chain_lens(order, n):
    """The deepest code there is: the 16 symbols of `order` get 1, 2, ... 14, 15, 15 bits in that order, the other symbols of the
    alphabet of n none."""
    assert len(order) == 16 and len(set(order)) == 16
    lens = [0] * n
    for k, s in enumerate(order):
        lens[s] = min(k + 1, 15)
    return lens


def equal_lens(symbols, n):
    """a complete code of equal lengths over `symbols` (a power of two of them)"""
    k = len(symbols).bit_length() - 1
    assert len(symbols) == 1 << k and k >= 1
    lens = [0] * n
    for s in symbols:
        lens[s] = k
    return lens


def full_lens(n, short=()):
    """A complete code over ALL n symbols: two neighbouring lengths, the shorter one for the symbols in `short` first, then from symbol
    0 up."""
    k = (n - 1).bit_length()
    n_short = (1 << k) - n
    order = list(short) + [s for s in range(n) if s not in set(short)]
    lens = [k] * n
    for s in order[:n_short]:
        lens[s] = k - 1
    return lens


def limited_lens(freq, max_len=15):
    """Code lengths of at most max_len bits for the symbols with freq > 0: Huffman's, and while the tree is too deep, again with the
    frequencies halved (never below one), which flattens it.  Always complete, except for a single symbol (one bit)."""
    freq = list(freq)
    assert sum(1 for f in freq if f) <= 1 << max_len
    while True:
        depth = huffman_depths(freq)
        if max(depth.values(), default=0) <= max_len:
            lens = [0] * len(freq)
            for s, d in depth.items():
                lens[s] = d
            return lens
        freq = [(f + 1) >> 1 if f else 0 for f in freq]


def lens_for(tokens, max_len=15, n_ll=None, n_d=None):
    """(ll_lens, d_lens) that fit one block's tokens, trimmed to the last symbol in use (HLIT >= 257, HDIST >= 1) unless sizes are given"""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if type(t) is tuple:
            ll[257 + (t[2] if len(t) == 3 else length_code(t[0]))] += 1
            d[distance_code(t[1])] += 1
        else:
            ll[t] += 1
    ll_lens, d_lens = limited_lens(ll, max_len), limited_lens(d, max_len)
    n_ll = n_ll or max(257, max(s for s, l in enumerate(ll_lens) if l) + 1)
    n_d = n_d or max([1] + [s + 1 for s, l in enumerate(d_lens) if l])
    return ll_lens[:n_ll], d_lens[:n_d]


def spell(lens):
    """The simple default spelling of a vector of code lengths: [(symbol, run)] -- 18 / 17 for runs of zeros, a length followed by 16s
    for runs of it, the longest repeats first.  The vector is spelt as ONE sequence, as the format has it: a run crosses the border
    between the two alphabets when the lengths on both sides are equal."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k)); run -= k
            if run >= 3:
                out.append((17, run)); run = 0
            out += [(0, 1)] * run
        else:
            out.append((v, 1)); run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k)); run -= k
            out += [(v, 1)] * run
        i = j
    return out


def expected_text(tokens):
    """the plain bytes the tokens spell, by the definition of a match"""
    out = bytearray()
    for t in tokens:
        if type(t) is tuple:
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out), (t, len(out))
            at = len(out) - dist
            if dist >= length:
                out += out[at:at + length]
            else:
                for i in range(length):
                    out.append(out[at + i])
        else:
            out.append(t)
    return bytes(out)


# ---- the writer -------------------------------------------------------------------------------------------------------------------
class Writer:
    """Bits first bit lowest (RFC 1951 3.1.1); Huffman codes most significant bit first.  `blocks` records what was asked for:
    (kind, tokens as (length, distance) pairs and ints, ll_lens, d_lens) per block."""

    def __init__(self):
        self.out = bytearray()
        self.acc = self.n = 0
        self.blocks = []

    @property
    def bit_length(self):
        return 8 * len(self.out) + self.n

    def bits(self, v, k):
        """k bits of v, lowest first"""
        assert 0 <= v < (1 << k) or k == 0, (v, k)
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, c, l):
        """a Huffman code of l bits, its first (most significant) bit first (of an over-subscribed code's overflowing values: the low l bits)"""
        return self.bits(int(format(c & ((1 << l) - 1), "0%db" % l)[::-1], 2) if l else 0, l)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self

    def getvalue(self):
        """the bytes so far, the last one padded with zero bits"""
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")

    # -- blocks
    def stored(self, data, final=False, length=None, nlength=None):
        """a stored block; length / nlength: what the LEN and NLEN fields say, if not the truth"""
        data = bytes(data)
        assert len(data) <= 65535
        self.bits(1 if final else 0, 1).bits(0, 2).align()
        ln = len(data) if length is None else length
        self.bits(ln, 16).bits(ln ^ 0xFFFF if nlength is None else nlength, 16)
        self.raw(data)
        self.blocks.append((0, list(data), None, None))
        return self

    def symbols(self, tokens, ll_lens, d_lens, eob=True):
        """the tokens of a Huffman block in the given codes, and the end-of-block code behind them"""
        ll, d = canonical_codes(ll_lens), canonical_codes(d_lens)
        for t in tokens:
            if type(t) is tuple:
                c = t[2] if len(t) == 3 else length_code(t[0])
                extra = t[0] - LEN_BASE[c]
                assert 0 <= extra < (1 << LEN_EXTRA[c]), t
                assert ll[257 + c][1], "no code for length symbol %d" % (257 + c)
                self.code(*ll[257 + c]).bits(extra, LEN_EXTRA[c])
                dc = distance_code(t[1])
                assert d[dc][1], "no code for distance symbol %d" % dc
                self.code(*d[dc]).bits(t[1] - DIST_BASE[dc], DIST_EXTRA[dc])
            else:
                assert ll[t][1], "no code for literal %d" % t
                self.code(*ll[t])
        if eob:
            assert ll[256][1]
            self.code(*ll[256])
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.bits(1 if final else 0, 1).bits(1, 2)
        self.symbols(tokens, FIXED_LL, FIXED_D, eob)
        self.blocks.append((1, [t[:2] if type(t) is tuple else t for t in tokens], None, None))
        return self

    def header(self, ll_lens, d_lens, final=False, cl_lens=None, cl_symbols=None, hclen=None, hlit=None, hdist=None):
        """The header of a dynamic block.  cl_symbols: the spelling of ll_lens + d_lens as [(symbol, run)] (run: 1 for a length, the
        number of repeats for 16 / 17 / 18), default spell(); cl_lens: the 19 lengths of the code length code, default: a code of
        at most 7 bits for the spelling's symbol counts; hclen: how many of them are sent, default: up to the last one in use."""
        if cl_symbols is None:
            cl_symbols = spell(list(ll_lens) + list(d_lens))
        if cl_lens is None:
            freq = [0] * 19
            for s, _ in cl_symbols:
                freq[s] += 1
            if sum(1 for f in freq if f) == 1:       # (a code length code of one symbol: give it a partner, the code is complete)
                freq[0 if freq[0] == 0 else 18] += 1
            cl_lens = limited_lens(freq, 7)
        if hclen is None:
            hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
        self.bits(1 if final else 0, 1).bits(2, 2)
        self.bits(((len(ll_lens) if hlit is None else hlit) - 257) & 31, 5)
        self.bits(((len(d_lens) if hdist is None else hdist) - 1) & 31, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl_lens[CL_ORDER[i]], 3)
        cl = canonical_codes(cl_lens)
        for s, run in cl_symbols:
            assert cl[s][1], "no code for code length symbol %d" % s
            self.code(*cl[s])
            if s == 16:
                self.bits(run - 3, 2)
            elif s == 17:
                self.bits(run - 3, 3)
            elif s == 18:
                self.bits(run - 11, 7)
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, cl_lens=None, cl_symbols=None, hclen=None):
        self.header(ll_lens, d_lens, final, cl_lens, cl_symbols, hclen)
        self.symbols(tokens, ll_lens, d_lens)
        self.blocks.append((2, [t[:2] if type(t) is tuple else t for t in tokens], list(ll_lens), list(d_lens)))
        return self

    def auto(self, tokens, final=False, max_len=15, **kw):
        """a dynamic block in a length-limited Huffman code made for its tokens"""
        ll_lens, d_lens = lens_for(tokens, max_len)
        return self.dynamic(tokens, ll_lens, d_lens, final, **kw)
