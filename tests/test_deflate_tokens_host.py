"""tests/deflate_tokens.py, the token-level DEFLATE reader the row kernel's tests judge with, held against streams whose text is
known: zlib's at levels 0 (stored blocks), 1, 6, 9 and with Z_FIXED, and the host row coder's (row_deflate.cpp) on the inputs of
test_row_deflate.py that reach the format's limits -- whose tokens are checked here on the way: a match of exactly 258, one at
exactly 32768, none beyond either."""
import zlib

import numpy as np
import pytest

from midas_amd import abi
from tests import deflate_tokens as DT
from tests.test_row_deflate import rows_of, second_tab, table_rows


def replay(tokens):
    """the text the tokens spell, by the definition of a match"""
    out = bytearray()
    for t in tokens:
        if type(t) is tuple:
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def texts():
    rng = np.random.default_rng(5)
    table = b"".join(table_rows(rng, 3000))
    return {"empty": b"", "one byte": b"x", "table": table, "random": rng.integers(0, 256, 70000).astype(np.uint8).tobytes(),
            "runs": b"a" * 70000 + b"ab" * 400 + bytes(range(256)) * 3,
            "skewed": bytes(rng.choice(np.arange(40, 60), 50000, p=np.array([2.0 ** -min(k + 1, 19) for k in range(19)] + [2.0 ** -19])).astype(np.uint8))}


def check(raw, text):
    p = DT.parse(raw)
    assert p.text == text and p.n_bytes == len(raw)
    assert replay(p.tokens) == text
    assert p.blocks[-1].final and not any(b.final for b in p.blocks[:-1])
    assert p.blocks[0].first_token == 0 and p.blocks[-1].end_token == len(p.tokens)
    for m in p.matches:
        assert 3 <= m[0] <= 258 and 1 <= m[1] <= 32768
    for b in p.blocks:
        if b.kind == 2:
            assert len(b.cl_lens) == 19 and 257 <= len(b.ll_lens) <= 286 and 1 <= len(b.d_lens) <= 30
            assert max(b.cl_lens) <= 7 and max(b.ll_lens) <= 15 and max(b.d_lens) <= 15
            assert DT.kraft(b.cl_lens)[0] == 32768 and DT.kraft(b.ll_lens)[0] == 32768
            k, used = DT.kraft(b.d_lens)
            assert k == 32768 or used <= 1
            # the symbols a block uses have codes, and what the code length symbols spelt is the two vectors
            ll, d = DT.frequencies(p.tokens[b.first_token:b.end_token])
            assert all(b.ll_lens[s] for s in range(len(ll)) if ll[s]) and all(b.d_lens[s] for s in range(30) if d[s])
    return p


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_zlib_streams(level):
    kinds = set()
    for name, text in texts().items():
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = c.compress(text) + c.flush()
        p = check(raw, text)
        kinds |= {b.kind for b in p.blocks}
        if level == 0:
            assert all(type(t) is int for t in p.tokens) and len(p.blocks) >= (len(text) + 65534) // 65535
        if level == 9 and name == "runs":
            assert (258, 1) in p.tokens
    assert kinds == ({0} if level == 0 else {0, 1, 2})       # (the random text goes out stored, the tiny ones fixed)


def test_fixed_blocks_and_a_stream_cut_into_blocks():
    for name, text in texts().items():
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        p = check(c.compress(text) + c.flush(), text)
        assert {b.kind for b in p.blocks} <= {0, 1}
    # sync flushes: empty stored blocks between the others, bits left over before them
    text = texts()["table"]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(c.compress(text[i:i + 9001]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(text), 9001)) + c.flush()
    p = check(raw, text)
    assert sum(b.kind == 0 and b.first_token == b.end_token for b in p.blocks) >= len(text) // 9001
    # what follows the final block is not the reader's
    assert DT.parse(raw + b"\x00trailer").n_bytes == len(raw)


def test_broken_streams_are_refused():
    text = texts()["table"]
    raw = zlib.compress(text, 6)[2:-4]
    with pytest.raises(DT.DeflateError):
        DT.parse(raw[:len(raw) // 2])
    with pytest.raises(DT.DeflateError):
        DT.parse(b"\x07")                                     # block type 3
    with pytest.raises(DT.DeflateError):
        DT.parse(bytes([0x03, 0x02, 0x00]))                   # fixed block, first token a match (3, 1): nothing to reach back into


def test_unconstrained_depths():
    assert DT.huffman_depths([0, 5, 0]) == {1: 1}
    assert DT.huffman_depths([1, 1]) == {0: 1, 1: 1}
    d = DT.huffman_depths([1, 1, 2, 4, 8, 16])
    assert [d[s] for s in range(6)] == [5, 5, 4, 3, 2, 1]
    flat = DT.huffman_depths([7] * 16)
    assert set(flat.values()) == {4}
    # every set of depths of a Huffman tree is a complete code
    rng = np.random.default_rng(2)
    for _ in range(50):
        f = rng.integers(0, 1000, 40).tolist()
        dep = DT.huffman_depths(f)
        if len(dep) > 1:
            assert sum(2.0 ** -v for v in dep.values()) == 1.0
    assert [DT.length_code(l) for l in (3, 10, 11, 12, 13, 257, 258)] == [0, 7, 8, 8, 9, 27, 28]
    assert [DT.distance_code(x) for x in (1, 4, 5, 6, 7, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 28, 29, 29]


def host_case(case):
    rng = np.random.default_rng(7)
    if case == "huge counts":
        lines = [b"c1\t%d\tN\t%d\t%d\t%d\t%d\t%d\n" % (4294967295 - i, 4 * 4294967295 - i, 4294967295, 4294967295 - i, 4294967295, 4294967295)
                 for i in range(2000)]
        tail = second_tab
    elif case == "long ids":
        lines = table_rows(rng, 600, ref_id=b"k" * 259 + b"z" * 259 + b"_" * 182)
        tail = second_tab
    else:
        filler = lambda n: bytes(rng.integers(97, 123, n - 1).astype(np.uint8)) + b"\n"
        t = b"\tA\t33\t33\t0\t0\t0\n"
        lines = [b"q" + t, filler(32768 - len(t) - 1), b"q" + t, filler(32767 - len(t) - 1), b"q" + t, filler(32769 - len(t) - 1), b"q" + t]
        tail = lambda r: 1 if r.startswith(b"q\t") else len(r) - 1
    return lines, rows_of(lines, tail)


@pytest.mark.parametrize("case", ["huge counts", "long ids", "far matches"])
def test_host_row_coder_token_by_token(case):
    lines, (text, rb, tb) = host_case(case)
    p = check(abi.deflate_rows(text, rb, tb), text)
    assert len(p.blocks) == 1 and p.blocks[0].kind == 2
    lengths, dists = [m[0] for m in p.matches], [m[1] for m in p.matches]
    if case == "long ids":         # a 700-byte head that repeats: it goes out in pieces of exactly 258
        assert max(lengths) == 258 and lengths.count(258) >= len(lines) - 1
    if case == "far matches":      # the tail 32768 back is taken, so is the one 32767 back; the one 32769 back cannot be
        t_len = len(b"\tA\t33\t33\t0\t0\t0\n")
        assert (t_len, 32768) in p.matches or any(d == 32768 and l >= t_len for l, d in p.matches)
        assert any(d == 32767 and l >= t_len for l, d in p.matches)
        assert max(dists) == 32768
