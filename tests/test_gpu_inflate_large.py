"""The device inflater (bgzf_inflate.hip) on DEFLATE streams longer than a BGZF block, held to zlib through Context.inflate_blocks:
payloads on both sides of 64 KiB and up to a mebibyte at zlib's levels 0, 1, 6 and 9, 40 000 table rows coded by the writers' own
row coder, matches at distance 32 768 resolved beyond the 64 KiB mark, more matches than the decoder's first-pass room, a run of
more literals than an escape token's 23 bits count (8 MiB of stored bytes: the one limit the decoder had), a 100-byte and a 1 MiB stream as
neighbours in one wavefront, and a truncated stream (a status, not a fault).  Sizes and CRC-32 are checked on
the device against zlib's; the bytes are compared here.  All streams go up in ONE launch, shared by the tests."""
import zlib

import numpy as np
import pytest

from midas_amd import abi

pytestmark = pytest.mark.gpu

LENGTHS = (65535, 65536, 65537, 200000, 1048577)
LEVELS = (0, 1, 6, 9)


def _raw(data: bytes, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def _mixed(n: int, seed: int) -> bytes:
    """n bytes: table-like text, incompressible bytes, four-letter noise and a long run, a quarter each."""
    rng = np.random.default_rng(seed)
    q = n // 4 + 1
    text = b"".join(b"contig_%03d\t%d\tA\t%d\t%d\t0\t0\t%d\n" % (i >> 12, i + 1, int(c), int(c), 0) for i, c in enumerate(rng.integers(0, 90, q // 24 + 1)))
    parts = [text[:q], bytes(rng.integers(0, 256, q, dtype=np.uint8)), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), q)), bytes(q)]
    return b"".join(parts)[:n]


def _table_rows(n_rows: int):
    """Rows as the table writers format them, with the offsets the row coder wants: every row's start and its tail's (the tab in
    front of the allele)."""
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 40, (n_rows, 4))
    out, row_begin, tail_begin = bytearray(), [], []
    for i in range(n_rows):
        row_begin.append(len(out))
        out += b"contig_%d\t%d" % (i // 15000, i % 15000 + 1)
        tail_begin.append(len(out))
        c = counts[i]
        out += b"\t%c\t%d\t%d\t%d\t%d\t%d\n" % (b"ACGT"[i & 3], int(c.sum()), c[0], c[1], c[2], c[3])
    return bytes(out), row_begin, tail_begin


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def inflated(ctx):
    cases, streams, plain = [], [], []
    tiny = bytes(np.random.default_rng(1).integers(97, 101, 100, dtype=np.uint8))
    for n in LENGTHS:
        data = _mixed(n, n)
        for level in LEVELS:
            cases.append("mixed/%d/level%d" % (n, level)); streams.append(_raw(data, level)); plain.append(data)
            if n == 1048577:      # a 100-byte stream next to every 1 MiB one: neighbours in one wavefront
                cases.append("tiny/beside/level%d" % level); streams.append(_raw(tiny, level)); plain.append(tiny)
    text, row_begin, tail_begin = _table_rows(40000)
    cases.append("rows_40000/row_coder"); streams.append(abi.deflate_rows(text, row_begin, tail_begin)); plain.append(text)
    rng = np.random.default_rng(9)
    half = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    far = half * 6                                               # every match at distance 32 768, most of them beyond 64 KiB
    cases.append("far_matches/196608"); streams.append(_raw(far, 9)); plain.append(far)
    tokens = rng.integers(0, 256, (400, 3), dtype=np.uint8)      # a match per three bytes: more tokens than the first pass has room for
    dense = (tokens.tobytes() + tokens[rng.integers(0, 400, 100000)].tobytes())[:300000]
    cases.append("dense_matches/300000"); streams.append(_raw(dense, 6)); plain.append(dense)
    assert len(dense) == 300000
    # one run of literals longer than the 23 bits of an escape token count (2^23 - 1): stored blocks, no match in between
    long_run = bytes(rng.integers(0, 256, (1 << 23) + 4097, dtype=np.uint8))
    cases.append("literal_run/8392705"); streams.append(_raw(long_run, 0)); plain.append(long_run)
    cpos, blob = [], bytearray()
    for s in streams:
        cpos.append(len(blob))
        blob += s
    sizes = [len(p) for p in plain]
    upos = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    out = ctx.inflate_blocks(bytes(blob), cpos, [len(s) for s in streams], upos, sizes, int(sum(sizes)), crc=[zlib.crc32(p) for p in plain])
    return {c: (p, bytes(out[int(u):int(u) + len(p)])) for c, p, u in zip(cases, plain, upos)}


def _same(name, inflated):
    want, got = inflated[name]
    assert len(got) == len(want)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        raise AssertionError("%s: first difference at byte %d of %d" % (name, int(np.nonzero(a != b)[0][0]), len(want)))


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("n", LENGTHS)
def test_payloads_around_and_beyond_64k(inflated, n, level):
    _same("mixed/%d/level%d" % (n, level), inflated)


@pytest.mark.parametrize("level", LEVELS)
def test_a_tiny_stream_beside_a_mebibyte(inflated, level):
    _same("tiny/beside/level%d" % level, inflated)


@pytest.mark.parametrize("name", ["rows_40000/row_coder", "far_matches/196608", "dense_matches/300000", "literal_run/8392705"])
def test_rows_far_matches_and_dense_matches(inflated, name):
    _same(name, inflated)


def test_a_truncated_long_stream_is_a_status(ctx):
    data = _mixed(200000, 200000)
    good = _raw(data, 6)
    for cut in (good[:-1], good[:len(good) // 2]):
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.inflate_blocks(cut, [0], [len(cut)], [0], [len(data)], len(data), crc=[zlib.crc32(data)])
        assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.read_index == 0
    assert bytes(ctx.inflate_blocks(good, [0], [len(good)], [0], [len(data)], len(data), crc=[zlib.crc32(data)])) == data
