"""tests/deflate_writer.py and the case table tests/deflate_cases.py, held on the host before the device sees them
(tests/test_gpu_inflate_format.py runs the same table): every crafted stream inflates under zlib to the text its tokens spell, the
token reader finds in it exactly the tokens, block kinds and code lengths the writer was asked for, and the case's CLAIM holds --
the predicate that proves the stream contains the edge it is named after.  Every malformed stream is one zlib refuses, for the
reason the case is named after.  And the committed libdeflate streams (tests/golden/make_deflate_streams.py) inflate under zlib and
show that encoder's dialect."""
import base64
import json
import os
import zlib

import pytest

from tests import deflate_cases as DC
from tests import deflate_tokens as DT
from tests import deflate_writer as DW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def zlib_verdict(raw, ulen):
    """(a complete stream of exactly ulen bytes?, the bytes, zlib's error or None)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error as e:
        return False, b"", str(e)
    return d.eof and len(out) == ulen, out, None


def test_the_writers_code_lengths():
    chain = DW.chain_lens(list(range(16)), 30)
    assert sorted(l for l in chain if l) == list(range(1, 16)) + [15] and DT.kraft(chain) == (32768, 16)
    assert DT.kraft(DW.equal_lens(list(range(64)), 286)) == (32768, 64)
    for n in (286, 30, 19, 257):
        full = DW.full_lens(n)
        assert all(full) and len(full) == n and DT.kraft(full) == (32768, n)
    skew = [1 << min(k, 40) for k in range(60)] + [0, 0, 7]
    for limit in (15, 9, 7, 6):
        lens = DW.limited_lens(skew, limit)
        assert max(lens) == limit and DT.kraft(lens) == (32768, 61) and lens[60] == lens[61] == 0
    assert DW.limited_lens([0, 5, 0]) == [0, 1, 0]
    # canonical codes: the RFC's own example (3.2.2): lengths 3, 3, 3, 3, 3, 2, 4, 4 -> 010, 011, 100, 101, 110, 00, 1110, 1111
    assert DW.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    lens = [0] * 140 + [3] * 9 + [0] * 4 + [7, 7, 7] + [0, 0]
    spelt, at = DW.spell(lens), []
    for s, run in spelt:
        at += [at[-1]] * run if s == 16 else [0] * run if s > 16 else [s]
    assert at == lens and [s for s, _ in spelt] == [18, 0, 0, 3, 16, 3, 3, 17, 7, 7, 7, 0, 0]
    assert DW.expected_text([97, 98, (5, 2), (3, 7), 99]) == b"abababaabac"
    assert DW.Writer().bits(5, 3).bits(1, 1).bits(0x1F, 5).getvalue() == bytes([0xFD, 0x01])      # first bit lowest
    assert DW.Writer().code(0b110, 3).getvalue() == bytes([0b011])                                 # a code's first bit first


def test_every_case_is_the_stream_it_says_it_is():
    cases = DC.cases()
    assert len(cases) > 160 and len({c[0] for c in cases}) == len(cases)
    for group in ("shape/", "header/", "bits/", "tokens/", "stored/", "room/", "placer/", "valid/"):
        assert any(c[0].startswith(group) for c in cases), group
    for name, raw, text, claim in cases:
        ok, out, err = zlib_verdict(raw, len(text))
        assert ok and out == text, (name, err)
        p = DT.parse(raw)
        assert p.text == text, name
        assert p.n_bytes == len(raw) or name.startswith("valid/trailing_garbage"), name
        want = DC.spec(name)
        assert [b.kind for b in p.blocks] == [w[0] for w in want], name
        assert p.blocks[-1].final and not any(b.final for b in p.blocks[:-1]), name
        for b, (kind, tokens, ll_lens, d_lens) in zip(p.blocks, want):
            assert p.tokens[b.first_token:b.end_token] == tokens, name
            if kind == 2:
                assert b.ll_lens == ll_lens and b.d_lens == d_lens, name
        assert DW.expected_text(p.tokens) == text, name
        assert claim(p), "%s: the stream does not contain what it is named after" % name
    assert DC.distance_32769_cannot_be_spelt()
    with pytest.raises(AssertionError):
        DT.distance_code(32769)


def test_the_stream_with_garbage_behind_it_is_valid_to_zlib():
    name, raw, text, _ = next(c for c in DC.cases() if c[0].startswith("valid/trailing_garbage"))
    d = zlib.decompressobj(-15)
    assert d.decompress(raw) == text and d.eof and len(d.unused_data) >= 8
    assert DT.parse(raw).n_bytes == len(raw) - len(d.unused_data)


def test_every_malformed_stream_is_one_zlib_refuses_for_that_reason():
    bad = DC.malformed()
    assert len(bad) > 35 and len({b[0] for b in bad}) == len(bad)
    assert set(DC.ZLIB_SAYS) <= {b[0] for b in bad}
    for name, raw, ulen, refused_by, says in bad:
        ok, out, err = zlib_verdict(raw, ulen)
        assert not ok, name
        assert (err is None) if says is None else (err is not None and says in err), (name, err)
        assert DC.status_code(refused_by) in range(1, 9) and refused_by.count("->") == 1, name     # (ONE line of the kernel, and its status)
    good, text = DC.good_stream()
    assert zlib_verdict(good, len(text)) == (True, text, None)


def test_libdeflates_streams_inflate_under_zlib_and_show_its_dialect():
    with open(os.path.join(GOLDEN, "deflate_streams.json")) as f:
        streams = json.load(f)["streams"]
    assert len(streams) == 12 and os.path.getsize(os.path.join(GOLDEN, "deflate_streams.json")) <= 256 * 1024
    longest, kinds = 0, set()
    for s in streams:
        raw = base64.b64decode(s["raw"])
        ok, out, err = zlib_verdict(raw, s["size"])
        assert ok and zlib.crc32(out) == s["crc32"] and 8 * 1024 <= s["size"] <= 48 * 1024, (s["name"], err)
        p = DT.parse(raw)
        assert p.text == out and p.n_bytes == len(raw), s["name"]
        kinds |= {b.kind for b in p.blocks}
        longest = max([longest] + [b.end_token - b.first_token + 1 for b in p.blocks if b.kind != 0])
    assert longest > 16383          # (zlib ends a block after 16 383 symbols: lit_bufsize - 1 at memLevel 8)
    assert 0 in kinds and 2 in kinds
