"""The device inflater (bgzf_inflate.hip) held to the FORMAT, not to zlib's habits: the hand-built streams of tests/deflate_cases.py
-- code shapes, header spellings, 48-bit matches, token and room edges, stored blocks, the placer's windows; each proved on the host
(tests/test_deflate_writer_host.py) to contain the edge it is named after -- and the streams of a second encoder, libdeflate
(tests/golden/deflate_streams.json).  Sizes and CRC-32 are checked on the device, the bytes here.  Then one malformed stream per
rule of RFC 1951: the verdict is zlib's, the device must answer with a status -- each was traced through bgzf_decode_kernel by
reading before it was run; the line that refuses it stands next to the case in deflate_cases.malformed()."""
import base64
import json
import os
import zlib

import numpy as np
import pytest

from midas_amd import abi
from tests import deflate_cases as DC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def table():
    return [(name, raw, text) for name, raw, text, _ in DC.cases()]


@pytest.fixture(scope="module")
def libdeflate_streams():
    with open(os.path.join(GOLDEN, "deflate_streams.json")) as f:
        streams = json.load(f)["streams"]
    out = []
    for s in streams:
        raw = base64.b64decode(s["raw"])
        out.append(("libdeflate/" + s["name"], raw, zlib.decompress(raw, -15)))       # (the reference is zlib's inflate)
        assert len(out[-1][2]) == s["size"]
    return out


def _place(items, align):
    """the streams back to back in one buffer, stream k at an offset of align(k) mod 4 (filler bytes in between, never zeros)"""
    blob, cpos = bytearray(), []
    for k, (_, raw, _) in enumerate(items):
        while len(blob) % 4 != align(k) % 4:
            blob.append(0xA5)
        cpos.append(len(blob))
        blob += raw
    return bytes(blob), cpos


def _inflate_and_compare(ctx, items, align=lambda k: 0):
    blob, cpos = _place(items, align)
    sizes = [len(text) for _, _, text in items]
    upos = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    out = ctx.inflate_blocks(blob, cpos, [len(raw) for _, raw, _ in items], upos, sizes, int(sum(sizes)), crc=[zlib.crc32(text) for _, _, text in items])
    for k, ((name, _, text), u) in enumerate(zip(items, upos)):
        got = bytes(out[int(u):int(u) + len(text)])
        assert got == text, "%s (stream %d, offset %d mod 4): first difference at %d of %d" % (
            name, k, cpos[k] % 4, next(i for i in range(len(text)) if got[i] != text[i]), len(text))


def test_every_crafted_stream_at_every_alignment(ctx, table):
    """The whole table, four times in one launch: copy a of stream k lies at an offset of (a + k) mod 4 (Bits::open_at reads byte by
    byte up to the first aligned word), short and long streams side by side in every wavefront as the table has them.  The launch's
    last stream ends in a length-3, distance-3 match whose 8-byte load reaches past the inflated bytes."""
    assert len(table) > 160
    items = [c for a in range(4) for c in table]
    assert items[-1][0] == "placer/length_3_distance_3_as_the_last_bytes"
    n = len(table)
    assert all({(a + k) % 4 for a in range(4)} == {0, 1, 2, 3} for k in range(n))
    _inflate_and_compare(ctx, items, lambda k: k // n + k % n)


def test_every_crafted_stream_alone_in_its_wavefront(ctx, table):
    """... and each stream with 63 finished lanes beside it: a stream per wavefront, the other lanes one stored byte each"""
    tiny = ("one stored byte", bytes([1, 1, 0, 0xFE, 0xFF, 0x78]), b"x")
    items = []
    for k, c in enumerate(table):
        lane = (7 * k) % 64
        items += [tiny] * lane + [c] + [tiny] * (63 - lane)
    _inflate_and_compare(ctx, items, lambda k: k % 3)


def test_matches_of_48_bits_beside_one_bit_literals_and_beside_finished_lanes(ctx, table):
    """Matches that take 15 + 5 + 15 + 13 bits each, 220 in a row: a lane that eats a word and a half per step (refill_fast twice a
    step, short_of_words, emergency) -- in a wavefront whose other lanes decode one-bit literals for as long (the common step comes
    every fourth symbol for all of them), and in one whose other lanes are done at once."""
    by_name = {c[0]: c for c in table}
    slow, slow258, ones = by_name["bits/220_matches_of_48_bits"], by_name["bits/220_matches_of_48_bits_length_258"], by_name["bits/one_bit_literals"]
    tiny = ("one stored byte", bytes([1, 1, 0, 0xFE, 0xFF, 0x78]), b"x")
    items = []
    for s, other, lane in ((slow, ones, 17), (slow258, ones, 40), (slow, tiny, 63), (slow258, tiny, 0), (slow258, slow, 5)):
        items += [other] * lane + [s] + [other] * (63 - lane)
    assert len(items) == 5 * 64
    _inflate_and_compare(ctx, items, lambda k: k)


def test_libdeflates_streams(ctx, table, libdeflate_streams):
    """A second encoder's dialect (one dynamic block of 40 000 symbols where zlib writes three): as they are, and all twelve in one
    wavefront next to crafted short streams."""
    assert len(libdeflate_streams) == 12
    _inflate_and_compare(ctx, libdeflate_streams)
    short = [c for c in table if len(c[2]) < 2000][:52]
    assert len(short) == 52
    items = []
    for k in range(64):                           # every fifth lane or so a libdeflate stream, crafted ones in between
        items.append(libdeflate_streams[k // 5] if k % 5 == 2 and k // 5 < 12 else short.pop())
    assert sum(1 for it in items if it[0].startswith("libdeflate/")) == 12 and len(items) == 64
    _inflate_and_compare(ctx, items, lambda k: k)


def test_one_malformed_stream_per_rule_is_a_status(ctx):
    """One call per malformed stream, behind one good stream: zlib refuses it (or does not inflate it to the stated size), so the device
    must raise ERR_BAD_LAYOUT and name stream 1, with the status of the line that was found to refuse it.  And the valid stream with
    garbage behind its final block: zlib's verdict is 'valid', the device delivers its bytes."""
    good, good_text = DC.good_stream()
    bad = DC.malformed()
    assert len(bad) > 35
    for name, raw, ulen, refused_by, _ in bad:
        d = zlib.decompressobj(-15)
        try:
            valid = len(d.decompress(raw)) == ulen and d.eof
        except zlib.error:
            valid = False
        assert not valid, name
        blob, cpos = _place([("good", good, good_text), (name, raw, None)], lambda k: 0)
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.inflate_blocks(blob, cpos, [len(good), len(raw)], [0, len(good_text)], [len(good_text), ulen], len(good_text) + ulen)
        assert ei.value.status == abi.ERR_BAD_LAYOUT and ei.value.read_index == 1, (name, refused_by, ei.value.status, ei.value.read_index, ei.value.message)
        # ... and by the line that reading found: the message names the kernel's status
        assert "code %u)" % DC.status_code(refused_by) in ei.value.message, (name, refused_by, ei.value.message)
    name, raw, text, _ = next(c for c in DC.cases() if c[0].startswith("valid/trailing_garbage"))
    _inflate_and_compare(ctx, [("good", good, good_text), (name, raw, text)])


def test_the_first_pass_room_ends_where_the_model_says(ctx, table, monkeypatch, capfd):
    """The room cases one by one with MIDAS_SNPS_TRACE set: the library says on stderr when streams were decoded again (inflate_again,
    after kMatchRoom), and that must be so for exactly the streams that deflate_cases.token_out_takes -- TokenOut's counters step by
    step -- finds too large for first_pass_room: the last that fits is not decoded again, the first that overflows by one dword is."""
    monkeypatch.setenv("MIDAS_SNPS_TRACE", "1")
    again = {}
    for name, raw, text in table:
        if not name.startswith("room/"):
            continue
        tokens = [t for block in DC.spec(name) for t in block[1]]
        capfd.readouterr()
        _inflate_and_compare(ctx, [(name, raw, text)])
        again[name] = "streams decoded again" in capfd.readouterr().err
        assert again[name] == (not DC.token_out_takes(tokens, DC.first_pass_dwords(len(text)))), (name, DC.room_needed(tokens), DC.first_pass_dwords(len(text)))
    assert len(again) == 17 and sum(again.values()) == 5 + 2
    assert all(again[n] == n.endswith("first_that_overflows") for n in again if "densest" not in n)
