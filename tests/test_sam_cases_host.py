"""tests/sam_cases.py held to itself and to the model, without a device: the colliding names collide, tests/sam_model.py decodes
every accepted case to the literals the case wrote down and refuses every refused case at its line for its reason, and the table
really covers what it says -- every reason sam_reason() of sam_scan.hip can word, every CIGAR offset the stride cases are named
after (computed from their text)."""
import os
import re

import numpy as np
import pytest

from tests import sam_cases as SC
from tests import sam_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = SC.cases()
ACCEPTED = [c for c in CASES if c.refused is None]
REFUSED = [c for c in CASES if c.refused is not None]


def test_the_table_is_well_formed():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert all((c.expect is None) != (c.refused is None) for c in CASES)
    assert all(isinstance(c, SC.Case) and isinstance(l, bytes) for c in CASES for l in c.lines)       # plain cases: none carries a mark
    assert len(ACCEPTED) >= 60 and len(REFUSED) >= 60
    assert SC.HEAD.count(b"\n") + 1 == SC.FIRST and len(SC.NAMES) == 16 == len(set(SC.NAMES))


def test_no_test_of_the_cases_is_skipped_or_expected_to_fail():
    marks = ("mark." + "skip", "mark." + "xfail", "pytest." + "skip(", "pytest." + "xfail(", "import" + "orskip")
    for f in ("test_sam_cases_host.py", "test_gpu_sam_lines.py", "sam_cases.py"):
        text = open(os.path.join(ROOT, "tests", f)).read()
        assert not [m for m in marks if m in text], f


def test_the_colliding_names_collide():
    assert SC.fnv1a(b"") == 0x811C9DC5 and SC.fnv1a(b"a") == 0xE40C292C and SC.fnv1a(b"foobar") == 0xBF9CF968      # the published vectors
    (a, b), (c, d) = SC.COLLIDING
    assert SC.fnv1a(a) == SC.fnv1a(b) == 0x016C7ABD and a != b and len(a) == len(b)
    assert SC.fnv1a(c) == SC.fnv1a(d) == 0x009D3086 and (len(c), len(d)) == (8, 7)
    assert all(n in SC.NAMES for n in (a, b, c, d))
    others = [SC.fnv1a(n) for n in SC.NAMES if n not in (a, b, c, d)]
    assert len(set(others)) == len(others) == 12 and not set(others) & {0x016C7ABD, 0x009D3086}
    # in the sorted hashes the second name of each pair stands behind the first: a record on it walks the run of equal hashes
    assert SC.NAMES.index(a) < SC.NAMES.index(b) and SC.NAMES.index(c) < SC.NAMES.index(d)


@pytest.mark.parametrize("case", ACCEPTED, ids=[c.name for c in ACCEPTED])
def test_the_model_decodes_an_accepted_case_to_its_literals(case):
    names, lens, cols = sam_model.decode(SC.data(case))
    assert [n.encode("latin-1") for n in names] == SC.NAMES and lens == SC.LENS
    SC.assert_literals(cols, case)
    assert all(len(cols[k]) == len(cols["refid"]) for k in ("pos", "mapq", "flag", "nm", "l_seq"))


@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_the_model_refuses_a_refused_case_at_its_line(case):
    with pytest.raises(sam_model.SamError) as ei:
        sam_model.decode(SC.data(case))
    assert (ei.value.line, ei.value.why) == case.refused
    # the lines in front of the bad one are good ones: alone they decode
    n_before = case.refused[0] - SC.FIRST
    assert len(sam_model.decode(case.head + b"".join(case.lines[:n_before]))[2]["refid"]) == n_before


def test_every_reason_of_the_decoder_is_some_cases_reason():
    src = open(os.path.join(ROOT, "midas_amd", "csrc", "sam_scan.hip")).read()
    body = src[src.index("const char* sam_reason("):]
    body = body[:body.index("\n}\n")]
    worded = re.findall(r'case kSam\w+: return "([^"]*)";', body)
    assert len(worded) >= 11 and len(set(worded)) == len(worded)
    assert sorted(worded) == sorted(SC.REASON_TEXT.values())
    stated = {c.refused[1] for c in REFUSED}
    assert stated == set(SC.REASON_TEXT)


def test_the_literal_seq_table_is_the_models():
    case = [c for c in ACCEPTED if c.name == "seq/every byte value"][0]
    seq = case.lines[0].split(b"\t")[9]
    assert seq == SC.ALL_BYTES_SEQ and len(seq) == 254 and set(range(256)) - set(seq) == {9, 10} and seq[-1] != 13 and 13 in seq
    cols = sam_model.decode(SC.data(case))[2]
    nibbles = np.stack([cols["seq4"] >> 4, cols["seq4"] & 15], axis=1).ravel().tolist()
    assert nibbles == [SC.SEQ_CODE[b] for b in seq]
    assert len(SC.SEQ_CODE) == 256 and cols["qual"].tolist() == [(i % 94) for i in range(254)]
    # the table against the rule's own words: "=ACMGRSVTWYHKDBN" -> 0..15, either case, any other byte 15
    for b in range(256):
        ch = chr(b)
        want = "=ACMGRSVTWYHKDBN".index(ch.upper()) if b < 128 and ch.upper() in "=ACMGRSVTWYHKDBN" else 15
        assert SC.SEQ_CODE[b] == want, b
    l_seqs = sorted(c.expect["l_seq"][0] for c in ACCEPTED if c.name.startswith("seq/l_seq "))
    assert l_seqs == [1, 2, 63, 64, 65, 127, 128, 129]
    for c in ACCEPTED:
        if c.name.startswith("seq/l_seq ") and c.expect["l_seq"][0] & 1:
            assert c.expect["seq4"][-1] & 15 == 0            # the pad nibble


def _digit_runs(text):
    """[(first offset, last offset)] of the runs of digits in a CIGAR text"""
    return [(m.start(), m.end() - 1) for m in re.finditer(rb"[0-9]+", text)]


def test_the_stride_cases_sit_where_their_names_say():
    texts = {name: SC.cigar_text(pairs) for name, pairs in SC.STRIDE_PAIRS.items()}
    for name, text in texts.items():           # the case's line holds this very text, its literals these very pairs
        case = [c for c in ACCEPTED if c.name == name][0]
        assert case.lines[0].split(b"\t")[5] == text
        assert case.expect["cigar"] == [l << 4 | "MIDNSHP=X".index(op) for l, op in SC.STRIDE_PAIRS[name]]
        assert re.fullmatch(rb"([0-9]+[MIDNSHP=X])+", text) and all(l < 1 << 28 for l, _ in SC.STRIDE_PAIRS[name])
    letters_at = lambda off: {chr(t[off]) for t in texts.values() if len(t) > off and not chr(t[off]).isdigit()}
    for off in (63, 64, 127, 128):
        assert letters_at(off), "no op letter at text offset %d" % off
    runs = [(a, b, name) for name, t in texts.items() for a, b in _digit_runs(t)]
    assert any(a <= 63 and b >= 64 for a, b, _ in runs) and any(a <= 127 and b >= 128 for a, b, _ in runs)
    assert any(a <= 63 and b >= 64 and b - a + 1 == 9 for a, b, _ in runs)
    assert any(b == 63 and b - a + 1 == 9 for a, b, _ in runs)            # a letter at lane 0 with nine digits in the stride before
    assert {63, 64, 65, 128, 129} <= {len(t) for t in texts.values()}
    first = set().union(*[letters_at(off) for off in range(64, 640, 64)])
    last = set().union(*[letters_at(off) for off in range(63, 640, 64)])
    assert first == set("MIDNSHP=X") == last
    widths = {b - a + 1 for a, b, _ in runs}
    assert set(range(1, 10)) <= widths                                     # every digit count a length under 2^28 can have


def test_the_number_ladders_hold_every_rung():
    for field in ("flag", "pos", "mapq"):
        top = dict(flag=65535, pos=2147483647, mapq=255)[field]
        names = {c.name for c in CASES if c.name.startswith("num/%s/" % field)}
        for rung in ("0%d" % top, "forty zeros then 16", str(top + 1), "4294967296", "4294967297", "18446744073709551616",
                     "18446744073709551617", "'+16'", "'-0'", "'1 6'", "''"):
            assert "num/%s/%s" % (field, rung) in names, (field, rung)


@pytest.mark.parametrize("n_ref", SC.REF_COUNTS)
def test_the_reference_count_cases(n_ref):
    case = SC.reference_count_case(n_ref)
    names, lens, cols = sam_model.decode(SC.data(case))
    assert len(names) == n_ref and names[-1] == "r%d" % (n_ref - 1)
    SC.assert_literals(cols, case)
    on = sorted(set(case.expect["refid"]))
    assert on == sorted({r for r in (0, 1, 255, 256, 65535, 65536, n_ref - 1) if r < n_ref}) and on[0] == 0 and on[-1] == n_ref - 1
    written = [int(l.split(b"\t")[2][1:]) for l in case.lines]
    assert written == sorted(written, reverse=True)                        # descending in the file


def test_the_accepted_file():
    data = SC.accepted_file()
    assert data == SC.accepted_file() and data.startswith(SC.HEAD)
    body = data[len(SC.HEAD):]
    lines = body.split(b"\n")[:-1]
    assert 80 < len(lines) < 300
    for c in ACCEPTED:
        for l in c.lines:
            assert l.rstrip(b"\n") in lines or l.rstrip(b"\r\n") + b"\r" in lines, c.name
    cols = sam_model.decode(data)[2]
    kept = sum(1 for l in lines if l.split(b"\t")[2] != b"*")
    assert len(cols["refid"]) == kept
    key = cols["refid"].astype(np.int64) << 32 | (cols["pos"].astype(np.int64) + 1)
    assert (np.diff(key) >= 0).all() and (np.diff(key) == 0).sum() > 50        # sorted, with many ties: their order is the file's


def test_the_sweep_files():
    (lf, starts), (crlf, starts2) = SC.sweep_file(b"\n"), SC.sweep_file(b"\r\n")
    assert len(starts) == 13 == len(starts2) and 500 <= starts[-1] <= 700
    assert lf[len(SC.HEAD) + starts[6]:].startswith(b"read_06:lane1\t") and crlf[len(SC.HEAD) + starts2[6]:].startswith(b"read_06:lane1\t")
    a, b = sam_model.decode(lf)[2], sam_model.decode(crlf)[2]
    sam_model.assert_columns_equal(a, b, "line ends")
    assert len(a["refid"]) == 11 and (np.diff(a["refid"]) >= 0).all() and len(set(a["refid"].tolist())) >= 5
