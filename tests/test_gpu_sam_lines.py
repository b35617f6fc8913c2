"""The device SAM decode (midas_amd/csrc/sam_scan.hip) on the chosen lines of tests/sam_cases.py, in its three forms -- the sorted
columns (midas_sam_load_device), the file-order columns (midas_sam_load_device_order) and the resident layout
(midas_sam_load_resident): every accepted case against the case's literals and against tests/sam_model.py, column for column;
every refused case as ERR_BAD_LAYOUT naming its line and its reason, whatever chunk met the line; one file decoded with the chunk
end on every byte of one of its lines; headers of 1 .. 65537 references."""
import numpy as np
import pytest

from midas_amd import abi
from tests import sam_cases as SC
from tests import sam_model
from tests.sam_model import assert_columns_equal, reads_columns
from tests.test_genes_sam_host import file_order_columns
from tests.test_gpu_sam_resident import resident_columns

pytestmark = pytest.mark.gpu
CASES = SC.cases()
ACCEPTED = [c for c in CASES if c.refused is None]
REFUSED = [c for c in CASES if c.refused is not None]
CHUNK = "MIDAS_SNPS_SAM_CHUNK_BYTES"
SMALLEST = "16"                       # the least the decoder takes: under every line here but the empty one, so it has to grow


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def _columns(ctx, path, form):
    """(names, lens, columns) of one device form"""
    if form == "resident":
        return resident_columns(ctx, path)
    names, lens, refid, reads = abi.read_sam(path, ctx, order="file") if form == "file" else abi.read_sam(path, ctx)
    assert reads.device is not None and reads.seq4.size == 0
    return names, lens, reads_columns(refid, ctx.fetch_payload(reads))


FORMS = ("columns", "file", "resident")


def _expected(data):
    """The model's word on `data`: names, lens, the sorted columns, the file-order columns, and whether the two are the same"""
    names, lens, sorted_cols = sam_model.decode(data)
    _, _, file_cols = file_order_columns(data)
    same = all(np.array_equal(sorted_cols[k], file_cols[k]) for k in sam_model.COLUMNS)
    return names, lens, sorted_cols, file_cols, same


def _check(ctx, path, exp, case=None, forms=FORMS, what=""):
    names, lens, sorted_cols, file_cols, same = exp
    for form in forms:
        gn, gl, got = _columns(ctx, path, form)
        assert gn == names and gl == lens, (what, form)
        assert_columns_equal(got, file_cols if form == "file" else sorted_cols, "%s, %s" % (what, form))
        if case is not None and (form != "file" or same):
            SC.assert_literals(got, case)


def _write(tmp_path, data):
    path = str(tmp_path / "x.sam")
    with open(path, "wb") as f:
        f.write(data)
    return path


# ---- accepted ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACCEPTED, ids=[c.name for c in ACCEPTED])
def test_an_accepted_case_decodes_to_its_literals_in_every_form(ctx, tmp_path, monkeypatch, case):
    data = SC.data(case)
    path = _write(tmp_path, data)
    exp = _expected(data)
    _check(ctx, path, exp, case, what=case.name)
    if len(data) < 4096:              # the records of a small case in chunks of a line or two: the same columns, ties in file order
        monkeypatch.setenv(CHUNK, SMALLEST)
        _check(ctx, path, exp, case, forms=FORMS if case.name.startswith("ties/") else ("columns",), what=case.name + ", smallest chunk")


def test_the_accepted_lines_in_one_file(ctx, tmp_path, monkeypatch):
    data = SC.accepted_file()
    path = _write(tmp_path, data)
    exp = _expected(data)
    assert not exp[4] and len(exp[2]["refid"]) > 80
    _check(ctx, path, exp, what="accepted file")
    monkeypatch.setenv(CHUNK, "300")                 # a line or two a chunk; the 131 kB line makes it grow on the way
    _check(ctx, path, exp, what="accepted file, 300-byte chunks")


# ---- refused -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", REFUSED, ids=[c.name for c in REFUSED])
def test_a_refused_case_names_its_line_and_its_reason(ctx, tmp_path, monkeypatch, case):
    path = _write(tmp_path, SC.data(case))
    line, why = case.refused
    bad = case.lines[line - SC.FIRST]
    seen = []
    for chunk in (None, SMALLEST):
        if chunk:
            assert int(chunk) < len(bad) or len(bad) <= 2       # (smaller than the bad line, but for the empty line)
            monkeypatch.setenv(CHUNK, chunk)
        for kw in (dict(), dict(resident=True), dict(order="file")):
            with pytest.raises(abi.MidasSnpsError) as ei:
                abi.read_sam(path, ctx, **kw)
            assert ei.value.status == abi.ERR_BAD_LAYOUT, (kw, chunk, ei.value.message)
            assert "line %d:" % line in ei.value.message and SC.REASON_TEXT[why] in ei.value.message, (kw, chunk, ei.value.message)
            seen.append(ei.value.message)
    assert len(set(seen)) == 1, seen                             # one text whatever form and chunk met the line


# ---- the chunk end on every byte of a line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_the_chunk_end_on_every_byte_of_a_line(ctx, tmp_path, monkeypatch, eol):
    data, starts = SC.sweep_file(eol)
    path = _write(tmp_path, data)
    exp = _expected(data)
    _check(ctx, path, exp, what="whole file")
    k = 6
    # the first chunk is the body's first `size` bytes: its end falls on each byte of line k, on its '\r', on its '\n', on the first
    # byte of line k + 1 and on the one behind it
    sizes = list(range(starts[k], starts[k + 1] + 3))
    assert data[len(SC.HEAD) + sizes[-3] - len(eol):][:len(eol)] == eol and len(sizes) > 40
    for size in sizes:
        monkeypatch.setenv(CHUNK, str(size))
        _check(ctx, path, exp, forms=("columns",), what="chunk %d" % size)
    for size in (sizes[0], sizes[len(sizes) // 2], sizes[-1]):
        monkeypatch.setenv(CHUNK, str(size))
        _check(ctx, path, exp, forms=("file", "resident"), what="chunk %d" % size)


# ---- reference counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ref", SC.REF_COUNTS)
def test_reference_counts_around_the_second_sorts_bits(ctx, tmp_path, n_ref):
    case = SC.reference_count_case(n_ref)
    data = SC.data(case)
    path = _write(tmp_path, data)
    exp = _expected(data)
    assert len(exp[0]) == n_ref
    _check(ctx, path, exp, case, forms=("columns", "resident"), what=case.name)
