"""The input end of `merge_midas.py snps` on the device (tables_scan.hip, tables_device.hip), held to the host readers:
the row parser on chosen rows against abi.read_snps_table on the same text; whole table sets inflated and parsed on the device
against abi.read_snps_counts, array for array, at every member border, row range and group cap; corrupt and reference-style files
(statuses, naming the file); the merge from the resident set against the merge from host arrays; and the command with
MIDAS_SNPS_MERGE_READERS=device -- alone, with the device writers, with a reference-style table among the samples', and as two
ranks on the one GPU -- against a run with nothing set, byte for byte."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, synth
from midas_amd.merge import snps as msnps

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"ref_id\tref_pos\tref_allele\tdepth\tcount_a\tcount_c\tcount_g\tcount_t\n"


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


# ---- b. the parser kernel on chosen rows ----------------------------------------------------------------------------------------
def _good_rows(n, seed=3):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 300, (n, 4))
    return [b"contig_%d\t%d\t%c\t%d\t%d\t%d\t%d\t%d" % (i // 100, i % 100 + 1, b"ACGT"[i & 3], int(c[i].sum()), c[i, 0], c[i, 1], c[i, 2], c[i, 3])
            for i in range(n)]


def _host_read(tmp_path, text, tag):
    """abi.read_snps_table on the text as a plain gzip file -> (counts, None) or (None, first bad row, 0-based)."""
    path = str(tmp_path / ("%s.snps.gz" % tag))
    with gzip.open(path, "wb", compresslevel=1) as h:
        h.write(text)
    try:
        return abi.read_snps_table(path, want_keys=False)[0], None
    except abi.MidasSnpsError as e:
        m = re.search(r"malformed row (\d+)", e.message)
        assert e.status == abi.ERR_BAD_LAYOUT and m, e.message
        return None, int(m.group(1)) - 1


def _same_as_host(ctx, tmp_path, text, tag):
    want, want_bad = _host_read(tmp_path, text, tag)
    counts, rows, bad = ctx.parse_rows(text, skip_header=True)
    if want_bad is None:
        assert bad == -1 and rows == want.shape[0], (tag, rows, bad, want.shape)
        np.testing.assert_array_equal(counts, want, err_msg=tag)
    else:
        assert bad == want_bad, (tag, bad, want_bad)
    return want, want_bad


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_parser_row_counts(ctx, tmp_path, n):
    rows = _good_rows(n, seed=n)
    for tag, text in (("nl", HEADER + b"".join(r + b"\n" for r in rows)), ("open", HEADER + b"\n".join(rows))):      # the last row with and without a newline
        want, bad = _same_as_host(ctx, tmp_path, text, "rows%d_%s" % (n, tag))
        assert bad is None and want.shape[0] == n
    if n == 0:        # header-only tables: with its newline, without, and no byte at all
        assert _same_as_host(ctx, tmp_path, HEADER[:-1], "header_open")[0].shape[0] == 0
        assert ctx.parse_rows(b"", skip_header=True)[1:] == (0, -1)


CHOSEN = {
    # accepted
    "tabs_7": (b"c\t1\tA\t6\t1\t2\t3\t0", True),
    "tabs_8": (b"c\t1\tA\textra\t6\t1\t2\t3\t0", True),
    "tabs_16": (b"\t".join([b"x"] * 13) + b"\t1\t2\t3\t4", True),
    "zero": (b"c\t1\tA\t0\t0\t0\t0\t0", True),
    "leading_zeros": (b"c\t1\tA\t7\t007\t0\t00\t0000000000000", True),
    "int32_max": (b"c\t1\tA\t9\t2147483647\t0\t0\t2147483647", True),
    "long_ref_id": (b"r" * 400 + b"\t1\tA\t6\t1\t2\t3\t0", True),
    # refused
    "tabs_6": (b"c\t1\t6\t1\t2\t3\t0", False),
    "tabs_17": (b"\t".join([b"x"] * 14) + b"\t1\t2\t3\t4", False),       # fields 13-16, the last one with the rest of the line: a tab in it
    "int32_max_plus_1": (b"c\t1\tA\t9\t1\t2147483648\t0\t0", False),
    "eleven_digits": (b"c\t1\tA\t9\t1\t0\t99999999999\t0", False),
    "plus_sign": (b"c\t1\tA\t9\t+5\t0\t0\t0", False),
    "empty_field": (b"c\t1\tA\t9\t1\t\t0\t0", False),
    "empty_last_field": (b"c\t1\tA\t9\t1\t2\t0\t", False),
    "letter": (b"c\t1\tA\t9\t1\t2\t3x\t0", False),
    "carriage_return": (b"c\t1\tA\t9\t1\t2\t3\t0\r", False),
    "empty_line": (b"", False),
    "space": (b"c\t1\tA\t9\t1\t 2\t3\t0", False),
}


@pytest.mark.parametrize("name", sorted(CHOSEN))
def test_parser_on_chosen_rows(ctx, tmp_path, name):
    """The chosen row at row 70 of 200 (a second wavefront), once more at row 150: the FIRST bad row is reported; and as the last
    row of the table, with and without a newline."""
    row, good = CHOSEN[name]
    rows = _good_rows(200, seed=len(name))
    rows[70] = row
    rows[150] = row
    want, bad = _same_as_host(ctx, tmp_path, HEADER + b"".join(r + b"\n" for r in rows), name)
    assert (bad is None) == good and (good or bad == 70)
    for tag, tail in (("last_nl", b"\n"), ("last_open", b"")):
        if name == "empty_line" and not tail:
            continue          # (an empty last line without a newline is no line)
        text = HEADER + b"".join(r + b"\n" for r in _good_rows(66)) + row + tail
        want, bad = _same_as_host(ctx, tmp_path, text, name + "_" + tag)
        assert (bad is None) == good and (good or bad == 66)


# ---- c. table sets, device against host -----------------------------------------------------------------------------------------
EXTRA = (0, 3, 700, 20000)       # table k holds n + EXTRA[k] rows: the result stops at the shortest


def _write_set(root, n):
    """Four tables of different lengths over three contigs, written at gz_level 0, 1 and 6 by write_table and contig by contig by
    write_rows."""
    rng = np.random.default_rng(n)
    paths = []
    for k, extra in enumerate(EXTRA):
        rows = n + extra
        lens = [rows] if rows < 3 else [rows // 2, rows // 3, rows - rows // 2 - rows // 3]
        ids = ["contig_%d" % (j + 1) for j in range(len(lens))]
        alleles = [rng.choice(np.frombuffer(b"ACGT", np.uint8), l) for l in lens]
        counts = [rng.integers(0, 60, (l, 4)).astype(np.uint32) for l in lens]
        path = os.path.join(root, "n%d_t%d.snps.gz" % (n, k))
        if k < 3:
            abi.write_table(path, ids, alleles, counts, gz_level=(0, 1, 6)[k], threads=2)
        else:
            abi.write_rows(path, False, ids[0], alleles[0], counts[0], gz_level=4, threads=2)
            for j in range(1, len(lens)):
                abi.write_rows(path, True, ids[j], alleles[j], counts[j], gz_level=4, threads=2)
        assert abi.count_snps_rows(path) == rows
        paths.append(path)
    return paths


RANGES = [(0, -1), (0, 1), (16383, 16385), (5, 5), (39999, 40000), (100000, 100010)]


def _device_equals_host(ctx, paths, lo, hi):
    try:
        want = abi.read_snps_counts(paths, lo, hi)
    except abi.MidasSnpsError as e:      # a range that begins behind the shortest table's end: refused, in the same words
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.read_snps_counts_device(paths, lo, hi)
        assert (ei.value.status, ei.value.message) == (e.status, e.message) and "asked of a table that holds fewer" in e.message
        return None
    with ctx.read_snps_counts_device(paths, lo, hi) as tables:
        assert (tables.n_samples, tables.n_rows) == (len(paths), want[0].shape[0]), (lo, hi)
        for k, w in enumerate(want):
            np.testing.assert_array_equal(tables.fetch(k), w, err_msg="table %d rows [%d, %d)" % (k, lo, hi))
        return tables.stats


@pytest.mark.parametrize("cap_kb", [None, 64])
@pytest.mark.parametrize("n", [1, 16383, 16384, 16385, 40000])
def test_table_sets_read_on_the_device_equal_the_host_readers(ctx, tmp_path, monkeypatch, n, cap_kb):
    paths = _write_set(str(tmp_path), n)
    if cap_kb is not None:
        monkeypatch.setenv("MIDAS_SNPS_MERGE_READ_KB", str(cap_kb))
    for lo, hi in RANGES:
        stats = _device_equals_host(ctx, paths, lo, hi)
        if (lo, hi) == (0, -1):
            assert stats["rows"] == n and stats["tables"] == 4
            if n >= 16383:
                assert (stats["groups"] > 4) == (cap_kb is not None), stats      # many groups under the forced cap, single-member ones among them


def test_a_table_written_by_the_batchs_device_writer(ctx, tmp_path):
    table, reads = synth.make_dataset(n_species=1, contigs_per_species=3, contig_len=15000, n_reads=6000, seed=synth.BASE_SEED + 7)
    b = ctx.batch(table, reads)
    b.run(abi.Thresholds.from_args(abi.DEFAULT_ARGS))
    counts, allele, _ = b.fetch()
    dev, host = str(tmp_path / "dev.snps.gz"), str(tmp_path / "host.snps.gz")
    before = ctx.row_coder_counts()
    b.write_part(dev, [0, 1, 2], table.ids, header=True, gz_level=4, threads=2)
    assert ctx.row_coder_counts()["members_on_device"] == before["members_on_device"] + 3      # (it WAS the device's coder)
    b.close()
    off = table.site_offsets()
    abi.write_table(host, table.ids, [allele[off[c]:off[c + 1]] for c in range(3)], [counts[off[c]:off[c + 1]] for c in range(3)], gz_level=4, threads=2)
    for lo, hi in ((0, -1), (14999, 15002)):
        _device_equals_host(ctx, [dev, host], lo, hi)
    with ctx.read_snps_counts_device([dev], 0, -1) as tables:
        np.testing.assert_array_equal(tables.fetch(0), counts)


def _members(raw):
    """(offset, total bytes) of the gzip members this library wrote"""
    out, p = [], 0
    while p < len(raw):
        total = int.from_bytes(raw[p + 16:p + 20], "little")
        out.append((p, total))
        p += total
    return out


def test_corrupt_and_reference_style_tables_are_a_status(ctx, tmp_path):
    """All of them in one process: a byte flipped inside a member's deflate data, a flipped CRC byte in its trailer, a member that
    announces another number of rows than it holds, a malformed row, and a plain gzip file among the tables."""
    paths = _write_set(str(tmp_path), 16385)[:3]
    good = open(paths[1], "rb").read()
    mem = _members(good)
    assert len(mem) >= 4
    at, total = mem[2]

    def damaged(edit, tag):
        raw = bytearray(good)
        edit(raw)
        p = str(tmp_path / (tag + ".snps.gz"))
        open(p, "wb").write(bytes(raw))
        return p

    def flip(i):
        def edit(raw):
            raw[i] ^= 0x20
        return edit

    def rows_announced(raw):
        raw[at + 24:at + 28] = (int.from_bytes(raw[at + 24:at + 28], "little") + 1).to_bytes(4, "little")

    cases = {"deflate": flip(at + 28 + (total - 36) // 2), "crc": flip(at + total - 8), "rows": rows_announced}
    for tag, edit in cases.items():
        bad = damaged(edit, tag)
        with pytest.raises(abi.MidasSnpsError) as ei:
            ctx.read_snps_counts_device([paths[0], bad, paths[2]], 0, -1)
        assert ei.value.status == abi.ERR_BAD_LAYOUT and bad in ei.value.message, (tag, ei.value.message)
        if tag == "crc":
            assert "CRC" in ei.value.message
    # a malformed row: the same first bad row as the host reader's
    rng = np.random.default_rng(1)
    n = 300
    counts = rng.integers(0, 9, (n, 4)).astype(np.uint32)
    p = str(tmp_path / "malformed.snps.gz")
    abi.write_table(p, ["c"], [np.full(n, 65, np.uint8)], [counts], gz_level=0, threads=1)
    raw = bytearray(open(p, "rb").read())
    at = _members(bytes(raw))[1][0] + 28 + 5                 # (level 0: the text lies behind the stored block's five bytes)
    rows = bytes(raw[at:]).split(b"\n")
    spot = at + sum(len(r) + 1 for r in rows[:201]) - 2      # the last digit of row 200
    raw[spot] = ord("x")
    text_lo, text_hi = at, at + sum(len(r) + 1 for r in rows[:n])
    import zlib
    raw[text_hi:text_hi + 4] = zlib.crc32(bytes(raw[text_lo:text_hi])).to_bytes(4, "little")
    open(p, "wb").write(bytes(raw))
    with pytest.raises(abi.MidasSnpsError) as eh:
        abi.read_snps_counts([p], 0, -1)
    with pytest.raises(abi.MidasSnpsError) as ed:
        ctx.read_snps_counts_device([p], 0, -1)
    assert eh.value.message == ed.value.message == "%s: malformed row 201" % p and ed.value.status == abi.ERR_BAD_LAYOUT
    with ctx.read_snps_counts_device([p], 0, 200) as tables:      # (in front of it: fine, as on the host)
        np.testing.assert_array_equal(tables.fetch(0), counts[:200])
    # written like the reference writes them
    plain = str(tmp_path / "plain.snps.gz")
    with gzip.open(plain, "wb") as h:
        h.write(gzip.open(paths[0], "rb").read())
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.read_snps_counts_device([paths[0], plain], 0, -1)
    assert ei.value.status == abi.ERR_UNSUPPORTED and plain in ei.value.message
    _device_equals_host(ctx, paths, 0, -1)                        # the context is as good as before


# ---- d. the merge from the resident set -------------------------------------------------------------------------------------------
def rewrite_as_library_tables(ds, gz_level=1):
    """The dataset's sample tables (written like the reference writes them) written again by this library's writer."""
    for sdir, c in zip(ds['samples'], ds['counts']):
        alleles, counts, off = [], [], 0
        for seq in ds['contig_seqs']:
            alleles.append(np.frombuffer(seq.encode(), np.uint8))
            counts.append(np.ascontiguousarray(c[off:off + len(seq)], np.uint32))
            off += len(seq)
        abi.write_table(os.path.join(sdir, 'snps', 'output', ds['species_id'] + '.snps.gz'), ds['contig_ids'], alleles, counts, gz_level=gz_level, threads=2)


def _mean_depths(ds):
    return [float(open(os.path.join(s, 'snps', 'summary.txt')).read().splitlines()[1].split('\t')[4]) for s in ds['samples']]


def test_merge_from_the_resident_set_equals_the_merge_from_arrays(ctx, tmp_path):
    ds = synth.make_merge_dataset(str(tmp_path / "ds"), n_samples=5, n_sites=40000, seed=23)
    rewrite_as_library_tables(ds)
    paths = [os.path.join(s, 'snps', 'output', 'sp1.snps.gz') for s in ds['samples']]
    arrays = [np.ascontiguousarray(c, np.uint32) for c in ds['counts']]
    mean = _mean_depths(ds)
    prm = abi.MergeParams.from_args(dict(abi.DEFAULT_MERGE_ARGS, snp_type=['any'], site_prev=0.0))
    with ctx.read_snps_counts_device(paths[1:], 0, -1, first_slot=1) as tables:
        tables.set_host(0, arrays[0])
        for k in range(5):
            np.testing.assert_array_equal(tables.fetch(k), arrays[k])
        want, got = ctx.merge_sites(prm, arrays, mean), ctx.merge_sites(prm, tables, mean)
        assert set(want) == set(got)
        for key in want:
            if key != 'kernel_ms':
                np.testing.assert_array_equal(got[key], want[key], err_msg=key)
        files = {}
        for tag, counts in (("arrays", arrays), ("resident", tables)):
            f, d = str(tmp_path / (tag + "_freq.txt")), str(tmp_path / (tag + "_depth.txt"))
            res = ctx.merge_sites_tables(prm, counts, mean, f, d, "site_id\ta\tb\tc\td\te\n", site_id_base=7)
            files[tag] = (open(f, "rb").read(), open(d, "rb").read(), res['n_keep'], res['flag'].tobytes(), res['pooled'].tobytes())
        assert files["arrays"] == files["resident"] and files["arrays"][2] > 30000
        # fewer sites than the set holds rows: a window of it
        tables.n_sites = 12345
        short = ctx.merge_sites(prm, tables, mean)
        for key in ('flag', 'pooled', 'depth', 'minor_count', 'count_samples'):
            np.testing.assert_array_equal(short[key], want[key][..., :12345] if want[key].ndim == 2 and key != 'pooled' else want[key][:12345], err_msg=key)


# ---- e. the command ---------------------------------------------------------------------------------------------------------------
def _tree(d):
    out = {}
    for base, _, files in os.walk(d):
        for f in files:
            out[os.path.relpath(os.path.join(base, f), d)] = open(os.path.join(base, f), "rb").read()
    return out


def test_command_with_the_device_readers(ctx, tmp_path, monkeypatch, capsys):
    from tests.test_gpu_merge_rows import _Shared, command_args
    ds = synth.make_merge_dataset(str(tmp_path / "ds"), n_samples=5, n_sites=6000, seed=11)
    rewrite_as_library_tables(ds)

    def run(tag, readers=None, writers=None):
        out = str(tmp_path / tag)
        args = command_args(monkeypatch, out, ds, '--all_sites')
        for k, v in (('MIDAS_SNPS_MERGE_READERS', readers), ('MIDAS_SNPS_MERGE_WRITERS', writers)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        capsys.readouterr()
        msnps.run_pipeline(args, make_context=lambda: _Shared(ctx))
        return _tree(out), capsys.readouterr().out

    want, log = run("plain")
    assert "sample tables" not in log and len(want["sp1/snps_freq.txt"].splitlines()) == 6001
    for writers in ("host", "device"):
        got, log = run("device_" + writers, "device", writers)
        assert got == want, writers
        assert "sample tables: device readers (4 tables" in log
    # one sample's table as the reference writes it: the host readers, and a line that says so
    p = os.path.join(ds['samples'][2], 'snps', 'output', 'sp1.snps.gz')
    text = gzip.open(p, "rb").read()
    with gzip.open(p, "wb", compresslevel=1) as h:
        h.write(text)
    got, log = run("fallback", "device", "device")
    assert got == want
    assert "sample tables: host readers (" in log and "sp1.snps.gz does not announce its rows)" in log


def test_two_ranks_on_the_one_gpu_with_the_device_readers(tmp_path):
    ds = synth.make_merge_dataset(str(tmp_path / "ds"), n_samples=5, n_sites=6000, seed=11)
    rewrite_as_library_tables(ds)
    env1 = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MIDAS_SNPS_MERGE_READERS", "MIDAS_SNPS_MERGE_WRITERS")}

    def argv(out):
        return [sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'snps', out, '-i', os.path.dirname(ds['samples'][0]), '-t', 'dir', '-d', ds['db'],
                '--all_sites']

    one = str(tmp_path / "one")
    r = subprocess.run(argv(one), capture_output=True, text=True, cwd=ROOT, env=env1, timeout=300)
    assert r.returncode == 0, r.stderr
    two = str(tmp_path / "two")
    procs = [subprocess.Popen(argv(two), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT,
                              env=dict(env1, RANK=str(k), LOCAL_RANK="0", WORLD_SIZE="2", MIDAS_SNPS_MERGE_READERS="device", MIDAS_SNPS_MERGE_WRITERS="device"))
             for k in range(2)]
    logs = []
    for p in procs:
        o, e = p.communicate(timeout=300)
        assert p.returncode == 0, e
        logs.append(o)
    assert all("sample tables: device readers" in o and "rows " in o for o in logs), logs
    assert _tree(os.path.join(two, 'sp1')) == _tree(os.path.join(one, 'sp1'))
