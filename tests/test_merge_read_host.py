"""The device readers of `merge_midas.py snps` from the host's side (no GPU): the entry points are declared, exported and bound;
with MIDAS_SNPS_MERGE_READERS=device load_sample_tables sends the first sample's table to the host reader and the others to the
context's device method, and it takes the host readers -- with one line that says why -- when the context has no such method, when
there is one sample, and when a table is written like the reference writes them."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from midas_amd import abi, build, synth
from midas_amd.merge import snps as msnps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['midas_merge_tables_create', 'midas_merge_tables_free', 'midas_merge_tables_shape', 'midas_merge_tables_set_host', 'midas_merge_tables_fetch',
       'midas_snps_tableset_read_counts_device', 'midas_snps_parse_rows_device', 'midas_merge_sites_resident', 'midas_merge_sites_tables_resident']


def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midas_snps.h")).read(), flags=re.S)
    build.build_native()
    raw = C.CDLL(build.LIB_PATH)
    lib = abi.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(raw, sym)
        assert getattr(lib, sym).argtypes[0] is C.c_void_p
    assert callable(abi.Context.read_snps_counts_device) and callable(abi.Context.parse_rows) and callable(abi.MergeTables.set_host)
    blob = open(build.LIB_PATH, "rb").read()
    assert b"tables_parse_kernel" in blob and b"tables_count_kernel" in blob and b"tables_ends_kernel" in blob


def test_environment_switches_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "MIDAS_SNPS_MERGE_READERS" in doc and "MIDAS_SNPS_MERGE_READ_KB" in doc


class _Species:
    def __init__(self, ds):
        self.id = ds['species_id']
        self.samples = [type("S", (), {"dir": d})() for d in ds['samples']]


class _Tables(abi.MergeTables):
    """What read_snps_counts_device hands back, without a device: the rows the host reader finds."""
    def __init__(self, arrays, first_slot):
        self.n_samples, self.n_rows, self.n_sites = first_slot + len(arrays), arrays[0].shape[0], arrays[0].shape[0]
        self.slots = dict((first_slot + k, a) for k, a in enumerate(arrays))
        self.stats, self.ms, self.closed = dict(members=len(arrays), groups=1), {}, False

    def set_host(self, sample, counts):
        self.slots[sample] = np.asarray(counts)

    def close(self):
        self.closed = True

    __del__ = close


class _Recording:
    def __init__(self):
        self.calls = []

    def read_snps_counts_device(self, paths, row_begin=0, max_rows=-1, first_slot=0, extra_slots=0):
        self.calls.append((list(paths), row_begin, max_rows, first_slot))
        return _Tables(abi.read_snps_counts(list(paths), row_begin, max_rows), first_slot)


@pytest.fixture()
def dataset(tmp_path):
    ds = synth.make_merge_dataset(str(tmp_path / "ds"), n_samples=3, n_sites=700, seed=4)
    for sdir, c in zip(ds['samples'], ds['counts']):      # the library's own tables: they announce their rows
        alleles, counts, off = [], [], 0
        for seq in ds['contig_seqs']:
            alleles.append(np.frombuffer(seq.encode(), np.uint8))
            counts.append(np.ascontiguousarray(c[off:off + len(seq)], np.uint32))
            off += len(seq)
        abi.write_table(os.path.join(sdir, 'snps', 'output', 'sp1.snps.gz'), ds['contig_ids'], alleles, counts, gz_level=1, threads=1)
    return ds


ARGS = {'max_sites': float('Inf'), 'threads': 1}


def test_first_table_to_the_host_reader_the_rest_to_the_device(dataset, monkeypatch, capsys):
    monkeypatch.setenv('MIDAS_SNPS_MERGE_READERS', 'device')
    host_reads = []
    real = abi.read_snps_table
    monkeypatch.setattr(abi, 'read_snps_table', lambda path, *a, **k: (host_reads.append(path), real(path, *a, **k))[1])
    ctx = _Recording()
    sp = _Species(dataset)
    paths = msnps._table_paths(sp)
    for row_range, lo, hi in ((None, 0, -1), ((100, 450), 100, 450)):
        host_reads.clear(); ctx.calls.clear()
        counts, keys, key_off = msnps.load_sample_tables(sp, ARGS, row_range, ctx)
        assert host_reads == [paths[0]]
        assert ctx.calls == [(paths[1:], lo, hi, 1)]
        assert isinstance(counts, abi.MergeTables) and counts.n_samples == 3 and counts.n_sites == (700 if row_range is None else 350)
        want = [np.asarray(c, np.uint32)[lo:(700 if hi < 0 else hi)] for c in dataset['counts']]
        for k in range(3):
            np.testing.assert_array_equal(counts.slots[k], want[k])
        assert len(key_off) == counts.n_sites + 1 and bytes(keys[:int(key_off[1])]).decode() == dataset['keys'][lo]
        assert "sample tables: device readers (2 tables" in capsys.readouterr().out
    # nothing set: the host readers, silently
    monkeypatch.delenv('MIDAS_SNPS_MERGE_READERS')
    ctx.calls.clear()
    counts, _, _ = msnps.load_sample_tables(sp, ARGS, None, ctx)
    assert isinstance(counts, list) and not ctx.calls and "sample tables" not in capsys.readouterr().out


def test_fallbacks_name_their_reason(dataset, monkeypatch, capsys):
    monkeypatch.setenv('MIDAS_SNPS_MERGE_READERS', 'device')
    sp = _Species(dataset)
    want = [np.asarray(c, np.uint32) for c in dataset['counts']]

    def host_path(ctx, species, reason):
        counts, keys, key_off = msnps.load_sample_tables(species, ARGS, None, ctx)
        assert isinstance(counts, list) and len(counts) == len(species.samples)
        for a, b in zip(counts, want):
            np.testing.assert_array_equal(a, b)
        out = capsys.readouterr().out
        assert out.count("sample tables: host readers (") == 1 and reason in out, out

    host_path(object(), sp, "the context has no device readers")              # the tests' CPU doubles
    one = _Species(dataset)
    one.samples = one.samples[:1]
    ctx = _Recording()
    host_path(ctx, one, "one sample")
    # a table written like the reference writes them
    p = msnps._table_paths(sp)[1]
    text = gzip.open(p, "rb").read()
    with gzip.open(p, "wb", compresslevel=1) as h:
        h.write(text)
    host_path(ctx, sp, "does not announce its rows")
    assert not ctx.calls

    class Refusing(_Recording):       # (a device method that finds it out by itself)
        def read_snps_counts_device(self, paths, *a, **k):
            raise abi.MidasSnpsError(abi.ERR_UNSUPPORTED, "%s: the file does not announce its rows" % paths[0])
    monkeypatch.setattr(abi, 'count_snps_rows', lambda path: 1)
    host_path(Refusing(), sp, "does not announce its rows")
