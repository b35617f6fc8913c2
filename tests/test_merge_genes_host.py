"""`merge_midas.py genes` without a GPU: the repr formatter, both native readers, the key-sequence reuse, the CLI's
arguments and error exits, and the whole command against tests/golden/merge_genes_vectors.json (the reference's own
output) with a numpy double of the device merge injected through run_pipeline's make_context."""
import gzip
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from tests import genes_merge_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()


def _doubles():
    rng = np.random.default_rng(7)
    parts = [rng.integers(0, 1 << 64, 400000, dtype=np.uint64, endpoint=False).view(np.float64),
             rng.integers(1, 1 << 52, 50000, dtype=np.uint64).view(np.float64),              # subnormals
             rng.integers(0, 1 << 53, 100000, dtype=np.int64).astype(np.float64),           # integers to 2^53
             rng.random(100000) * 10.0 ** rng.integers(-6, 18, 100000),
             np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 5e-324, 1e-5, 1e16, 1e-4, 9.999999999999999e15, 0.1, 1.0])]
    tens = np.array([float('1e%d' % k) for k in range(-323, 309)])
    parts += [tens, np.nextafter(tens, np.inf), np.nextafter(tens, -np.inf), -tens]
    base = np.concatenate(parts)
    return np.concatenate([base, -rng.permutation(base)[:1000000 - base.shape[0]]]) if base.shape[0] < 1000000 else base


def test_repr_formatter_is_pythons_repr():
    v = _doubles()
    assert v.shape[0] >= 1000000
    got = abi.format_repr_f64(v)
    exp = [repr(float(x)) for x in v]
    bad = [(e, g) for e, g in zip(exp, got) if e != g]
    assert len(got) == len(exp) and not bad, bad[:10]


def _python_parse(data):
    """utility.parse_file under Python 3 (universal newlines) -> (header, rows as dicts)."""
    f = io.TextIOWrapper(io.BytesIO(data))
    fields = next(f).rstrip('\n').split('\t')
    rows = []
    for line in f:
        values = line.rstrip('\n').split('\t')
        if len(values) == len(fields):
            rows.append(dict(zip(fields, values)))
    return fields, rows


@pytest.mark.parametrize("pid", ['75', '80', '85', '90', '95', '99'])
def test_cluster_map_reader_matches_python(tmp_path, pid):
    for sp in VEC['species']:
        path = str(tmp_path / ('%s.gene_info.txt.gz' % sp['id']))
        with gzip.open(path, 'wb') as h:
            h.write(sp['gene_info'].encode())
        cm = abi.GeneClusterMap(path, 'centroid_%s' % pid)
        m = {}
        for r in _python_parse(sp['gene_info'].encode())[1]:
            m[r['centroid_99']] = r['centroid_%s' % pid]
        clusters = sorted(set(m.values()))
        assert [cm.cluster(k).decode() for k in range(cm.n_clusters)] == clusters
        ids = bytes(cm.gene_ids)
        got = {ids[cm.gene_off[k]:cm.gene_off[k + 1]].decode(): clusters[cm.gene_cluster[k]] for k in range(cm.n_genes)}
        assert got == m and list(got) == list(m)


def test_table_reader_matches_python(tmp_path):
    import base64
    for sp in VEC['species']:
        paths = []
        for smp in sp['samples']:
            p = str(tmp_path / ('%s.genes.gz' % smp['id']))
            with gzip.open(p, 'wb') as h:
                h.write(base64.b64decode(smp['table']))
            paths.append(p)
        t = abi.GeneTables(paths, threads=3)
        for k, smp in enumerate(sp['samples']):
            fields, rows = _python_parse(base64.b64decode(smp['table']))
            gid = 'ref_id' if 'ref_id' in fields else 'gene_id'
            cp = 'normalized_coverage' if 'normalized_coverage' in fields else 'copy_number'
            dp = 'raw_coverage' if 'raw_coverage' in fields else 'coverage'
            ids = bytes(t.ids[k])
            assert [ids[t.id_off[k][i]:t.id_off[k][i + 1]].decode() for i in range(t.rows[k])] == [r[gid] for r in rows]
            exp_c = np.array([float(r[cp]) for r in rows])
            exp_d = np.array([float(r[dp]) for r in rows])
            exp_r = np.array([int(r['count_reads']) if 'count_reads' in r else 0 for r in rows], np.int64)
            assert np.array_equal(t.copy[k].view(np.uint64), exp_c.view(np.uint64))
            assert np.array_equal(t.depth[k].view(np.uint64), exp_d.view(np.uint64))
            assert np.array_equal(t.reads[k], exp_r)


def _write_table(path, text):
    with gzip.open(path, 'wb') as h:
        h.write(text.encode())


def test_key_sequence_reuse_equals_hash_lookups(tmp_path):
    gi = tmp_path / 'gene_info.txt'
    gi.write_text('centroid_99\tcentroid_95\n' + ''.join('g%d\tc%d\n' % (k, k % 7) for k in range(50)))
    a = 'gene_id\tcount_reads\tcoverage\tcopy_number\n' + ''.join('g%d\t1\t0.5\t0.25\n' % k for k in range(50))
    b = 'gene_id\tcount_reads\tcoverage\tcopy_number\n' + ''.join('g%d\t2\t1.5\t1.25\n' % k for k in reversed(range(50)))
    paths = []
    for k, text in enumerate([a, a, b, a, b]):
        paths.append(str(tmp_path / ('s%d.genes.gz' % k)))
        _write_table(paths[-1], text)
    cm = abi.GeneClusterMap(str(gi), 'centroid_95')
    reuse, hashed = abi.GeneTables(paths), abi.GeneTables(paths)
    reuse.resolve(cm, reuse=True)
    hashed.resolve(cm, reuse=False)
    assert reuse.same_as == [-1, 0, -1, 0, 2]
    assert hashed.same_as == [-1] * 5
    for x, y in zip(reuse.cluster, hashed.cluster):
        assert np.array_equal(x, y)
    assert np.array_equal(hashed.cluster[0], np.array([int(cm.cluster(0) != b'c0') * 0 + [b'c%d' % (k % 7) for k in range(7)].index(
        b'c%d' % (k % 7)) for k in range(50)], np.uint32))


def _merge_cli(*argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py')] + list(argv), capture_output=True,
                          text=True, cwd=ROOT, env=env)


def test_cli_usage_and_arguments(tmp_path):
    r = _merge_cli()
    assert r.returncode == 0 and 'genes' in r.stdout
    r = _merge_cli('species', str(tmp_path))
    assert r.returncode != 0 and 'not part of this build' in r.stderr
    assert _merge_cli('genes', str(tmp_path)).returncode != 0
    r = _merge_cli('genes', '-h')
    assert r.returncode == 0 and '--cluster_pid' in r.stdout and '--min_copy' in r.stdout
    db, dirs = M.write_golden_dataset(str(tmp_path / 'in'), VEC)
    for flag in ('--min_copy', '--sample_depth', '--max_samples'):
        r = _merge_cli('genes', str(tmp_path / 'o'), '-i', ','.join(dirs), '-t', 'list', '-d', db, flag, '-1')
        assert r.returncode != 0 and flag in r.stderr and 'negative' in r.stderr
    r = _merge_cli('genes', str(tmp_path / 'o'), '-i', ','.join(dirs), '-t', 'list', '-d', db, '--cluster_pid', '97')
    assert r.returncode != 0


def _run(tmp_path, db, dirs, *extra, make_context=M.NumpyGenesContext, out='out'):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import merge_midas
    finally:
        sys.path.pop(0)
    from midas_amd.merge import genes
    argv = ['merge_midas.py', 'genes', str(tmp_path / out), '-i', ','.join(dirs), '-t', 'list', '-d', db] + list(extra)
    old = sys.argv
    sys.argv = argv
    try:
        args = merge_midas.genes_arguments()
    finally:
        sys.argv = old
    merge_midas.check_arguments(args)
    genes.run_pipeline(args, make_context=make_context)
    return str(tmp_path / out)


@pytest.mark.parametrize("pid", ['75', '80', '85', '90', '95', '99'])
def test_whole_command_matches_the_reference_text(tmp_path, pid):
    db, dirs = M.write_golden_dataset(str(tmp_path / 'in'), VEC)
    out = _run(tmp_path, db, dirs, '--cluster_pid', pid, '--threads', '3')
    M.check_outputs(out, VEC, pid)


def _error_of(tmp_path, db, dirs, *extra):
    with pytest.raises(SystemExit) as e:
        _run(tmp_path, db, dirs, *extra, make_context=lambda: pytest.fail("the device must not be reached"))
    return str(e.value.code)


def test_error_exits_name_file_and_line(tmp_path):
    sp = VEC['species'][0]
    db, dirs = M.write_golden_dataset(str(tmp_path / 'in'), VEC)
    ids = ['--species_id', sp['id']]
    mine = [d for d in dirs if os.path.basename(d).startswith(sp['id'])]
    table = os.path.join(mine[1], 'genes', 'output', sp['id'] + '.genes.gz')
    good = gzip.open(table, 'rb').read().decode()
    lines = good.split('\n')
    # a gene id the cluster map lacks (the reference's KeyError)
    _write_table(table, '\n'.join(lines[:3] + ['nosuchgene\t1\t1.0\t1.0'] + lines[3:]))
    msg = _error_of(tmp_path, db, mine, *ids)
    assert msg.startswith('\nError: ') and 'nosuchgene' in msg and 'line 4' in msg and table in msg
    # a number this build does not read (Python would take 1_0: a documented limit)
    _write_table(table, '\n'.join(lines[:2] + ['%s\t1\t1_0\t1.0' % lines[1].split('\t')[0]] + lines[2:]))
    msg = _error_of(tmp_path, db, mine, *ids)
    assert 'line 3' in msg and table in msg
    _write_table(table, '\n'.join(lines[:2] + ['%s\t1.0\t1.0\t1.0' % lines[1].split('\t')[0]] + lines[2:]))
    assert 'count_reads' in _error_of(tmp_path, db, mine, *ids)
    # a missing required column
    _write_table(table, 'gene_id\tcount_reads\tcopy_number\n' + lines[1].split('\t')[0] + '\t1\t1.0\n')
    msg = _error_of(tmp_path, db, mine, *ids)
    assert "'coverage'" in msg and table in msg
    # a missing sample table
    os.remove(table)
    msg = _error_of(tmp_path, db, mine, *ids)
    assert 'missing genes table' in msg and table in msg
    _write_table(table, good)
    # a missing gene_info.txt
    for ext in ('', '.gz'):
        p = os.path.join(db, 'pan_genomes', sp['id'], 'gene_info.txt' + ext)
        if os.path.exists(p):
            os.remove(p)
    assert 'gene_info' in _error_of(tmp_path, db, mine, *ids)


def test_numbers_python_takes(tmp_path):
    """float()'s spellings this build reads, each the same double as Python's; int() likewise."""
    spell = ['1', '-0', '+1.5', ' 2.5 ', '\x0b3e2\x0c', '1E5', '.5', '5.', 'nan', '-NaN', 'inf', '-Infinity', '1e400', '-1e-400',
             '4.9e-324', '1e-5', '0x10']
    gi = tmp_path / 'gene_info.txt'
    gi.write_text('centroid_99\tcentroid_95\n' + ''.join('g%d\tc%d\n' % (k, k) for k in range(len(spell))))
    for k, s in enumerate(spell):
        p = str(tmp_path / ('t%d.genes.gz' % k))
        _write_table(p, 'gene_id\tcount_reads\tcoverage\tcopy_number\ng%d\t +7\t%s\t1\n' % (k, s))
        try:
            exp = float(s)
        except ValueError:
            exp = None
        if exp is None or s == '0x10':
            with pytest.raises(abi.MidasSnpsError):
                abi.GeneTables([p])
            continue
        t = abi.GeneTables([p])
        assert struct.pack('<d', t.depth[0][0]) == struct.pack('<d', exp) or (np.isnan(exp) and np.isnan(t.depth[0][0])), s
        assert t.reads[0][0] == 7
