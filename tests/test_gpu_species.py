"""run_species.py on the GPU box: midas_species_classify against the sequential model (tests/species_model.py) -- every decoded
pid and score as bit patterns, every integer, the unique counters and the CSR of the ambiguous reads -- on about 20 000 synthetic
lines in one chunk, in 4 KB chunks, shuffled, and with the query hash narrowed to 8 and 4 bits; the edge inputs and every error,
the earliest bad line at two chunk sizes; every golden case (tests/golden/species_vectors.json) in process and through the
script; and the chain run_species.py --classify -> run_midas.py snps --build_db --species_topn."""
import os
import stat
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi
from midas_amd.run import species as mspecies
from tests import species_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = [c['name'] for c in VEC['cases']]
SEED = 20261017


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def arrays(db, mapid=None):
    """A model Database as the arrays Context.species_classify takes."""
    sp = dict((s, k) for k, s in enumerate(db.species))
    markers = sorted(db.cutoffs)
    mk = dict((m, k) for k, m in enumerate(markers))
    names = list(db.genes)
    return dict(gene_names=[g.encode() for g in names], gene_species=[sp[db.genes[g][0]] for g in names],
                gene_marker=[mk[db.genes[g][1]] for g in names], n_species=len(db.species),
                marker_cutoff=[mapid if mapid else db.cutoffs[m] for m in markers], markers=markers)


def run(ctx, text, db, aln_cov=0.75, mapid=None, **kw):
    a = arrays(db, mapid)
    return ctx.species_classify(text.encode(), a['gene_names'], a['gene_species'], a['gene_marker'], a['n_species'], a['marker_cutoff'], aln_cov, **kw)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist()


def expect(text, db, aln_cov=0.75, mapid=None):
    """What the model says the device step returns."""
    rows = M.parse_lines(text, db, mapid, aln_cov)
    hits = M.best_hits(rows)
    indptr, sp, aln, reads, bases = M.csr(hits, db.species)
    index = dict((s, k) for k, s in enumerate(db.species))
    mk = dict((m, k) for k, m in enumerate(sorted(db.cutoffs)))
    return dict(rows=rows, hits=hits, indptr=indptr, hit_species=sp, hit_aln=aln, uniq_reads=reads, uniq_aln=bases,
                pid=bits([r['pid'] for r in rows]), score=bits([r['score'] + 0.0 for r in rows]), aln=[r['aln'] for r in rows],
                qlen=[r['qlen'] for r in rows], species=[index[r['species']] for r in rows], marker=[mk[r['marker']] for r in rows],
                passed=[int(r['passed']) for r in rows])


def same(got, want, lines=True):
    assert got['lines'] == len(want['rows']) and got['passing'] == sum(want['passed'])
    assert got['unique'] == sum(1 for h in want['hits'] if len(h) == 1) and got['ambiguous'] == len(want['indptr']) - 1
    assert got['uniq_reads'].tolist() == want['uniq_reads'] and got['uniq_aln'].tolist() == want['uniq_aln']
    assert got['indptr'].tolist() == want['indptr']
    assert got['hit_species'].tolist() == want['hit_species'] and got['hit_aln'].tolist() == want['hit_aln']
    if lines:
        for k in ('aln', 'qlen', 'species', 'marker', 'passed'):
            assert got[k].tolist() == want[k], k
        assert bits(got['pid']) == want['pid'] and bits(got['score']) == want['score']


@pytest.fixture(scope="module")
def big():
    db, text = M.synth_m8(5000, 40, 15, SEED)
    want = expect(text, db)
    assert 18000 < len(want['rows']) < 22000 and len(want['indptr']) > 500 and 0.3 < np.mean(want['passed']) < 0.9
    return db, text, want


def test_one_chunk(ctx, big):
    db, text, want = big
    got = run(ctx, text, db, dump=True)
    same(got, want)
    assert got['chunks'] == 1 and got['side_cells'] > 100              # some spellings went to the host's parser
    assert got['side_cells'] < got['lines'] // 4                       # ... and most numbers did not


def test_small_chunks(ctx, big):
    db, text, want = big
    got = run(ctx, text, db, dump=True, chunk_bytes=4000)              # (rounded to 4000: lines and queries straddle the chunks)
    same(got, want)
    assert got['chunks'] == (len(text) + got['chunk_bytes'] - 1) // got['chunk_bytes'] > 250
    same(run(ctx, text, db, dump=True, chunk_bytes=4099), want)        # not a multiple of 16 as given


def test_shuffled_lines(ctx):
    db, text = M.synth_m8(5000, 40, 15, SEED, shuffle=True)
    want = expect(text, db)
    where = {}
    for k, r in enumerate(want['rows']):
        where.setdefault(r['query'], []).append(k)
    assert sum(1 for v in where.values() if v[-1] - v[0] + 1 != len(v)) > 1000      # queries whose lines are apart
    same(run(ctx, text, db, dump=True), want)
    same(run(ctx, text, db, dump=True, chunk_bytes=4096, hash_bits=8), want)


@pytest.mark.parametrize("hash_bits", [64, 33, 8, 4])
def test_hash_width_changes_nothing(ctx, big, hash_bits):
    db, text, want = big
    same(run(ctx, text, db, hash_bits=hash_bits), want, lines=False)


def test_chain_after_the_device_step(ctx, big):
    db, text, want = big
    got = run(ctx, text, db)
    import random
    py_state, np_state = random.Random(5).getstate(), np.random.RandomState(5).get_state()
    r, b, draws = abi.species_assign(got['indptr'], got['hit_species'], got['hit_aln'], got['uniq_reads'], got['uniq_aln'], py_state, np_state)
    py, nprng = M.generators(5)
    reads, bases, _, _ = M.assign(want['hits'], db.species, py, nprng)
    assert r.tolist() == [reads[s] for s in db.species] and b.tolist() == [bases[s] for s in db.species]
    assert draws[1] > 500


def test_mapid_and_aln_cov(ctx, big):
    db, text, _ = big
    same(run(ctx, text, db, aln_cov=0.5, mapid=98.25, dump=True), expect(text, db, 0.5, 98.25))
    same(run(ctx, text, db, aln_cov=1.0, dump=True), expect(text, db, 1.0))


# ---- edge inputs ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    db, text = M.synth_m8(120, 6, 3, 7)
    return db, text


def test_empty_file(ctx, small):
    db, _ = small
    got = run(ctx, '', db, dump=True)
    assert got['lines'] == got['passing'] == got['unique'] == got['ambiguous'] == 0
    assert got['indptr'].tolist() == [0] and not got['uniq_reads'].any() and got['pid'].size == 0


def test_one_line_without_newline(ctx, small):
    db, text = small
    line = text.split('\n')[0]
    same(run(ctx, line, db, dump=True), expect(line + '\n', db))
    same(run(ctx, text[:-1], db, dump=True), expect(text, db))
    same(run(ctx, text[:-1], db, dump=True, chunk_bytes=64), expect(text, db))


def test_blanks_between_fields(ctx, small):
    db, text = small
    wide = '\n'.join('   \t '.join(l.split()) + '  \r' for l in text.splitlines()) + '\n'
    want = expect(wide, db)
    assert want['passed'] == expect(text, db)['passed']
    same(run(ctx, wide, db, dump=True), want)
    same(run(ctx, wide, db, dump=True, chunk_bytes=160), want)


def test_more_side_cells_than_the_first_list_holds(ctx, big):
    """Every pid and score spelled beyond 15 digits: the field kernel counts the cells, the list is made as long, the kernel runs again."""
    db, text, _ = big
    lines = []
    for l in text.splitlines()[:900]:
        f = l.split()
        f[2], f[11] = '%.17f' % float(f[2]), '0%s00000000000000001' % repr(float(f[11]))
        lines.append('\t'.join(f))
    long_text = '\n'.join(lines) + '\n'
    got = run(ctx, long_text, db, dump=True)
    assert got['side_cells'] == 1800 > 900 // 8 + 1024
    same(got, expect(long_text, db))


def _with_bad(text, bad):
    lines = text.splitlines()
    for number, line in bad.items():
        lines[number - 1] = line
    return '\n'.join(lines) + '\n'


def _edit(text, number, field, value):
    f = text.splitlines()[number - 1].split('\t')
    f[field] = value
    return '\t'.join(f)


ERRORS = [('fields', 1, lambda t, n: '\t'.join(t.splitlines()[n - 1].split('\t')[:11])),
          ('fields', 1, lambda t, n: ''),
          ('target', 2, lambda t, n: _edit(t, n, 1, 'no.such.peg.1')),
          ('target', 2, lambda t, n: _edit(t, n, 1, t.splitlines()[n - 1].split('\t')[1] + '0')),
          ('qlen', 3, lambda t, n: _edit(t, n, 0, 'read_x')),
          ('qlen', 3, lambda t, n: _edit(t, n, 0, 'read_0')),
          ('qlen', 3, lambda t, n: _edit(t, n, 0, 'read_')),
          ('aln', 4, lambda t, n: _edit(t, n, 3, '12.5')),
          ('aln', 4, lambda t, n: _edit(t, n, 3, '99999999999')),
          ('number', 5, lambda t, n: _edit(t, n, 2, '9x.5')),
          ('number', 5, lambda t, n: _edit(t, n, 11, '1e'))]


@pytest.mark.parametrize("k", range(len(ERRORS)))
@pytest.mark.parametrize("chunk_bytes", [0, 1024])
def test_errors_name_the_earliest_line(ctx, small, k, chunk_bytes):
    db, text = small
    name, reason, make = ERRORS[k]
    n_lines = len(text.splitlines())
    first, later = n_lines // 3, 2 * n_lines // 3
    other = ERRORS[(k + 3) % len(ERRORS)][2]
    bad = _with_bad(text, {first: make(text, first), later: other(text, later), n_lines: make(text, n_lines)})
    if name != 'aln' or '9999' not in make(text, first):
        with pytest.raises(M.BadLine) as m:
            M.parse_lines(bad, db)
        assert (m.value.line, m.value.reason) == (first, name)
    with pytest.raises(abi.MidasSnpsError) as e:
        run(ctx, bad, db, chunk_bytes=chunk_bytes)
    assert e.value.status == abi.ERR_BAD_LAYOUT and e.value.bad == (reason, first) and 'line %d:' % first in str(e.value)
    # the same two bad lines the other way round: the other reason, still the earliest line
    swapped = _with_bad(text, {first: other(text, first), later: make(text, later)})
    with pytest.raises(abi.MidasSnpsError) as e:
        run(ctx, swapped, db, chunk_bytes=chunk_bytes)
    assert e.value.bad == (ERRORS[(k + 3) % len(ERRORS)][1], first)


def test_unknown_cutoff_and_nan_score(ctx, small):
    db, text = small
    a = arrays(db)
    cut = list(a['marker_cutoff'])
    cut[1] = float('nan')
    with pytest.raises(abi.MidasSnpsError) as e:
        ctx.species_classify(text.encode(), a['gene_names'], a['gene_species'], a['gene_marker'], a['n_species'], cut, 0.75)
    first = 1 + next(k for k, r in enumerate(M.parse_lines(text, db)) if r['marker'] == a['markers'][1])
    assert e.value.bad == (6, first)
    with pytest.raises(abi.MidasSnpsError) as e:
        run(ctx, _with_bad(text, {9: _edit(text, 9, 11, 'nan')}), db)
    assert e.value.bad == (7, 9)


# ---- the golden cases ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gdb(tmp_path_factory):
    return M.write_db(str(tmp_path_factory.mktemp("species_db")), VEC['db'], genomes=['Species_%02d' % k for k in range(12)])


def _case(name):
    return next(c for c in VEC['cases'] if c['name'] == name)


@pytest.mark.parametrize("name", CASES)
def test_golden_in_process(ctx, gdb, name):
    import random
    c = _case(name)
    mdb = mspecies.MarkerDatabase(gdb, c['mapid'])
    text = np.frombuffer(c['m8'].encode(), np.uint8)
    for kw in (dict(), dict(chunk_bytes=256, hash_bits=3)):
        reads, bases, hits = mspecies.classify(ctx, text, mdb, c['aln_cov'], py_state=random.Random(c['seed']).getstate(),
                                               np_state=np.random.RandomState(c['seed']).get_state(), **kw)
        rows, total = mspecies.abundance(mdb, reads, bases)
        got = '\t'.join(['species_id', 'count_reads', 'coverage', 'relative_abundance']) + '\n' + ''.join('\t'.join(str(x) for x in r) + '\n' for r in rows)
        assert got == c['profile']
        assert ["  total alignments: %s" % hits['lines'], "  uniquely mapped reads: %s" % hits['unique'],
                "  ambiguously mapped reads: %s" % hits['ambiguous'], "  total marker-gene coverage: %s" % round(total, 3)] == c['printed']
    if name == 'hand':
        assert hits['side_cells'] >= 2              # the 20-digit pid and the 16-digit score


def _script(*argv, env=None):
    return subprocess.run([sys.executable] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)


@pytest.mark.parametrize("name", CASES)
def test_golden_through_the_script(tmp_path, gdb, name):
    c = _case(name)
    out = M.write_sample(str(tmp_path / 'sample'), c['m8'])
    argv = [os.path.join(ROOT, 'scripts', 'run_species.py'), out, '-d', gdb, '--classify', '--seed', str(c['seed']), '--aln_cov', str(c['aln_cov'])]
    if c['mapid']:
        argv += ['--mapid', str(c['mapid'])]
    r = _script(*argv)
    assert r.returncode == 0, r.stderr
    assert open(os.path.join(out, 'species', 'species_profile.txt')).read() == c['profile']
    printed = r.stdout.splitlines()
    for line in c['printed']:
        assert line in printed
    assert os.path.isfile(os.path.join(out, 'species', 'log.txt')) and os.path.isdir(os.path.join(out, 'species', 'temp'))


def test_script_reports_a_bad_line(tmp_path, gdb):
    c = _case('hand')
    lines = c['m8'].splitlines()
    lines[4] = '\t'.join(lines[4].split('\t')[:7])
    out = M.write_sample(str(tmp_path / 'sample'), '\n'.join(lines) + '\n')
    r = _script(os.path.join(ROOT, 'scripts', 'run_species.py'), out, '-d', gdb, '--classify')
    assert r.returncode == 1 and 'line 5: fewer than 12 fields' in r.stderr and 'alignments.m8' in r.stderr
    assert not os.path.exists(os.path.join(out, 'species', 'species_profile.txt'))


def test_profile_selects_the_species_of_the_snps_database(tmp_path, gdb):
    c = _case('mixed')
    out = M.write_sample(str(tmp_path / 'sample'), c['m8'])
    r = _script(os.path.join(ROOT, 'scripts', 'run_species.py'), out, '-d', gdb, '--classify', '--seed', str(c['seed']))
    assert r.returncode == 0, r.stderr
    stub = tmp_path / 'bin'
    stub.mkdir()
    tool = stub / 'bowtie2-build'
    tool.write_text('#!/bin/sh\nexit 0\n')
    tool.chmod(tool.stat().st_mode | stat.S_IXUSR)
    env = dict(os.environ, PATH=str(stub) + os.pathsep + os.environ.get('PATH', ''))
    r = _script(os.path.join(ROOT, 'scripts', 'run_midas.py'), 'snps', out, '-d', gdb, '--build_db', '--species_topn', '2', env=env)
    assert r.returncode == 0, r.stderr
    rows = [l.split('\t') for l in c['profile'].splitlines()[1:]]
    top = set(x[0] for x in sorted(rows, key=lambda x: float(x[3]), reverse=True)[:2])
    want = [x[0] for x in rows if x[0] in top]
    assert open(os.path.join(out, 'snps', 'species.txt')).read().split() == want and len(want) == 2
    fa = open(os.path.join(out, 'snps', 'temp', 'genomes.fa')).read()
    assert [l[1:] for l in fa.splitlines() if l.startswith('>')] == ['%s_contig' % s for s in want]
