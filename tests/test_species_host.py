"""run_species.py without a GPU: the sequential model (tests/species_model.py) against the vectors recorded from the reference's own
functions (tests/golden/species_vectors.json), the native serial chain (abi.species_assign) against the model's, the number
decoder against float() / int(), the read streamer against the reference's streamer, the script's argument checks, and
select_species with --species_cov / --species_topn / exclude.txt."""
import io
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, build
from midas_amd.run import snps as msnps
from midas_amd.run import species as mspecies
from tests import species_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = [c['name'] for c in VEC['cases']]


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    return M.write_db(str(tmp_path_factory.mktemp("species_db")), VEC['db'], genomes=['Species_%02d' % k for k in range(12)])


@pytest.fixture(scope="module")
def mdb(db):
    return M.Database.read(db)


def _case(name):
    return next(c for c in VEC['cases'] if c['name'] == name)


@pytest.mark.parametrize("name", CASES)
def test_model_equals_the_reference(mdb, name):
    c = _case(name)
    got = M.classify(c['m8'], mdb, seed=c['seed'], mapid=c['mapid'], aln_cov=c['aln_cov'])
    assert got['profile'] == c['profile']
    assert got['printed'] == c['printed']


def test_vectors_pin_the_chain(mdb):
    """Some case's profile is another when the weights of the draws are frozen after the unique pass."""
    differs = [c['name'] for c in VEC['cases']
               if M.classify(c['m8'], mdb, seed=c['seed'], mapid=c['mapid'], aln_cov=c['aln_cov'], frozen=True)['profile'] != c['profile']]
    assert differs


def _chain_by_model(indptr, sp, aln, reads, bases, py_state, np_state):
    py, nprng = M.generators(py_state=py_state, np_state=np_state)
    reads, bases = list(reads), list(bases)
    for q in range(len(indptr) - 1):
        ids = sp[indptr[q]:indptr[q + 1]]
        pick = M.draw([reads[i] for i in ids], py, nprng)
        reads[ids[pick]] += 1
        bases[ids[pick]] += aln[indptr[q] + ids.index(ids[pick])]
    return reads, bases


@pytest.mark.parametrize("name", CASES)
def test_native_chain_on_the_golden_cases(mdb, name):
    c = _case(name)
    rows = M.parse_lines(c['m8'], mdb, c['mapid'], c['aln_cov'])
    indptr, sp, aln, reads, bases = M.csr(M.best_hits(rows), mdb.species)
    py_state, np_state = random.Random(c['seed']).getstate(), np.random.RandomState(c['seed']).get_state()
    r, b, _ = abi.species_assign(indptr, sp, aln, reads, bases, py_state=py_state, np_state=np_state)
    want = M.classify(c['m8'], mdb, seed=c['seed'], mapid=c['mapid'], aln_cov=c['aln_cov'])
    assert r.tolist() == [want['reads'][s] for s in mdb.species] and b.tolist() == [want['bases'][s] for s in mdb.species]
    text, _ = M.profile_text(mdb, dict(zip(mdb.species, r.tolist())), dict(zip(mdb.species, b.tolist())))
    assert text == c['profile']


def test_native_chain_on_random_lists():
    rng = np.random.default_rng(5)
    drew_py = drew_np = 0
    for trial in range(200):
        S = int(rng.integers(2, 30))
        nq = int(rng.integers(0, 60))
        sizes = rng.integers(2, 9, size=nq)
        indptr = [0] + np.cumsum(sizes).tolist()
        sp = rng.integers(0, S, size=indptr[-1]).tolist()
        aln = rng.integers(-5, 300, size=indptr[-1]).tolist()
        reads = (rng.integers(0, 4, size=S) * (rng.random(S) < 0.4)).tolist()
        bases = rng.integers(0, 1000, size=S).tolist()
        seed = int(rng.integers(0, 2 ** 31))
        py_r, np_r = random.Random(seed), np.random.RandomState(seed)
        for _ in range(int(rng.integers(0, 700))):       # any position in the state, the regeneration at 624 included
            py_r.getrandbits(32)
            np_r.random_sample()
        py_state, np_state = py_r.getstate(), np_r.get_state()
        r, b, draws = abi.species_assign(indptr, sp, aln, reads, bases, py_state=py_state, np_state=np_state)
        wr, wb = _chain_by_model(indptr, sp, aln, reads, bases, py_state, np_state)
        assert r.tolist() == wr and b.tolist() == wb, trial
        drew_py += draws[0]
        drew_np += draws[1]
    assert drew_py > 100 and drew_np > 1000


def test_model_generators_are_the_interpreters():
    """The model's MT19937, index draw and double against random and numpy themselves."""
    for seed in (0, 1, 12345):
        py, nprng = M.generators(seed)
        r, n = random.Random(seed), np.random.RandomState(seed)
        for k in (1, 2, 3, 5, 8, 21, 22, 1000) * 90:
            assert py.below(k) == r.sample(list(range(k)), 1)[0]
        for _ in range(700):
            assert nprng.double() == n.random_sample()
    rng = np.random.default_rng(1)
    for _ in range(300):
        counts = rng.integers(0, 6, size=int(rng.integers(2, 9))).tolist()
        if sum(counts) == 0:
            continue
        seed = int(rng.integers(0, 10 ** 6))
        py, nprng = M.generators(seed)
        n = np.random.RandomState(seed)
        ids = list(range(len(counts)))
        assert ids[M.draw(counts, py, nprng)] == n.choice(ids, 1, p=[float(c) / sum(counts) for c in counts])[0]


SPELLINGS = ['0', '-0', '0.0', '-0.0', '1', '+1', '100', '100.0', '1e+02', '1E2', '1e-3', '98.7', '98.75', '99.999999999999', '123456789012345',
             '1234567890123456', '0.1234567890123456789', '98.76543210987654321', '1e22', '1e23', '1e-22', '1e-23', '123456789012345e22',
             '123456789012345e-22', '9007199254740993', '.5', '5.', '-.5e1', '1_0.5', 'inf', '-inf', 'nan', 'Infinity', '1e400', '1e-400',
             '2.2250738585072014e-308', '4.9e-324', '179.76931348623157e306', '0.000001', '000012.5000', '1e0001', '1.7976931348623157e308',
             '0.30000000000000004', '144.5', '59.8', '1e1000', '1e-1000']
NOT_NUMBERS = ['', '+', '-', '.', 'e5', '1e', '1e+', '1..2', '1.2.3', '1,5', 'abc', '1x', '0x10', '--1', '1__0', '_1', '1_', 'nan(1)']


def test_parse_number_equals_float_and_int():
    fast = 0
    for s in SPELLINGS:
        got = abi.species_parse_number(s.encode())
        assert got is not None, s
        assert np.float64(got[0]).tobytes() == np.float64(float(s)).tobytes() or (got[0] != got[0] and float(s) != float(s)), s
        fast += got[1]
    assert 15 < fast < len(SPELLINGS) - 10
    assert abi.species_parse_number(b'98.76543210987654321')[1] is False and abi.species_parse_number(b'99.5')[1] is True
    for s in NOT_NUMBERS:
        assert abi.species_parse_number(s.encode()) is None, s
        with pytest.raises(ValueError):
            float(s)
    rng = np.random.default_rng(3)
    for _ in range(3000):
        x = float(rng.random() * 10 ** int(rng.integers(-5, 6)))
        for s in (repr(x), '%.2f' % x, '%.6e' % x, '%.14g' % x, '%.15g' % x):
            got = abi.species_parse_number(s.encode())
            assert got is not None and got[0] == float(s), s
    for s, want in (('0', 0), ('150', 150), ('-7', -7), ('+12', 12), ('007', 7), ('999999999', 999999999), ('1234567890', 1234567890), ('1_000', 1000)):
        assert abi.species_parse_number(s.encode(), 'int')[0] == want == int(s)
    for s in ('', '1.0', '1e2', 'x', '-', '1 2'):
        assert abi.species_parse_number(s.encode(), 'int') is None


@pytest.mark.parametrize("k", range(len(VEC['stream']['cases'])))
def test_streamer_equals_the_reference(tmp_path, k):
    c = VEC['stream']['cases'][k]
    for name, text in VEC['stream']['files'].items():
        (tmp_path / name).write_text(text)
    argv = [str(tmp_path / a) if a in VEC['stream']['files'] else a for a in c['argv']]
    opts = dict(zip(argv[0::2], argv[1::2]))
    out = io.StringIO()
    counts = mspecies.stream_reads([p for p in (opts.get('-1'), opts.get('-2')) if p], out, int(opts['-l']) if '-l' in opts else None,
                                   int(opts['-n']) if '-n' in opts else None)
    assert out.getvalue() == c['stdout']
    assert '%s\t%s' % counts == c['stderr']


def test_streamer_reads_compressed_files(tmp_path):
    import bz2
    import gzip
    text = VEC['stream']['files']['reads.fq']
    with gzip.open(str(tmp_path / 'r.fq.gz'), 'wt') as h:
        h.write(text)
    with bz2.open(str(tmp_path / 'r.fq.bz2'), 'wt') as h:
        h.write(text)
    want = next(c for c in VEC['stream']['cases'] if c['argv'] == ['-1', 'reads.fq'])
    for name in ('r.fq.gz', 'r.fq.bz2'):
        out = io.StringIO()
        mspecies.stream_reads([str(tmp_path / name)], out)
        assert out.getvalue() == want['stdout']


def _cli(*argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'run_species.py')] + list(argv), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, env=env)


def test_script_argument_checks(tmp_path, db):
    out = str(tmp_path / 'sample')
    fq = tmp_path / 'reads.fq'
    fq.write_text(VEC['stream']['files']['reads.fq'])
    r = _cli(out, '-d', db)
    assert r.returncode == 2 and 'required: -1' in r.stderr
    r = _cli(out, '-d', db, '-1', str(tmp_path / 'nope.fq'))
    assert r.returncode == 1 and "Input file does not exist: '%s'" % (tmp_path / 'nope.fq') in r.stderr
    r = _cli(out, '-d', db, '-1', str(fq), '--word_size', '11')
    assert r.returncode == 1 and "Invalid word size: 11. Must be greater than or equal to 12" in r.stderr
    r = _cli(out, '-d', db, '-1', str(fq), '--mapid', '101')
    assert r.returncode == 1 and "Invalid mapping identity: 101.0. Must be between 0 and 100" in r.stderr
    r = _cli(out, '-d', db, '-1', str(fq), '--aln_cov', '1.5')
    assert r.returncode == 1 and "Invalid alignment coverage: 1.5. Must be between 0 and 1" in r.stderr
    r = _cli(out, '-d', str(tmp_path / 'no_db'), '-1', str(fq))
    assert r.returncode == 1 and "Specified reference database does not exist" in r.stderr
    env = dict(os.environ, PATH=str(tmp_path))              # no aligner on PATH
    r = _cli(out, '-d', db, '-1', str(fq), env=env)
    assert r.returncode == 1 and "hs-blastn not found on PATH" in r.stderr and "the aligner is not part of this build" in r.stderr
    r = _cli(out, '-d', db, '--classify')
    assert r.returncode == 1 and "no alignments were found" in r.stderr
    bad = tmp_path / 'reads.fq.gz'
    bad.write_text(VEC['stream']['files']['reads.fq'])
    r = _cli(out, '-d', db, '-1', str(bad))
    assert r.returncode == 1 and ("does not match expected compression" in r.stderr or "could not be recognized" in r.stderr or r.stderr)
    assert _cli('-h').returncode == 0


def test_run_midas_still_refuses_the_word_and_points_here():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'run_midas.py'), 'species', 'x'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and 'not part of this build' in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'run_midas.py'), '-h'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and 'run_species.py' in r.stdout


PROFILE = ('species_id\tcount_reads\tcoverage\trelative_abundance\n'
           'Species_04\t90\t9.5\t0.30\nSpecies_01\t80\t3.0\t0.35\nSpecies_07\t40\t2.9\t0.20\nSpecies_02\t10\t4.0\t0.10\nSpecies_09\t0\t0.0\t0\n')


def _select(tmp_path, db, **kw):
    out = tmp_path / 'sample'
    (out / 'species').mkdir(parents=True, exist_ok=True)
    (out / 'species' / 'species_profile.txt').write_text(PROFILE)
    args = dict(outdir=str(out), db=db, species_id=None, species_cov=None, species_topn=None)
    args.update(kw)
    return msnps.select_species(args)


def test_select_species_from_the_profile(tmp_path, db):
    assert _select(tmp_path, db, species_cov=3.0) == ['Species_04', 'Species_01', 'Species_02']
    assert _select(tmp_path, db, species_topn=2) == ['Species_04', 'Species_01']
    assert _select(tmp_path, db, species_topn=3, species_cov=3.0) == ['Species_04', 'Species_01']
    assert _select(tmp_path, db, species_cov=2.0, species_id=['Species_07', 'Species_02', 'Species_11']) == ['Species_07', 'Species_02']
    assert _select(tmp_path, db, species_id=['Species_03', 'Species_01']) == ['Species_03', 'Species_01']
    with pytest.raises(SystemExit) as e:
        _select(tmp_path, db, species_cov=50.0)
    assert 'no species sastisfied your selection criteria' in str(e.value)
    with pytest.raises(SystemExit) as e:
        _select(tmp_path, db, species_id=['Species_99'])
    assert 'Species id not found in database: Species_99' in str(e.value)


def test_select_species_excludes(tmp_path):
    db2 = M.write_db(str(tmp_path / 'db2'), VEC['db'], genomes=['Species_%02d' % k for k in range(12)])
    with open(os.path.join(db2, 'exclude.txt'), 'w') as handle:
        handle.write('Species_04\nSpecies_55\n')
    assert _select(tmp_path, db2, species_topn=2) == ['Species_01']
    with open(os.path.join(db2, 'exclude.txt'), 'w') as handle:
        handle.write('Species_04\nSpecies_01\n')
    with pytest.raises(SystemExit) as e:
        _select(tmp_path, db2, species_topn=2)
    assert 'no species sastisfied your selection criteria' in str(e.value)


def test_select_species_without_a_profile(tmp_path, db):
    with pytest.raises(SystemExit) as e:
        msnps.select_species(dict(outdir=str(tmp_path / 'none'), db=db, species_id=None, species_cov=3.0, species_topn=None))
    assert 'Could not locate species profile' in str(e.value)


def test_marker_database_arrays(db, mdb):
    m = mspecies.MarkerDatabase(db)
    assert m.species == mdb.species and len(m.gene_names) == 48 and b'9999.1.peg.1' not in m.gene_names
    assert m.cutoff.tolist() == [94.5, 95.5, 96.5, 98.0]
    assert mspecies.MarkerDatabase(db, 97.0).cutoff.tolist() == [97.0] * 4
    length = dict((s, 0) for s in mdb.species)
    for g in mdb.genes.values():
        length[g[0]] += g[2]
    assert m.marker_length == [length[s] for s in mdb.species]


def test_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'midas_snps.h')).read()
    lib = abi.load_library()
    for sym in abi.SPECIES_SYMBOLS:
        assert sym + '(' in header and getattr(lib, sym).argtypes is not None
    assert 'species_hits.hip' in build.SOURCES and 'species_assign.cpp' in build.SOURCES
    assert build.SOURCE_FLAGS['species_hits.hip'] == ['-ffp-contract=off']
    assert abi.ABI_VERSION == 4
    blob = open(build.LIB_PATH, 'rb').read()
    assert b'sp_fields_kernel' in blob and b'sp_rep_kernel' in blob
