"""merge_species.py without a GPU: the sequential model (tests/merge_species_model.py) against every golden case recorded from
the reference's own functions, byte for byte; the script's argument checks, warnings and messages, all of which end before a
device is opened; merge_midas.py pointing to the script; the entry points declared, bound and built."""
import os
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, build
from tests import merge_species_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = M.load_vectors()
CASES = [c['name'] for c in VEC['cases']]


def _cli(*argv, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_species.py')] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, env=env)


@pytest.mark.parametrize("name", CASES)
def test_model_equals_the_reference(name):
    case = VEC['cases'][CASES.index(name)]
    files, err = M.run_case(VEC, case)
    for f in M.FILES:
        assert files[f] == case['outputs'][f], f
    assert err == case['stderr']


def test_vectors_tell_numpy_round_from_python_round():
    ids = M.species_ids(VEC['species_info'])
    case = VEC['cases'][CASES.index('hand_odd')]
    got = M.merge(case['indirs'], [case['profiles'][d] for d in case['indirs']], ids, 1.0)
    v = got['median_coverage'][0]
    assert v == 2.675 and str(round(v, 2)) == '2.68' and str(round(float(v), 2)) == '2.67'
    assert 'Bacteroides_vulgatus_57955\t2.67\t2.68\t' in case['outputs']['species_prevalence.txt']
    assert '\t123456.78\t123456.78\t' in case['outputs']['species_prevalence.txt']
    assert str(np.rint(np.float64(2.675) * 100) / 100) == '2.68'


def test_model_names_the_earliest_refusal():
    ids = ['a', 'b', 'c']
    head = 'species_id\tcount_reads\tcoverage\trelative_abundance\n'
    good = head + 'a\t1\t1.0\t0.5\nb\t2\t2.0\t0.25\nc\t3\t3.0\t0.25\n'
    assert M.first_error([good, good], ids) is None
    cases = [
        (good.replace('b\t2', 'q\t2'), M.UNKNOWN, 3), (good.replace('c\t3\t3.0\t0.25\n', ''), M.MISSING, 4), (good + 'a\t1\t1.0\t0.5\n', M.TWICE, 5),
        (good.replace('coverage', 'depth'), M.HEADER + 2, 1), (good.replace('2.0', 'two'), M.CELL + 1, 3), (good.replace('\t3\t', '\t3.5\t'), M.CELL, 4),
        (good.replace('0.5', 'nan'), M.NON_FINITE + 1, 2), (good.replace('3.0', '1e999'), M.NON_FINITE, 4), (good.replace('\t2\t', '\t9223372036854775808\t'), M.RANGE, 3),
    ]
    for text, reason, line in cases:
        e = M.first_error([good, text, text.replace('a\t1', 'z\t1')], ids)
        assert (e.reason, e.sample, e.line) == (reason, 1, line), (text, e)
    assert M.read_profile(good.replace('b\t2\t2.0\t0.25\n', 'b\t2\t2.0\n\nb\t2\t2.0\t0.25\n'), ids)['b'] == (2, 2.0, 0.25)       # short lines are dropped


def _tree(tmp_path, name='hand_odd'):
    case = VEC['cases'][CASES.index(name)]
    db, indirs = M.write_case(str(tmp_path / 'in'), VEC, case)
    return case, db, indirs


def test_argument_checks_end_before_the_device(tmp_path):
    case, db, indirs = _tree(tmp_path)
    out = str(tmp_path / 'out')
    r = _cli()
    assert r.returncode == 2 and 'the following arguments are required' in r.stderr
    r = _cli(out, '-i', ','.join(indirs), '-t', 'list', env=dict((k, v) for k, v in os.environ.items() if k != 'MIDAS_DB'))
    assert r.returncode == 1 and "No reference database specified" in r.stderr
    r = _cli(out, '-i', ','.join(indirs), '-t', 'list', env=dict(os.environ, MIDAS_DB=str(tmp_path / 'nowhere')))
    assert r.returncode == 1 and "Specified reference database does not exist" in r.stderr
    assert os.path.isdir(out)                               # (created before the checks, as in the reference)
    for flag in ('--sample_depth', '--max_samples'):
        r = _cli(out, '-i', ','.join(indirs), '-t', 'list', '-d', db, flag, '-1')
        assert r.returncode == 1 and "\nError: %s cannot be a negative value\n" % flag in r.stderr
    r = _cli(out, '-i', str(tmp_path / 'none'), '-t', 'dir', '-d', db)
    assert r.returncode == 1 and "Specified input directory '%s' does not exist" % (tmp_path / 'none') in r.stderr
    r = _cli(out, '-i', str(tmp_path / 'none.txt'), '-t', 'file', '-d', db)
    assert r.returncode == 1 and "Specified input file '%s' does not exist" % (tmp_path / 'none.txt') in r.stderr
    r = _cli(out, '-i', indirs[0] + ',' + str(tmp_path / 'none'), '-t', 'list', '-d', db)
    assert r.returncode == 1 and "Specified input directory '%s' does not exist" % (tmp_path / 'none') in r.stderr
    r = _cli(out, '-i', ','.join(indirs), '-t', 'bogus', '-d', db)
    assert r.returncode == 2


def test_no_sample_left_warns_and_ends_before_the_device(tmp_path):
    case, db, indirs = _tree(tmp_path)
    bare = [str(tmp_path / 'bare_1'), str(tmp_path / 'bare_2')]
    for d in bare:
        os.makedirs(d)
    r = _cli(str(tmp_path / 'out'), '-i', ','.join(bare), '-t', 'list', '-d', db)
    assert r.returncode == 1
    assert r.stderr == ''.join("Warning: missing/incomplete output: %s\n" % d for d in bare) + "\nError: no samples with species profiles\n\n"
    assert "===========Parameters===========" in r.stdout and "Script: merge_species.py" in r.stdout
    assert "Minimum coverage for estimating prevalence: 1.0" in r.stdout and "Keep <=" not in r.stdout
    os.remove(os.path.join(db, 'species_info.txt'))
    r = _cli(str(tmp_path / 'out'), '-i', ','.join(indirs), '-t', 'list', '-d', db, '--max_samples', '2')
    assert r.returncode == 1 and "Could not locate species info" in r.stderr and "Keep <= 2 samples" in r.stdout


def test_sample_rules_are_the_reference_s(tmp_path):
    from midas_amd.merge import species
    case, db, indirs = _tree(tmp_path, 'warnings')
    import contextlib
    import io
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        samples = species.identify_samples(dict(indirs=indirs, max_samples=case['max_samples']))
    assert err.getvalue().replace(str(tmp_path / 'in') + os.sep, '') == case['stderr']
    assert [s.id for s in samples] == case['outputs']['coverage.txt'].split('\n')[0].split('\t')[1:]
    assert species.read_species_ids(db) == M.species_ids(VEC['species_info'])
    with open(os.path.join(db, 'species_info.txt'), 'a') as handle:
        handle.write('short line\nSp_2\tG1\t1\nNew\tG2\t2\n')      # a dropped line, an id again, a new one
    assert species.read_species_ids(db) == M.species_ids(VEC['species_info']) + ['New']


def test_help_texts():
    r = _cli('-h')
    assert r.returncode == 0
    for word in ('--sample_depth', '--max_samples', '--profile', 'species_prevalence.txt', 'list|file|dir'):
        assert word in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), '-h'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and 'merge_species.py' in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'merge_midas.py'), 'species', 'x'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and 'not part of this build' in r.stderr


def test_symbols_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, 'include', 'midas_snps.h')).read()
    lib = abi.load_library()
    for sym in abi.SPECIES_MERGE_SYMBOLS:
        assert sym + '(' in header and getattr(lib, sym).argtypes is not None
    assert 'species_merge.hip' in build.SOURCES and build.SOURCE_FLAGS['species_merge.hip'] == ['-ffp-contract=off']
    assert abi.ABI_VERSION == 4
    blob = open(build.LIB_PATH, 'rb').read()
    for kernel in (b'sm_fields_kernel', b'sm_lookup_kernel', b'sm_scatter_kernel', b'sm_stats_kernel', b'sm_long_median_kernel'):
        assert kernel in blob
