"""The device writers of `merge_midas.py snps` from the host's side (no GPU): the two entry points are declared, exported and
bound; a context that offers merge_sites alone still drives merge_species through the host writers; and the '{0:.3g}' digit
routine the kernels share with the host (csrc/merge_fmt.h) equals snprintf("%.3g") on the formatter's value grid, in a stand-alone
program (tests/merge_fmt_check.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from midas_amd import abi, build, synth
from midas_amd.merge import snps as msnps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['midas_merge_write_matrix_device', 'midas_merge_sites_tables']


def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "midas_snps.h")).read(), flags=re.S)
    build.build_native()
    raw = C.CDLL(build.LIB_PATH)
    lib = abi.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in abi.EXPORTED_SYMBOLS and hasattr(raw, sym)
        assert getattr(lib, sym).argtypes[0] is C.c_void_p and getattr(lib, sym).restype is C.c_int32
    assert callable(abi.write_merge_matrix_device) and callable(abi.Context.merge_sites_tables)
    blob = open(build.LIB_PATH, "rb").read()
    assert b"rows_write_kernel" in blob and b"rows_length_kernel" in blob


def test_environment_switches_are_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "MIDAS_SNPS_MERGE_WRITERS" in doc and "MIDAS_SNPS_MERGE_TEXT_MB" in doc


def _command_args(monkeypatch, outdir, ds, *extra):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import merge_midas
    finally:
        sys.path.pop(0)
    monkeypatch.setattr(sys, 'argv', ['merge_midas.py', 'snps', outdir, '-i', os.path.dirname(ds['samples'][0]), '-t', 'dir',
                                      '-d', ds['db']] + list(extra))
    merge_midas.get_program()
    args = merge_midas.snps_arguments()
    merge_midas.check_arguments(args)
    return args


def test_a_context_with_merge_sites_alone_takes_the_host_writers(tmp_path, monkeypatch):
    from tests.test_gpu_merge import oracle_fields, oracle_text

    class OracleContext:
        """midas_merge_sites' contract by the restated reference; no merge_sites_tables."""
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def merge_sites(self, prm, counts, mean_depth):
            names = [t for t, bit in abi.SNP_TYPE_BITS.items() if prm.snp_types & bit]
            args = dict(allele_freq=prm.allele_freq, site_depth=prm.site_depth, site_ratio=prm.site_ratio, site_prev=prm.site_prev,
                        snp_type=names)
            out = oracle_fields([np.asarray(c) for c in counts], [float(x) for x in mean_depth], args)
            out['kernel_ms'] = 0.0
            return out

    ds = synth.make_merge_dataset(str(tmp_path / "ds"), n_samples=3, n_sites=400, seed=4)
    out = str(tmp_path / "merged")
    args = _command_args(monkeypatch, out, ds, '--all_sites')
    called = []
    real = abi.write_merge_matrix
    monkeypatch.setattr(abi, 'write_merge_matrix', lambda *a, **k: (called.append(1), real(*a, **k))[1])
    msnps.run_pipeline(args, make_context=OracleContext)
    assert len(called) == 2
    info, freq, depth = oracle_text(ds, dict(abi.DEFAULT_MERGE_ARGS, snp_type=['any'], site_prev=0.0))
    ids = "\t".join("sample_%d" % (k + 1) for k in range(3))
    d = os.path.join(out, 'sp1')
    assert open(os.path.join(d, 'snps_freq.txt')).read() == "site_id\t" + ids + "\n" + "".join(freq)
    assert open(os.path.join(d, 'snps_depth.txt')).read() == "site_id\t" + ids + "\n" + "".join(depth)
    assert len(open(os.path.join(d, 'snps_info.txt')).read().splitlines()) == 1 + len(info)


def _host_compiler():
    for cand in ('g++', 'c++', 'clang++'):
        if shutil.which(cand):
            return [shutil.which(cand)]
    return [build._hipcc(), '-x', 'c++']


def test_digit_routine_equals_snprintf_on_the_value_grid(tmp_path):
    """Every (m, d) with 0 <= m <= d <= 1200, the tie families, the exponent border and the extremes, 300 000 random pairs."""
    exe = str(tmp_path / "merge_fmt_check")
    cc = _host_compiler()
    r = subprocess.run(cc + ['-O2', '-std=c++17', os.path.join(ROOT, 'tests', 'merge_fmt_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"(\d+) compared, 0 differ", r.stdout)
    assert m and int(m.group(1)) > 1300000


def test_python_agrees_with_snprintf_where_the_tests_use_it():
    """The GPU tests build their expected text with Python's format; the stand-alone program compares with snprintf: the two agree
    on the named cases."""
    for (m, d), want in {(9985, 10000): '0.999', (1999, 2000): '1', (1, 32): '0.0312', (3, 32): '0.0938', (99949, 10 ** 9): '9.99e-05',
                         (99950, 10 ** 9): '0.0001', (1, 4294967294): '2.33e-10', (1, 10240): '9.77e-05'}.items():
        assert '{0:.3g}'.format(float(m) / d) == want
