"""`run_midas.py genes --device_inflate` without a GPU: the option, the choice of the route as a pure function, and the new entry
point in the header, the binding and the library built here."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

from midas_amd import abi, build
from midas_amd.run import genes as run_genes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_MIDAS = os.path.join(ROOT, "scripts", "run_midas.py")


def _parser():
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_midas_script", RUN_MIDAS)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.build_genes_parser()


def test_the_genes_parser_takes_the_three_values_and_refuses_a_fourth(capsys):
    p = _parser()
    base = ["genes", "OUT", "-1", "reads.fq"]
    assert vars(p.parse_args(base))['device_inflate'] == 'auto'
    for v in ('auto', 'on', 'off'):
        assert vars(p.parse_args(base + ["--device_inflate", v]))['device_inflate'] == v
    with pytest.raises(SystemExit) as ei:
        p.parse_args(base + ["--device_inflate", "maybe"])
    assert ei.value.code == 2 and "--device_inflate" in capsys.readouterr().err


def test_help_names_the_option_and_what_auto_does():
    r = subprocess.run([sys.executable, RUN_MIDAS, "genes", "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and "--device_inflate {auto,on,off}" in r.stdout and "pangenomes.bam" in r.stdout
    if run_genes.AUTO_DEVICE_BAM_BYTES is None:
        assert "'on' selects it" in r.stdout


def test_the_route_over_all_its_cases():
    for option, has, known, one in itertools.product(('auto', 'on', 'off'), (False, True), (False, True), (False, True)):
        able = has and known and one
        # (auto with the threshold the module carries, then with one given: below it and at it)
        got = run_genes.bam_route(option, has, known, one, bam_bytes=1 << 40)
        if option == 'off' or not able:
            assert got == 'host', (option, has, known, one)
        elif option == 'on':
            assert got == 'device'
        else:
            assert got == ('host' if run_genes.AUTO_DEVICE_BAM_BYTES is None else 'device')
        for size, want in ((99, 'host'), (100, 'device'), (101, 'device')):
            got = run_genes.bam_route(option, has, known, one, bam_bytes=size, auto_bytes=100)
            assert got == ('host' if option == 'off' or not able else 'device' if option == 'on' else want), (option, has, known, one, size)
        assert run_genes.bam_route(option, has, known, one, bam_bytes=1 << 40, auto_bytes=None) == ('device' if option == 'on' and able else 'host')


def test_a_context_double_without_the_entry_takes_the_host_route():
    class Double:
        def genes_count(self, *a):
            raise AssertionError
    assert not hasattr(Double(), 'genes_count_bam')
    assert run_genes.bam_route('on', hasattr(Double(), 'genes_count_bam'), True, True) == 'host'
    assert hasattr(abi.Context, 'genes_count_bam') and hasattr(abi.Context, 'genes_count_bam_timing')


def test_the_header_declares_the_entry_and_abi_binds_it():
    header = open(os.path.join(ROOT, "include", "midas_snps.h")).read()
    assert "int32_t midas_genes_count_bam(midas_snps_ctx* ctx, midas_bam* bam, const midas_snps_thresholds* thr, int64_t n_genes," in header
    assert "#define MIDAS_SNPS_ABI_VERSION 4 " in header and abi.ABI_VERSION == 4
    assert "midas_genes_count_bam" in abi.EXPORTED_SYMBOLS
    assert len(abi.GENES_BAM_PHASES) == 6 and abi.GENES_BAM_STATS[0] == 'records'


def test_the_library_built_here_exports_the_symbol():
    lib = C.CDLL(build.build_native())
    assert hasattr(lib, "midas_genes_count_bam")
    assert lib.midas_snps_abi_version() == 4
    assert b"bam_genes_facts_kernel" in open(build.LIB_PATH, "rb").read()
    bound = abi.load_library(build_if_missing=False)
    # null arguments are refused before anything is touched
    assert bound.midas_genes_count_bam(None, None, None, 0, None, None, None, None, None, None, None) == abi.ERR_INVALID_ARG


def test_open_bam_device_needs_a_device_context():
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.open_bam_device("x.bam", None)
    assert ei.value.status == abi.ERR_INVALID_ARG
