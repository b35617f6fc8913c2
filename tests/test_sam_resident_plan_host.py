"""The host arithmetic of the resident SAM decode (midas_amd/csrc/sam_resident_plan.h), checked without a device by
tests/cpp/sam_resident_plan_check.cpp: the direct layout's units total, recovered from the low 32 bits the device's scan keeps, and
the side buffer's entries and bytes equal a record-by-record model over random (l_seq, n_cigar, flag) tables; 2^32 - 1 units fit
the layout and 2^32 do not; low bits no total can have are refused.  And the binding: the header declares the entry point, the
library exports it, abi binds it among the SAM symbols and refuses resident records in file order before anything is touched."""
import ctypes as C
import os
import subprocess

import pytest

from midas_amd import abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sam_resident_plan_against_its_model(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "sam_resident_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "sam_resident_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr


def test_the_library_exports_the_resident_entry_point():
    assert "midas_sam_load_resident" in abi.SAM_SYMBOLS and "midas_sam_load_resident" not in abi.EXPORTED_SYMBOLS
    lib = C.CDLL(build.build_native())
    header = open(os.path.join(ROOT, "include", "midas_snps.h")).read()
    assert hasattr(lib, "midas_sam_load_resident")
    assert "int32_t midas_sam_load_resident(const char* path, midas_snps_ctx* ctx, midas_bam** out, int64_t* n_reads, int64_t* sum_l_seq, char* err256);" in header
    blob = open(build.LIB_PATH, "rb").read()
    assert b"sam_direct_kernel" in blob and b"sam_resident_sizes_kernel" in blob
    # a null context is refused before anything is touched
    bound = abi.load_library()
    h, n = C.c_void_p(), C.c_int64()
    assert bound.midas_sam_load_resident(b"x.sam", None, C.byref(h), C.byref(n), C.byref(n), None) == abi.ERR_INVALID_ARG


def test_read_sam_refuses_resident_records_without_a_device_or_in_file_order():
    class Dev:
        inflates = True
        _h = None
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.read_sam("x.sam", None, resident=True)
    assert ei.value.status == abi.ERR_INVALID_ARG
    with pytest.raises(abi.MidasSnpsError) as ei:
        abi.read_sam("x.sam", Dev(), order='file', resident=True)
    assert ei.value.status == abi.ERR_INVALID_ARG and "resident" in ei.value.message


def test_the_stage_reads_its_switch_at_the_call(monkeypatch):
    from midas_amd.run import snps
    monkeypatch.delenv("MIDAS_SNPS_SAM_RESIDENT", raising=False)
    assert snps._sam_resident() is snps.SAM_RESIDENT_DEFAULT
    monkeypatch.setenv("MIDAS_SNPS_SAM_RESIDENT", "1")
    assert snps._sam_resident() is True
    monkeypatch.setenv("MIDAS_SNPS_SAM_RESIDENT", "0")
    assert snps._sam_resident() is False
