"""The sizes of a walk over text matrices by row groups (midas_amd/csrc/row_group_plan.h), checked without a device by
tests/cpp/row_group_plan_check.cpp against the three formulas the function replaced, written out as they stood -- RowGroups::init
over two matrices, midas_genes_compare and midas_genes_linkage over one: random requests and sizes, and the borders crossed with
each other (zero and non-zero requests, a quarter of the free memory below 1 MiB, a text shorter than 64 bytes, a row bound of 1,
a chunk at 2^30)."""
import os
import subprocess


def test_row_group_plan_against_the_formulas_it_replaced(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "row_group_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "row_group_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
