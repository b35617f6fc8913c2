"""The host arithmetic of the device table readers (midas_amd/csrc/tables_plan.h), checked without a device by
tests/cpp/tables_plan_check.cpp against a row-by-row model: random member tables (empty members, a header-only first member), row
ranges (empty, inside one member, beyond the end) and caps; the members chosen are exactly those that hold rows of the range, their
skip and take counts add up to the range, the header member is the first one that holds text, and the groups are contiguous,
disjoint, cover the chosen members and respect the cap except for single oversized members."""
import os
import subprocess


def test_tables_plan_against_its_model(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "tables_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "tables_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
