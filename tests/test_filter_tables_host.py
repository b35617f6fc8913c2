"""keep_read's integer tables (midas_amd/csrc/filter_tables.h), checked without a device by tests/cpp/filter_tables_check.cpp: for
every length 1..kMaxLSeq and six threshold pairs -- the defaults, thresholds everything passes, thresholds only a perfect read
passes, ratios that do not round, an identity threshold below every table entry and thresholds nothing passes -- each entry passes
the reference's own fp64 expression and the value below it does not, with the two end cases; at six lengths the entries are
compared against a full linear scan as well."""
import os
import subprocess


def test_filter_tables_against_the_reference_expressions(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "filter_tables_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "filter_tables_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
