"""The packed path's work plan (midas_amd/csrc/work_plan.h), checked without a device by tests/cpp/work_plan_check.cpp: no tiles, one
tile, equal tiles, one hot tile among five, two adjacent hot tiles and a tile whose part count would pass 4096.  Every tile appears
once as a whole item or as parts 0..np-1 of one np, whole items come first and n_whole counts them, a tile is split exactly when
its reads exceed max(2048, 2 * fair), np <= 4096, the zero ranges are disjoint, ascending, merged where adjacent and cover exactly
the split tiles' sites, and the same input gives the same plan."""
import os
import subprocess


def test_work_plan_properties(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "work_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "work_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
