"""The host arithmetic of the device BAM decode (midas_amd/csrc/decode_plan.h), checked without a device by
tests/cpp/decode_plan_check.cpp: the arena's regions are ordered, disjoint and 256-byte aligned; every group of a streamed decode
fits the slot (the match lists of its last block included), the last group ends with the job range and every other one stops where
the next begins; and the stitching of the walk's chunks gives the model walker's records -- guesses right and wrong, exact and
guessed starts, chunks without a record boundary, bad chunks on and off the chain, and a walk that never settles."""
import os
import subprocess


def test_decode_plan_against_its_model(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "decode_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "decode_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
