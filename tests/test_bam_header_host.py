"""The pure pieces of the host's BAM reader (midas_amd/csrc/bam_parse.h), checked without the library by tests/cpp/bam_header_check.cpp:
the header parser answers "more bytes needed" for every proper prefix of a header of 0, 1 and 3 references (each prefix in a heap
buffer of exactly its size) and gives names, lengths and rec_begin for all of it, with and without bytes behind it; a wrong magic, a
reference with l_name == 0 and an l_text that points past the buffer are told apart; and the two searches over a block table (the
block holding an uncompressed offset, the first block at or behind a file offset) agree with a linear scan for every offset of
tables of 0, 1, 2 and 17 blocks, empty blocks among them."""
import os
import subprocess


def test_bam_header_and_block_searches_against_a_scan(tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "bam_header_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(here, "..", "midas_amd", "csrc"), "-o", exe, os.path.join(here, "cpp", "bam_header_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
