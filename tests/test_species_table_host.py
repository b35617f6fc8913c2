"""The table of species ids (midas_amd/csrc/species_table.h: sm_hash and species_table_build, which species_merge.hip includes)
without a device: tests/cpp/species_table_check.cpp, built stand-alone with the address and undefined-behaviour sanitizers, reads
id lists and prints the table size and every id's hash and slot; the mirror of tests/merge_species_cases.py (sm_hash, table_of)
must say the same for every id list of the cases module, at the growth borders R = 1, 7, 8, 15, 16 (and 17, 31, 32), for the
empty id, for long ids and bytes above 0x7F, and both must refuse a list that names an id twice."""
import os
import subprocess

import pytest

from tests import merge_species_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("species_table") / "species_table_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # (the program carries its sanitizer runtimes: nothing of them is looked up at load time)
                    "-I", os.path.join(HERE, "..", "midas_amd", "csrc"), "-o", path, os.path.join(HERE, "cpp", "species_table_check.cpp")], check=True)
    return path


def table_by_the_program(exe, ids):
    r = subprocess.run([exe], input=''.join(K.raw(s).hex() + '\n' for s in ids), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.split('\n')[:-1]
    if lines == ['twice']:
        return None
    assert lines[0].startswith('table ') and len(lines) == 1 + len(ids), r.stdout
    return int(lines[0].split()[1]), [int(x.split()[0], 16) for x in lines[1:]], [int(x.split()[1]) for x in lines[1:]]


def id_lists():
    out = [(c['name'], c['ids']) for f in K.FAMILIES if f != 'write' for c in K.cases(f)]
    out += [('%d ids' % R, K.CANDIDATES[:R]) for R in (1, 7, 8, 15, 16, 17, 31, 32, 500)]
    out += [('the empty id', ['', 'a']), ('the empty id alone', ['']), ('bytes above 0x7F', [b'\xff\x80', b'\xff', b'\x80\xff', 'Spé']),
            ('a prefix and its extensions', ['Sp', 'Sp_', 'Sp_1', 'S']), ('a long id', ['x' * 3000, 'x' * 2999])]
    return out


def test_the_mirror_builds_the_table_the_library_builds(exe):
    sizes = set()
    for name, ids in id_lists():
        got = table_by_the_program(exe, ids)
        assert got is not None, name
        size, slot, at = K.table_of(ids)
        assert got[0] == size == K.table_size(len(ids)), name
        assert got[1] == [K.sm_hash(s) for s in ids], name
        assert got[2] == at, name
        assert [slot[k] for k in at] == list(range(1, len(ids) + 1)) and sum(1 for x in slot if x) == len(ids)
        sizes.add((len(ids), size))
    assert {(1, 16), (7, 16), (8, 32), (15, 32), (16, 64), (31, 64), (32, 128)} <= sizes


def test_an_id_listed_twice_is_refused_by_both(exe):
    full = K.named('table/seven_in_one_slot')['ids']
    for ids in (['a', 'a'], ['a', 'b', 'c', 'b'], ['', 'x', ''], full + full[6:], K.CANDIDATES[:16] + K.CANDIDATES[:1]):
        assert table_by_the_program(exe, ids) is None
        with pytest.raises(ValueError):
            K.table_of(ids)
    # equal hashes' low bits, equal lengths, other bytes: not the same id
    assert table_by_the_program(exe, full) is not None
