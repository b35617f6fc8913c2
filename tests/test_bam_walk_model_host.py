"""The fixtures of tests/test_gpu_bam_walk.py, proved on the CPU: for every one the model of the device record walk
(tests/bam_walk_model.py), stitched, finds exactly the records of the serial walk, and the file does what its name says -- the
guesses it is meant to make wrong ARE wrong in the model, in the direction claimed, as often as claimed.  No GPU test can pass on
a fixture that tests nothing.  The host decode reads every one of them and returns what was written."""
import numpy as np
import pytest

from midas_amd import abi
from tests import bam_walk_model as M


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("bam_walk_host")


def _agrees_with_the_serial_walk(fx):
    """the model's stitched records are the serial walk's; the host decode returns what was written"""
    t = fx.truth
    kept = t["refid"] >= 0
    assert fx.result["what"] == "settled"
    assert fx.offsets == [int(x) for x in t["offset"][kept]]
    assert fx.result["n_records"] == int(kept.sum()) == fx.reads.n_reads and fx.result["n_unmapped"] == int((~kept).sum()) == fx.dropped
    assert fx.result["first"] == fx.rec_begin and fx.result["end"] == fx.total
    unmapped = t["offset"][~kept]
    assert fx.result["first_unmapped"] == (int(unmapped[0]) if unmapped.size else M.NONE)
    for k, col in (("refid", fx.refid), ("pos", fx.reads.pos), ("mapq", fx.reads.mapq), ("flag", fx.reads.flag), ("l_seq", fx.reads.l_seq),
                   ("n_cigar", np.diff(fx.reads.cigar_off)), ("nm", fx.reads.nm)):
        np.testing.assert_array_equal(t[k][kept], np.asarray(col, np.int64), err_msg=k)
    _, _, rid, got = abi.read_bam(fx.path)
    np.testing.assert_array_equal(rid, fx.refid)
    for k in abi._SOA_DTYPES:
        np.testing.assert_array_equal(getattr(got, k), getattr(fx.reads, k), err_msg=k)
    # every chunk walked again had a guess that was not where the chain stood; no other chunk was touched
    assert sum(c["again"] for c in fx.chunks) == fx.again


def _wrong_guesses(fx):
    """(in front, behind): the chunks walked again whose guess lay in front of / behind the true boundary the chain brought"""
    front = [c for c in fx.chunks if c["again"] and c["guess"] != M.NONE and c["guess"] < c["start"]]
    behind = [c for c in fx.chunks if c["again"] and (c["guess"] == M.NONE or c["guess"] > c["start"])]
    return front, behind


def test_the_plain_file_makes_no_guess_wrong(tmp):
    """what profiles/genes_bam.txt records as `chunks_again 0`"""
    fx = M.plain(tmp)
    _agrees_with_the_serial_walk(fx)
    assert len(fx.chunks) == 50 and fx.total > 1600000
    assert fx.again == 0
    starts = fx.true_starts()
    assert all(c["guess"] in starts for c in fx.chunks)


def test_decoy4_every_decoy_costs_a_second_walk(tmp):
    fx = M.decoy4(tmp)
    _agrees_with_the_serial_walk(fx)
    placed = fx.facts["placed"]
    assert len(placed) >= 20
    assert fx.again == len(placed)
    front, behind = _wrong_guesses(fx)
    assert not behind and [(c["lo"] - fx.rec_begin) // M.CHUNK for c in front] == [c for c, _ in placed]
    starts = fx.true_starts()
    for c, at in placed:
        assert fx.chunks[c]["guess"] == at and at not in starts
    # some wrong walks met decoys without a reference, some turned bad: the second walk replaced both
    wrong = [M.walk(fx.stream, at, fx.chunks[c]["hi"], fx.total, fx.total) for c, at in placed]
    assert any(w[1] > 0 for w in wrong) and any(w[4] for w in wrong)
    assert fx.result["n_unmapped"] == 0


def test_decoy3_is_one_short_of_the_chain(tmp):
    fx = M.decoy3(tmp)
    _agrees_with_the_serial_walk(fx)
    assert len(fx.facts["placed"]) >= 20
    assert fx.again == 0
    # ... and with a chain of three the same file fools the scan: kChain is what stands between
    rec_begin, ref_lens = M.header(fx.stream)
    c, at = fx.facts["placed"][0]
    assert M.guess(fx.stream, fx.chunks[c]["lo"], fx.chunks[c]["hi"], fx.total, ref_lens, chain=3) == at != fx.chunks[c]["guess"]


def test_refused_names_put_the_guess_behind_the_boundary(tmp):
    fx = M.refused_names(tmp)
    _agrees_with_the_serial_walk(fx)
    changed = fx.facts["changed"]
    assert len(changed) == len(fx.chunks) - 1 == 49
    front, behind = _wrong_guesses(fx)
    assert not front and len(behind) == fx.again == 49
    for c, i in changed:
        ch = fx.chunks[c]
        assert ch["start"] == int(fx.truth["offset"][i]) and ch["guess"] == int(fx.truth["offset"][i + 1]) > ch["start"]
    raw =[bytes(fx.stream[int(o) + 36:int(o) + 36 + int(l) - 1]) for o, l in zip(fx.truth["offset"], fx.truth["l_name"])]
    assert any(b" " in raw[i] for _, i in changed) and any(max(raw[i]) >= 0x80 for _, i in changed)
    assert fx.total == M._plain(tmp)["total"]          # the offsets and the grid did not move


@pytest.mark.parametrize("d", M.BORDER_DISTANCES + ("end",))
def test_borders_a_record_starts_at_the_chosen_distance(tmp, d):
    fx = M.borders(tmp, d)
    _agrees_with_the_serial_walk(fx)
    assert fx.again == 0
    if d == "end":
        assert (fx.total - fx.rec_begin) % M.CHUNK == 0 and fx.chunks[-1]["hi"] - fx.chunks[-1]["lo"] == M.CHUNK
        return
    at = int(fx.truth["offset"][fx.facts["record"]])
    c = (at - fx.rec_begin) // M.CHUNK
    assert c >= 1 and at == fx.chunks[c]["lo"] + d
    if d in (0, 1):
        assert fx.chunks[c]["guess"] == at                      # the first record of its chunk
    else:
        assert fx.chunks[c + 1]["guess"] == at + int(fx.truth["size"][fx.facts["record"]])      # the last one: the next chunk begins inside it


@pytest.mark.parametrize("k", M.SHORT_TAILS)
def test_short_tail_the_chain_reaches_the_end_before_four_records(tmp, k):
    fx = M.short_tail(tmp, k)
    _agrees_with_the_serial_walk(fx)
    assert fx.again == 0
    last = fx.chunks[-1]
    if k == "under36":
        assert last["hi"] - last["lo"] == 35 and last["guess"] == M.NONE and last["start"] == M.NONE and last["kept"] == 0
        return
    at = int(fx.truth["offset"][-k])
    assert last["lo"] == at == last["guess"] and last["kept"] == k < M.CHAIN and last["end"] == fx.total
    assert M.guess(fx.stream, last["lo"] + 1, last["hi"], fx.total, M.header(fx.stream)[1]) == (int(fx.truth["offset"][-k + 1]) if k > 1 else M.NONE)


def test_end_decoy_is_taken_as_a_boundary(tmp):
    fx = M.end_decoy(tmp)
    _agrees_with_the_serial_walk(fx)
    at = fx.facts["decoy"]
    last = fx.chunks[-1]
    assert int(fx.truth["offset"][-1]) < last["lo"] == at and at not in fx.true_starts()        # the last record straddles the last border
    assert last["guess"] == at
    assert M.plausible(fx.stream, at, fx.total, M.header(fx.stream)[1]) + 4 + at == fx.total
    # The chain from the header's end passes the last chunk by (it stands at the stream's end): the chunk is emptied, not walked
    # again.  A grid that starts behind the last record's start has nothing else to go by: see the slices of the GPU test.
    assert fx.again == 0 and last["start"] == M.NONE and last["kept"] == 0
    rec_begin, ref_lens = M.header(fx.stream)
    assert M.guess(fx.stream, int(fx.truth["offset"][-1]) + 1, fx.total, fx.total, ref_lens) == at


def test_long_record_chunks_without_a_record_start(tmp):
    fx = M.long_record(tmp)
    _agrees_with_the_serial_walk(fx)
    o, size = int(fx.truth["offset"][M.LONG_AT]), int(fx.truth["size"][M.LONG_AT])
    assert size > 3 * M.CHUNK
    starts = fx.true_starts()
    inside = [c for c in fx.chunks if o < c["lo"] and c["hi"] <= o + size]          # no record starts in these
    assert len(inside) >= 3 and not any(c["lo"] <= s < c["hi"] for c in inside for s in starts)
    placed = dict(fx.facts["placed"])
    decoyed = [c for c in inside if (c["lo"] - fx.rec_begin) // M.CHUNK in placed]
    assert len(decoyed) >= 2
    for c in decoyed:            # the guess is the decoy; the chain passes the chunk by: emptied, not walked again
        assert c["guess"] == c["lo"] and c["start"] == M.NONE and c["kept"] == 0 and not c["again"]
    # the chunk in which the long record ends has a decoy too, and record starts behind it: that one is walked again
    ends_in = [c for c in fx.chunks if c["lo"] < o + size < c["hi"]]
    assert len(ends_in) == 1 and ends_in[0]["again"] and ends_in[0]["guess"] == ends_in[0]["lo"] and ends_in[0]["start"] == o + size
    assert fx.again == 1


def test_everywhere_many_guesses_are_wrong_on_any_grid(tmp):
    fx = M.everywhere(tmp)
    _agrees_with_the_serial_walk(fx)
    assert fx.again >= 20
    assert 20 <= fx.dropped <= 40 and len(set(fx.truth["l_name"])) >= 19
    starts = fx.true_starts()
    # the streamed decode's grids (five blocks a group) and the slices' are fooled as well, and settle on the same records
    groups, again, offs = M.streamed(fx.path, fx.stream, 5)
    assert groups >= 3 and again >= 20 and offs == fx.offsets
    for n in (2, 3):
        for k in range(n):
            u_lo, u_hi, r = M.slice_walk(fx.path, k, n, fx.stream)
            assert r is not None and u_lo < u_hi
            if r["what"] == "settled" and r["first"] in starts:
                assert r["end"] in starts or r["end"] == fx.total
