"""The direct layout's base byte (midas_amd/csrc/layout.h dense_byte / dense_threshold / dense_exact / dense_nibble / dense_qual),
compiled for the host from the header itself and checked against a Python model of what the pileup needs: for every 4-bit code
and every quality 0-255, `byte >= threshold` is the reference's "an A/C/G/T base with q >= baseq" for every baseq the direct
kernel serves, the bytes of the reads that are not exceptional decode to their SEQ / QUAL exactly, and the exceptional ones are
exactly those the byte cannot hold.  The device encoder and decoder themselves (dense_bases.h, built for the host with one lane a
group) are run on whole reads -- every length 0-40 and 150 / 151, pad nibbles, absent QUAL, the tail chunks -- against the model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "midas_amd", "csrc")
SRC = r'''
#define __host__
#define __device__
#define __forceinline__ inline
// stand-ins for the HIP names dense_bases.h uses: one lane a group (G = 1)
struct { unsigned x; } threadIdx;
inline int __shfl(int v, int) { return v; }
inline int __shfl_xor(int v, int) { return v; }
inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
inline unsigned atomicOr(unsigned* p, unsigned v) { unsigned o = *p; *p |= v; return o; }
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { unsigned long long o = *p; *p += v; return o; }
#include "dense_bases.h"
using namespace midas;
extern "C" {
// the device producers' encoder and the raw-column cut's decoder, one lane
int d_encode(unsigned char* dst, unsigned room, const unsigned char* seq, const unsigned char* qual, unsigned l, unsigned* flags) {
  DenseSide side{};
  const bool exc = dense::encode<1>(dst, room, seq, qual, l, 0, &side);
  *flags = side.flags;
  return exc ? 1 : 0;
}
void d_decode(unsigned char* seq, unsigned char* qual, const unsigned char* src, unsigned l) { dense::decode<1>(seq, qual, src, l, 0); }
int d_byte(unsigned nib, unsigned q) { return dense_byte(nib, q); }
int d_thr(int baseq) { return (int)dense_threshold(baseq); }
int d_exact(unsigned nib, unsigned q) { return dense_exact(nib, q) ? 1 : 0; }
int d_nib(unsigned b) { return (int)dense_nibble(b); }
int d_qual(unsigned b) { return (int)dense_qual(b); }
unsigned d_units(unsigned l, unsigned n) { return direct_payload_units(l, n); }
unsigned long long d_room(unsigned l) { return dense_side_room(l); }
}
'''
ACGT = {1: 0, 2: 1, 4: 2, 8: 3}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("dense")
    src, so = d / "dense.cpp", d / "dense.so"
    src.write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def model_byte(nib, q):
    if nib in ACGT:
        return ((min(q, 50) + 13) << 2) | ACGT[nib]
    return min(q, 51)


def test_every_code_and_quality(lib):
    for nib in range(16):
        for q in range(256):
            b = lib.d_byte(nib, q)
            assert b == model_byte(nib, q), (nib, q)
            assert (b >= 52) == (nib in ACGT)
            exact = lib.d_exact(nib, q) == 1
            assert exact == ((nib in ACGT and q <= 50) or (nib == 15 and q <= 51)), (nib, q)
            if exact:
                assert (lib.d_nib(b), lib.d_qual(b)) == (nib, q), (nib, q)
            if nib in ACGT:
                assert (b & 3) == ACGT[nib]


@pytest.mark.parametrize("baseq", list(range(-3, 96)) + [200, 255, 256])
def test_threshold_is_the_reference_comparison(lib, baseq):
    t = lib.d_thr(baseq)
    assert t == (256 if baseq > 50 else (max(baseq, 0) + 13) << 2)
    for nib in range(16):
        for q in range(256):
            counts = lib.d_byte(nib, q) >= t
            want = nib in ACGT and q >= baseq
            if q > 50 and nib in ACGT and baseq > 50:
                # the clamped case: the batch flag (kDenseClampedQual) sends such a run to the long path
                assert not counts
                continue
            assert counts == want, (baseq, nib, q)


@pytest.mark.parametrize("q", [49, 50, 51, 52])
def test_the_cap_boundaries(lib, q):
    for nib in (1, 2, 4, 8):
        assert lib.d_exact(nib, q) == (1 if q <= 50 else 0)
        assert lib.d_qual(lib.d_byte(nib, q)) == min(q, 50)
    assert lib.d_exact(15, q) == (1 if q <= 51 else 0)
    assert lib.d_byte(15, q) == min(q, 51)


def _encode(seq4, qual, l):
    """model of one read's payload part behind its CIGAR: the sum word, the bytes; and whether it is exceptional"""
    nib = [(seq4[j >> 1] >> (0 if j & 1 else 4)) & 15 for j in range(l)]
    absent = l > 0 and qual[0] == 0xFF
    word = int(sum(int(x) for x in qual[:l])) | (0x80000000 if absent else 0)
    exc = any(not ((n in ACGT and q <= 50) or (n == 15 and q <= 51)) for n, q in zip(nib, qual))
    exc = exc or (l % 2 == 1 and (seq4[l >> 1] & 15) != 0)
    return word, bytes(model_byte(n, int(q)) for n, q in zip(nib, qual)), exc


def _decode(b, l):
    seq4 = bytearray((l + 1) // 2)
    qual = bytearray(l)
    for j in range(l):
        x = b[j]
        n, q = ((1 << (x & 3)), (x >> 2) - 13) if x >= 52 else (15, x)
        seq4[j >> 1] |= n << (0 if j & 1 else 4)
        qual[j] = q
    return bytes(seq4), bytes(qual)


@pytest.mark.parametrize("l", [0, 1, 2, 7, 8, 9, 31, 150, 151])
def test_round_trip_and_exceptional_reads(lib, l):
    rng = np.random.default_rng(l)
    for trial in range(200):
        kind = trial % 5
        codes = rng.choice([1, 2, 4, 8, 15], size=l) if kind < 3 else rng.integers(0, 16, size=l)
        quals = rng.integers(0, 51, size=l) if kind < 2 else rng.integers(0, 256, size=l)
        if kind == 4 and l:
            quals[:] = 0xFF                      # absent QUAL
        seq4 = bytearray((l + 1) // 2)
        for j, n in enumerate(codes):
            seq4[j >> 1] |= int(n) << (0 if j & 1 else 4)
        if kind == 1 and l % 2:
            seq4[-1] |= 0x05                     # a nonzero pad nibble
        word, b, exc = _encode(seq4, quals, l)
        assert len(b) == l
        assert (word & 0x7FFFFFFF) == int(quals.sum())
        assert bool(word >> 31) == (l > 0 and int(quals[0]) == 0xFF)
        if not exc:
            assert _decode(b, l) == (bytes(seq4), bytes(int(q) for q in quals))
        else:
            assert kind >= 1 or l == 0
        units = lib.d_units(l, 3)
        assert units * 8 >= 12 + 4 + l and units * 8 < 12 + 4 + l + 8
        assert lib.d_room(l) >= (l + 1) // 2 + l and lib.d_room(l) % 8 == 0


def _run_encode(lib, seq4, quals, l):
    room = ((4 + l + 7) & ~7)
    dst = (C.c_ubyte * (room + 8))(*([0xAB] * (room + 8)))
    s = (C.c_ubyte * (len(seq4) + 8)).from_buffer_copy(bytes(seq4) + bytes(8))
    q = (C.c_ubyte * (l + 8)).from_buffer_copy(bytes(int(x) for x in quals) + bytes(8))
    flags = C.c_uint(0)
    exc = lib.d_encode(dst, room, s, q, l, C.byref(flags))
    out = bytes(dst)
    assert out[room:] == bytes([0xAB] * 8)           # nothing written past the read's units
    return int.from_bytes(out[:4], "little"), out[4:4 + l], out[4 + l:room], bool(exc), flags.value


def _run_decode(lib, b, l):
    seq = (C.c_ubyte * ((l + 1) // 2 + 8))()
    qual = (C.c_ubyte * (l + 8))()
    src = (C.c_ubyte * (l + 8)).from_buffer_copy(bytes(b) + bytes(8))
    lib.d_decode(seq, qual, src, l)
    assert bytes(seq)[(l + 1) // 2:] == bytes(8) and bytes(qual)[l:] == bytes(8)
    return bytes(seq)[:(l + 1) // 2], bytes(qual)[:l]


@pytest.mark.parametrize("l", list(range(0, 41)) + [150, 151])
def test_device_encoder_and_decoder(lib, l):
    rng = np.random.default_rng(1000 + l)
    for trial in range(120):
        kind = trial % 6
        codes = rng.choice([1, 2, 4, 8, 15], size=l) if kind < 3 else rng.integers(0, 16, size=l)
        quals = rng.integers(0, 51, size=l) if kind < 2 else rng.integers(0, 256, size=l)
        if kind == 5 and l:
            quals[:] = 0xFF
        seq4 = bytearray((l + 1) // 2)
        for j, n in enumerate(codes):
            seq4[j >> 1] |= int(n) << (0 if j & 1 else 4)
        if kind in (1, 4) and l % 2:
            seq4[-1] |= 0x05
        word, b, tail, exc, flags = _run_encode(lib, seq4, quals, l)
        mword, mb, mexc = _encode(seq4, quals, l)
        assert (word, b, exc) == (mword, mb, mexc), (l, trial)
        assert tail == bytes(len(tail))
        assert bool(flags & 1) == any(int(n) in ACGT and int(q) > 50 for n, q in zip(codes, quals))
        seq_d, qual_d = _run_decode(lib, b, l)
        assert (seq_d, qual_d) == _decode(b, l)
        if not exc:
            assert (seq_d, qual_d) == (bytes(seq4), bytes(int(q) for q in quals)), (l, trial)
