"""The library's two generic device primitives (device_sort.hip) on their own: the exclusive scan of 32-bit counters and the
stable radix sort of (key, value) pairs, through midas_snps_scan_u32 / midas_snps_sort_pairs -- the launches the packer, the
genes count and merge, the text front ends and the species steps use, on arrays of the tests' choosing.  The references are numpy
on the host ((cumsum - v) mod 2^32; argsort(kind='stable')) and every comparison is exact.  Every device buffer of a call lies
between guard words and the scratch buffers are exactly as large as the callers make them: each case asserts that no guard word
changed.

The sizes are the borders of the code: a thread's four counters, a workgroup's 4096, the one-workgroup in-place route against the
three-kernel route, and more than 4096 x 4096 counters, where the scan of the workgroups' sums goes round its carry loop more than
once (what a text front end does on any input above 256 MiB); for the sort a wave's round of 64, its quarter of 1024, the
workgroup's 4096 and the step of its histogram scan from one workgroup to three kernels between 65 536 and 65 537 pairs.

Not covered: sorts above 268 435 456 pairs, where the sort's own histogram scan would go round the carry loop -- the buffers alone
are more than 4 GiB, and the scan sizes here take the same launch_scan_u32 round that loop."""
import ctypes as C

import numpy as np
import pytest

from midas_amd import abi

pytestmark = pytest.mark.gpu

Z = 4096 * 4096                  # counters one round of the carry loop covers
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    with abi.Context(0) as c:
        yield c


def assert_same(got, exp, what):
    """exact equality of two arrays, naming the first index at which they differ"""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.flatnonzero(got != exp)
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: %d of %d differ, the first at index %d: got %s, expected %s (around it: got %s, expected %s)"
                             % (what, bad.size, got.size, i, got[i], exp[i], got[max(i - 2, 0):i + 3].tolist(), exp[max(i - 2, 0):i + 3].tolist()))


# ---- the scan ---------------------------------------------------------------------------------------------------------------------------

SCAN_SIZES = [0, 1, 3, 4, 5, 4095, 4096, 4097, 8191, 8192, 8193, 12289, Z - 1, Z, Z + 1, 2 * Z + 4099]
SCAN_DATA = ["ones", "newline_counts", "full_words", "spikes"]
SPIKES = (4095, 4096, Z - 1, Z)

_scan_case = {}


def scan_case(n, data):
    """(v, the expected prefix) of a size and a data set; the last one is kept, for the in-place and the out-of-place run"""
    if _scan_case.get("key") != (n, data):
        _scan_case.clear()
        rng = np.random.default_rng(1000 + 7 * n + SCAN_DATA.index(data))
        if data == "ones":                     # the prefix is the index: a failure names its place
            v = np.ones(n, np.uint32)
        elif data == "newline_counts":         # what a count of newlines per 16 bytes looks like
            v = rng.integers(0, 4, n, dtype=np.uint32)
        elif data == "full_words":             # the sums wrap every other counter
            v = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        else:                                  # a wrap right at a workgroup's border and at the carry loop's
            v = np.zeros(n, np.uint32)
            v[[p for p in SPIKES if p < n]] = M32
        exp = ((np.cumsum(v, dtype=np.uint64) - v) & M32).astype(np.uint32)
        v.setflags(write=False)
        exp.setflags(write=False)
        _scan_case.update(key=(n, data), v=v, exp=exp)
    return _scan_case["v"], _scan_case["exp"]


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("data", SCAN_DATA)
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_equals_the_prefix_sums_modulo_2_32(ctx, n, data, in_place):
    """(cumsum(v) - v) mod 2^32, exactly, in place and out of place, the guards untouched and -- out of place -- the input as it was.
    Z + 1 takes the second round of the carry loop for one sum, 2 Z + 4099 three rounds, the last one partial."""
    v, exp = scan_case(n, data)
    got, guards_ok, in_kept = ctx.scan_u32(v, in_place=in_place)
    assert guards_ok, "a guard word around in, out or sums changed (n = %d)" % n
    assert in_kept, "the out-of-place scan wrote to its input (n = %d)" % n
    assert_same(got, exp, "scan of %d counters (%s)" % (n, data))


# ---- the sort ---------------------------------------------------------------------------------------------------------------------------

KINDS = ["u32", "f64"]
# NaNs with payloads (quiet, signalling, negative), -0.0, the smallest and the largest subnormal, the infinities, 0.0
SPECIAL_BITS = np.array([0x7FF8000000000001, 0x7FF0000000000001, 0xFFF8DEADBEEF0123, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000,
                         0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000, 0], np.uint64)


def values(kind, n):
    """u32: the input index (inside equal keys the sorted values must ascend); f64: random 64-bit patterns and the special ones"""
    if kind == "u32":
        return np.arange(n, dtype=np.uint32)
    bits = np.random.default_rng(77 + n).integers(0, 1 << 64, n, dtype=np.uint64)
    bits[::5] = SPECIAL_BITS[np.arange(bits[::5].size) % SPECIAL_BITS.size]
    return bits.view(np.float64)


def uniform_keys(n, bits, seed=0):
    if bits == 0:
        return np.zeros(n, np.uint32)
    return np.random.default_rng(31 * n + bits + seed).integers(0, 1 << bits, n, dtype=np.uint64).astype(np.uint32)


def check_sort(ctx, key, bits, kind):
    n = key.size
    val = values(kind, n)
    key0, val0 = key.copy(), val.copy()
    got_key, got_val, which, guards_ok = ctx.sort_pairs(key, val, bits)
    assert guards_ok, "a guard word around a key buffer, a value buffer or the scratch changed (n = %d, bits = %d)" % (n, bits)
    # kernels.h: the result is "one of the two buffer pairs" -- every pass of eight bits goes from one pair to the other
    assert which == (0 if n == 0 else -(-bits // 8) % 2), (which, n, bits)
    assert key.tobytes() == key0.tobytes() and val.tobytes() == val0.tobytes()
    order = np.argsort(key, kind='stable')
    assert_same(got_key, key[order], "sorted keys (n = %d, bits = %d, %s)" % (n, bits, kind))
    if kind == "u32":
        assert got_val.dtype == np.uint32
        same_key = got_key[1:] == got_key[:-1]
        unstable = np.flatnonzero(same_key & (got_val[1:] <= got_val[:-1]))
        assert unstable.size == 0, "not stable: inside key %d input %d comes before input %d (output index %d; %d such places)" % (
            got_key[unstable[0]], got_val[unstable[0]], got_val[unstable[0] + 1], unstable[0], unstable.size)
        assert_same(got_val, val[order], "sorted values (n = %d, bits = %d, u32)" % (n, bits))
    else:
        assert got_val.dtype == np.float64
        assert_same(got_val.view(np.uint64), val.view(np.uint64)[order], "sorted values as bit patterns (n = %d, bits = %d, f64)" % (n, bits))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", [8, 17, 32])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65536, 65537, 200003])
def test_sort_at_the_size_borders(ctx, n, bits, kind):
    """Uniform keys below 2^bits at sizes around a wave's round (64), a wave's quarter (1024), the workgroup's 4096 pairs and the
    step of the histogram scan from one workgroup (65 536 pairs: 4096 counters) to three kernels (65 537)."""
    check_sort(ctx, uniform_keys(n, bits), bits, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", [0, 1, 3, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32])
def test_sort_at_every_number_of_passes(ctx, bits, kind):
    """bits that are and are not multiples of 8: ceil(bits / 8) passes; bits == 0: no pass, the output is the input."""
    key = uniform_keys(70001, bits, seed=5)
    if bits:
        assert int(key.max()) >> (bits - 1) == 1       # (the top bit of the range is in use)
    check_sort(ctx, key, bits, kind)


def key_shapes(n):
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(4242)
    shapes = {
        "all_equal": np.full(n, 0xDEADBEEF, np.int64),
        "two_keys": np.where(rng.random(n) < 0.5, 5, 0x80000000),
        "descending": (n - 1 - i) * 61001 + 7,              # strictly; every byte of the key varies
        "ascending": i * 61001 + 7,
        "top_byte_only": (rng.integers(0, 256, n) << 24) | 0x00ABCDEF,
        "heavy_key": np.where(rng.random(n) < 0.25, 0x01020304, rng.integers(0, 1 << 32, n)),
    }
    for s in (0, 8, 16, 24):
        shapes["64_digits_a_round_byte_%d" % (s // 8)] = (i % 64) << s          # all 64 lanes of a round differ in one pass, agree in the others
        shapes["one_digit_a_round_byte_%d" % (s // 8)] = (i // 64 % 256) << s   # all 64 lanes of a round share their digit in every pass
    assert all(int(k.min()) >= 0 and int(k.max()) <= M32 for k in shapes.values())
    return {name: k.astype(np.uint32) for name, k in shapes.items()}


N_SHAPES = 70001
KEY_SHAPES = key_shapes(N_SHAPES)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", sorted(KEY_SHAPES))
def test_sort_key_shapes(ctx, shape, kind):
    key = KEY_SHAPES[shape]
    if shape == "descending":
        assert (np.diff(key.astype(np.int64)) < 0).all()
    if shape == "heavy_key":
        assert 0.2 * N_SHAPES < int((key == 0x01020304).sum()) < 0.3 * N_SHAPES
    check_sort(ctx, key, 32, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_sort_a_million_pairs(ctx, kind):
    check_sort(ctx, uniform_keys(1 << 20, 20), 20, kind)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    """A negative n and bits outside 0..32 are MIDAS_SNPS_ERR_INVALID_ARG (answered before anything is allocated or launched); so is a
    null context."""
    v = np.ones(8, np.uint32)
    with pytest.raises(abi.MidasSnpsError) as ei:
        ctx.scan_u32(v, n=-1)
    assert ei.value.status == abi.ERR_INVALID_ARG
    for kind in KINDS:
        for n, bits in ((-1, 8), (8, 33), (8, -1)):
            with pytest.raises(abi.MidasSnpsError) as ei:
                ctx.sort_pairs(v, values(kind, 8), bits, n=n)
            assert ei.value.status == abi.ERR_INVALID_ARG, (kind, n, bits)
    lib = abi.load_library()
    out, a, b = np.zeros(8, np.uint32), C.c_int32(-1), C.c_int32(-1)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.midas_snps_scan_u32(None, 8, p(v), 0, p(out), C.byref(a), C.byref(b)) == abi.ERR_INVALID_ARG
    assert lib.midas_snps_sort_pairs(None, 8, 8, 0, p(v), p(v), p(out), p(out), C.byref(a), C.byref(b)) == abi.ERR_INVALID_ARG
    assert (a.value, b.value) == (-1, -1) and not out.any()
    # the context is as usable as before
    got, guards_ok, in_kept = ctx.scan_u32(v)
    assert guards_ok and in_kept and got.tolist() == list(range(8))
