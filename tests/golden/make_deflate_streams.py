"""Writes tests/golden/deflate_streams.json: raw DEFLATE streams as libdeflate writes them -- the encoder behind most real BAMs (htslib
built with libdeflate), whose dialect differs from zlib's: one long dynamic block where zlib ends a block after 16 383 symbols, other
match choices, other header spellings.  Four payloads at levels 1, 6 and 12.

Run on a developer's machine that has libdeflate.so.0 (loaded through ctypes); the tests never load it: they inflate the committed
streams with zlib (tests/test_deflate_writer_host.py) and on the device (tests/test_gpu_inflate_format.py)."""
import base64
import ctypes
import json
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def payloads():
    rng = np.random.default_rng(1951)
    # BAM-like: 4-bit bases two to a byte, then qualities from a short alphabet with runs
    bases = rng.integers(0, 4, 2 * 14000)
    nibbles = ((1 << bases[0::2]) << 4 | (1 << bases[1::2])).astype(np.uint8)
    quals = np.repeat(rng.choice(np.array([2, 11, 25, 37, 37, 37, 40], np.uint8), 7000), rng.integers(1, 6, 7000))[:20000]
    bam_like = nibbles.tobytes() + quals.astype(np.uint8).tobytes()
    noise = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 48 * 1024))
    rows = b"".join(b"contig_%04d\t%d\t%c\t%d\t%d\t%d\t%d\t%d\n" % (i // 900, i % 900 + 1, b"ACGT"[i % 4], *(int(x) for x in rng.poisson((9, 3, 0.2, 0.1, 0.1))))
                    for i in range(1500))
    mix = bytes(rng.integers(0, 256, 16000, dtype=np.uint8)) + rows[:11000] + b"\0" * 3000 + bytes(rng.integers(0, 256, 40, dtype=np.uint8))
    return [("bam_like", bam_like), ("four_letter_noise", noise), ("table_text", rows), ("mix_with_incompressible", mix)]


def main():
    lib = ctypes.CDLL("libdeflate.so.0")
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    streams = []
    for name, data in payloads():
        assert 8 * 1024 <= len(data) <= 48 * 1024, (name, len(data))
        for level in (1, 6, 12):
            c = lib.libdeflate_alloc_compressor(level)
            buf = ctypes.create_string_buffer(len(data) + 1024)
            n = lib.libdeflate_deflate_compress(c, data, len(data), buf, len(buf))
            lib.libdeflate_free_compressor(c)
            raw = buf.raw[:n]
            assert n > 0 and zlib.decompress(raw, -15) == data
            streams.append({"name": "%s/level%d" % (name, level), "size": len(data), "crc32": zlib.crc32(data), "raw": base64.b64encode(raw).decode()})
    path = os.path.join(HERE, "deflate_streams.json")
    with open(path, "w") as f:
        json.dump({"encoder": "libdeflate (libdeflate_deflate_compress), raw DEFLATE", "streams": streams}, f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", sum(len(base64.b64decode(s["raw"])) for s in streams), "compressed")
    assert os.path.getsize(path) <= 256 * 1024


if __name__ == "__main__":
    main()
