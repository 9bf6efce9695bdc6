"""Device BGZF (fq_deflate_bgzf): every member of the device's stream is checked field by field
and inflated with zlib, on inputs picked for the compressor's edges (member boundaries, one-symbol
alphabets, matches at exactly the window, no legal match, a forced stored block, skewed symbol
counts) and on real FASTQ text at several levels.  One handle serves all cases, in an order of
decreasing and then increasing size, so state left in the scratch by a larger input would show."""
import ctypes
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from fqtool_amd import abi

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
MAX_BYTES = 2 << 20
MEMBER = 65280


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def make_inputs():
    r1 = gzip.open(os.path.join(INPUTS, "r1.fq.gz")).read()[: 1 << 20]
    synth = gzip.open(os.path.join(INPUTS, "synth_r1.fq.gz")).read()
    assert len(synth) <= MAX_BYTES
    rnd = np.random.default_rng(7)
    R = rnd.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    R2 = rnd.integers(0, 256, 32769, dtype=np.uint8).tobytes()
    skew = np.concatenate([np.full(f, 40 + 3 * i, np.uint8) for i, f in enumerate(fib(22))])
    np.random.default_rng(2).shuffle(skew)
    cases = {"len%d" % n: r1[:n] for n in (0, 1, 2, 3, 4, 258, 259, 65279, 65280, 65281, 2 * MEMBER, 2 * MEMBER + 1)}
    cases["runs"] = b"A" * 70000
    cases["dist32768"] = R + R
    cases["no_legal_match"] = R2 + R2
    cases["stored"] = np.random.default_rng(1).integers(0, 256, MEMBER, dtype=np.uint8).tobytes()
    cases["all_bytes"] = bytes(range(256)) * 300
    cases["skew"] = skew.tobytes()
    cases["r1"] = r1
    cases["synth"] = synth
    return cases


@pytest.fixture(scope="module")
def inputs():
    return make_inputs()


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.fixture(scope="module")
def handle(lib):
    h = ctypes.c_void_p()
    assert lib.fq_deflate_create(0, MAX_BYTES, ctypes.byref(h)) == 0
    yield h
    lib.fq_deflate_destroy(h)


def device_bgzf(lib, h, data, level):
    n = len(data)
    bound = lib.fq_deflate_bound(n)
    src = np.frombuffer(data, np.uint8).copy() if n else np.zeros(1, np.uint8)
    out = np.full(bound + 64, 0xA5, np.uint8)
    got = ctypes.c_size_t(12345)
    rc = lib.fq_deflate_bgzf(h, src.ctypes.data, n, level, out.ctypes.data, bound, ctypes.byref(got))
    assert rc == 0
    assert got.value <= bound
    assert (out[got.value:] == 0xA5).all(), "bytes after the stream were written"
    return out[: got.value].tobytes()


def walk_blocks(payload):
    """The deflate payload must be whole blocks ending in one with BFINAL, and nothing after it."""
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    assert d.eof and d.unused_data == b""
    return out


def check_stream(stream, data):
    pos, parts = 0, []
    while pos < len(stream):
        h = stream[pos:pos + 18]
        assert len(h) == 18
        assert h[:4] == b"\x1f\x8b\x08\x04" and h[4:8] == b"\0\0\0\0", h
        assert h[8] == 4 and h[9] == 0xFF, "XFL 4 marks a member the device wrote"
        assert h[10:12] == b"\x06\x00" and h[12:14] == b"BC" and h[14:16] == b"\x02\x00"
        size = struct.unpack("<H", h[16:18])[0] + 1
        member = stream[pos:pos + size]
        assert len(member) == size and 26 < size <= 65536
        crc, isize = struct.unpack("<II", member[-8:])
        assert 0 < isize <= MEMBER
        plain = walk_blocks(member[18:-8])
        assert len(plain) == isize and zlib.crc32(plain) == crc
        d = zlib.decompressobj(31)
        assert d.decompress(member) == plain and d.eof
        assert size <= isize + 31
        parts.append(plain)
        pos += size
    assert pos == len(stream)
    assert len(parts) == -(-len(data) // MEMBER)
    assert all(len(p) == MEMBER for p in parts[:-1])
    assert b"".join(parts) == data


def zlib_members(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    total = 0
    for i in range(0, len(data), MEMBER):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += 26 + len(c.compress(data[i:i + MEMBER]) + c.flush())
    return total


# decreasing, then increasing size
ORDER = ["r1", "synth", "len130561", "len130560", "all_bytes", "runs", "no_legal_match", "dist32768", "len65281",
         "len65280", "stored", "len65279", "skew", "len259", "len258", "len4", "len3", "len2", "len1", "len0",
         "len1", "len2", "len3", "len4", "len258", "len259", "skew", "len65279", "stored", "len65280", "len65281",
         "dist32768", "no_legal_match", "runs", "all_bytes", "len130560", "len130561", "synth", "r1"]


def test_every_input_round_trips(lib, handle, inputs):
    assert set(ORDER) == set(inputs)
    for name in ORDER:
        data = inputs[name]
        stream = device_bgzf(lib, handle, data, 3)
        check_stream(stream, data)
        assert len(stream) <= lib.fq_deflate_bound(len(data)), name  # never larger than stored
        print("%-16s %8d -> %8d" % (name, len(data), len(stream)))


def test_matches_are_found_and_used(lib, handle, inputs):
    # runs: 70000 equal bytes must collapse (two members of a few hundred bytes); distance 32768:
    # the second half of R + R (within the first member) has matches only at exactly the window,
    # and random bytes gain nothing otherwise, so any gain over stored shows such matches in use
    # (the one-entry hash buckets keep only some positions that far back, so the gain is partial)
    assert len(device_bgzf(lib, handle, inputs["runs"], 3)) < 2000
    first = inputs["dist32768"][:MEMBER]
    s = device_bgzf(lib, handle, first, 3)
    check_stream(s, first)
    assert len(s) < MEMBER


def test_stored_block_when_nothing_compresses(lib, handle, inputs):
    s = device_bgzf(lib, handle, inputs["stored"], 3)
    assert len(s) == MEMBER + 31
    assert s[18] == 1 and s[19:23] == struct.pack("<HH", MEMBER, MEMBER ^ 0xFFFF)
    assert s[23:23 + MEMBER] == inputs["stored"]


@pytest.mark.parametrize("level", [1, 3, 6, 9])
def test_real_text_levels(lib, handle, inputs, level):
    for name in ("r1", "synth"):
        data = inputs[name]
        stream = device_bgzf(lib, handle, data, level)
        check_stream(stream, data)
        z = zlib_members(data, level)
        print("%s level %d: device %.4f zlib %.4f of the input, device/zlib %.3f" % (
            name, level, len(stream) / len(data), z / len(data), len(stream) / z))
        assert len(stream) <= lib.fq_deflate_bound(len(data))
        if name == "r1":
            assert len(stream) < zlib_members(data, 6, zlib.Z_HUFFMAN_ONLY)


def test_refusals(lib, handle, inputs):
    data = inputs["len65281"]
    n = len(data)
    src = np.frombuffer(data, np.uint8).copy()
    bound = lib.fq_deflate_bound(n)
    out = np.full(bound + 64, 0xA5, np.uint8)
    got = ctypes.c_size_t(0)
    args = (handle, src.ctypes.data, n)
    assert lib.fq_deflate_bgzf(*args, 3, out.ctypes.data, bound - 1, ctypes.byref(got)) == abi.FQ_E_INVALID
    assert lib.fq_deflate_bgzf(*args, 0, out.ctypes.data, bound, ctypes.byref(got)) == abi.FQ_E_INVALID
    assert lib.fq_deflate_bgzf(*args, 10, out.ctypes.data, bound, ctypes.byref(got)) == abi.FQ_E_INVALID
    big = np.zeros(MAX_BYTES + 1, np.uint8)
    bigout = np.full(lib.fq_deflate_bound(big.size), 0xA5, np.uint8)
    assert lib.fq_deflate_bgzf(handle, big.ctypes.data, big.size, 3, bigout.ctypes.data, bigout.size,
                               ctypes.byref(got)) == abi.FQ_E_INVALID
    assert (out == 0xA5).all() and (bigout == 0xA5).all()
    # the handle still works
    check_stream(device_bgzf(lib, handle, data, 3), data)
