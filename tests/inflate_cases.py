"""Inputs of the device-inflate tests, built deterministically so that the host simulation
(test_inflate_cpu.py) and the GPU (test_inflate_gpu.py) see the same bytes.

A member is (payload, crc, isize): a raw deflate payload made with zlib.compressobj(level, DEFLATED,
-15, 8, strategy), or by hand, with the CRC32 and ISIZE its BGZF trailer claims.  A case is a short
chain of members.  The expected verdict of every member comes from zlib (`verdict`), never from a
hand-written table: a flipped padding bit is legitimately fine.

BGZF's BSIZE is 16 bits, so a member's payload is at most 65510 bytes: 65536 bytes cannot be framed
as stored blocks (level 0, or random bytes), and that size is covered by the compressible texts."""
import gzip
import os
import struct
import zlib

import numpy as np

INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
HEAD = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0])
SIZES = (0, 1, 2, 258, 259, 65279, 65280, 65536)
FLIPS = 64
_cache = {}


def text():
    if "text" not in _cache:
        _cache["text"] = gzip.open(os.path.join(INPUTS, "r1.fq.gz")).read()
    return _cache["text"]


def frame(member):
    payload, crc, isize = member
    assert len(payload) + 25 <= 0xFFFF
    return HEAD + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def chain(members):
    return b"".join(frame(m) for m in members)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for o in range(0, len(data), flush_every):
        out += c.compress(data[o:o + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
        if o == 0:
            out += c.flush(zlib.Z_FULL_FLUSH)  # (an empty stored block right after another)
    return out + c.flush()


def good(data, *args, **kw):
    return (deflate(data, *args, **kw), zlib.crc32(data), len(data))


def verdict(member):
    """(ok, bytes) as zlib sees the member: raw inflate capped at ISIZE + 1 bytes, then the length,
    then the CRC32.  Bytes after the last block's end are ignored, as the tool's host path does."""
    payload, crc, isize = member
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, isize + 1)
    except zlib.error:
        return False, b""
    if not d.eof or len(out) != isize or zlib.crc32(out) != crc & 0xFFFFFFFF:
        return False, out[:isize]
    return True, out


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def periodic(period, n, seed):
    unit = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8).tobytes()
    return (unit * (n // period + 1))[:n]


def valid_members():
    """name -> member; every one must come back OK and byte-identical to zlib."""
    if "valid" in _cache:
        return _cache["valid"]
    t = text()
    big = t[:65280]
    rnd = np.random.default_rng(7)
    R = rnd.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    skew = np.concatenate([np.full(f, 40 + 3 * i, np.uint8) for i, f in enumerate(fib(22))])
    np.random.default_rng(2).shuffle(skew)
    m = {}
    for n in SIZES:
        m["len%d" % n] = (b"\x03\x00", 0, 0) if n == 0 else good(t[:n])
    m["level0"] = good(big, 0)
    m["level0_blocks"] = good(t[:65000], 0, flush_every=20000)  # several stored blocks, empty ones between
    for n in (1, 2, 258, 259):
        m["level0_len%d" % n] = good(t[:n], 0)
    m["fixed"] = good(big, 6, zlib.Z_FIXED)
    m["fixed_65536"] = good(t[:65536], 6, zlib.Z_FIXED)
    m["huffman_only"] = good(big, 6, zlib.Z_HUFFMAN_ONLY)
    m["rle"] = good(big, 6, zlib.Z_RLE)
    for level in (1, 6, 9):
        m["level%d" % level] = good(t[70000:70000 + 65280], level)
    m["full_flush"] = good(big, 6, flush_every=3000)
    m["runs"] = good(b"A" * 65280)
    m["period3"] = good((b"abc" * 21760)[:65280])
    for p in (63, 64, 65):
        m["period%d" % p] = good(periodic(p, 20000 + p, p))
    # zlib never looks back further than 32506 bytes: the largest distance is encoded by hand
    tokens = list(R) + [(258, 32768)] * 126 + [(130, 32768)] * 2
    m["dist32768"] = (fixed_block(tokens), zlib.crc32(R + R), 65536)
    m["dist32768_zlib"] = good(R[:32000] + R[:32000], 9)
    m["skew"] = good(skew.tobytes())
    m["stored_random"] = good(np.random.default_rng(1).integers(0, 256, 65280, dtype=np.uint8).tobytes())
    _cache["valid"] = m
    return m


# decreasing, then increasing size (one handle serves every case)
def valid_order():
    m = valid_members()
    names = sorted(m, key=lambda k: (-m[k][2], k))
    return names + names[::-1]


def mixed_chain():
    """About 2 MiB of FASTQ text in members of every kind above, interleaved with the special ones,
    then the EOF member: a wave that strides over several members shows any state left behind."""
    t = text()
    kinds = [(6, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY),
             (6, zlib.Z_RLE), (1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY)]
    specials = [v for k, v in sorted(valid_members().items())]
    members, o, k = [], 0, 0
    while o < min(len(t), 2 << 20):
        n = (65280, 30000, 65536, 4097, 1)[k % 5]
        level, strategy = kinds[k % len(kinds)]
        if level == 0:
            n = min(n, 65280)
        members.append(good(t[o:o + n], level, strategy))
        if k < len(specials):
            members.append(specials[k])
        o += n
        k += 1
    members.append((b"\x03\x00", 0, 0))
    return members


class Bits:
    """Deflate's bit order: values from the least significant bit, Huffman codes from the most."""

    def __init__(self):
        self.out, self.v, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.v & 0xFF)
            self.v >>= 8
            self.n -= 8
        return self

    def code(self, value, nbits):
        for b in range(nbits - 1, -1, -1):
            self.put((value >> b) & 1, 1)
        return self

    def bytes(self, pad_to=0):
        out = bytes(self.out) + (bytes([self.v]) if self.n else b"")
        return out + b"\0" * max(0, pad_to - len(out))


def fixed_block(tokens):
    """One final fixed-Huffman block of literals (ints) and matches ((length, distance)), RFC 1951 3.2.6."""
    w = Bits().put(1, 1).put(1, 2)

    def lit(s):
        if s < 144:
            w.code(0x30 + s, 8)
        elif s < 256:
            w.code(0x190 + s - 144, 9)
        elif s < 280:
            w.code(s - 256, 7)
        else:
            w.code(0xC0 + s - 280, 8)

    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            l = length - 3
            if length == 258:
                lit(285)
            elif l < 8:
                lit(257 + l)
            else:
                e = l.bit_length() - 3
                lit(261 + 4 * e + ((l >> e) & 3))
                w.put(l & ((1 << e) - 1), e)
            d = dist - 1
            if d < 4:
                w.code(d, 5)
            else:
                e = d.bit_length() - 2
                w.code(2 * e + 2 + ((d >> e) & 1), 5)
                w.put(d & ((1 << e) - 1), e)
        else:
            lit(t)
    lit(256)
    return w.bytes()


def handmade():
    """name -> member: payloads no compressor writes; ISIZE and CRC are those of some plausible text."""
    t = text()[:1000]
    crc = zlib.crc32(t)
    h = {}
    h["block_type_3"] = (Bits().put(1, 1).put(3, 2).bytes(8), crc, len(t))
    h["hlit_287"] = (Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(15, 4).bytes(64), crc, len(t))
    over = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(15, 4)
    for _ in range(19):
        over.put(1, 3)
    h["oversubscribed_code_lengths"] = (over.bytes(64), crc, len(t))
    # the code-length code: symbols 0 and 16 with one bit each (0 -> code 0, 16 -> code 1); the
    # first length symbol is 16, "repeat the previous length", with nothing before it
    rep = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(1, 3).code(1, 1).put(0, 2)
    h["repeat_first"] = (rep.bytes(64), crc, len(t))
    h["stored_nlen"] = (b"\x01" + struct.pack("<HH", len(t), (len(t) ^ 0xFFFF) ^ 0x0100) + t, crc, len(t))
    # fixed block: literal 'a', then length 3 at distance 2 with one byte produced
    far = Bits().put(1, 1).put(1, 2).code(0x30 + 97, 8).code(1, 7).code(1, 5).code(0, 7)
    h["distance_before_start"] = (far.bytes(), zlib.crc32(b"aaaa"), 4)
    data = text()[:65280]
    p = deflate(data)
    h["cut_by_1"] = (p[:-1], zlib.crc32(data), len(data))
    h["cut_by_half"] = (p[:len(p) // 2], zlib.crc32(data), len(data))
    h["isize_minus_1"] = (p, zlib.crc32(data), len(data) - 1)
    h["isize_plus_1"] = (p, zlib.crc32(data), len(data) + 1)
    h["wrong_crc"] = (p, zlib.crc32(data) ^ 0x5A, len(data))
    return h


def flip_sources():
    data = text()[:65280]
    return {"dynamic": good(data), "fixed": good(data, 6, zlib.Z_FIXED), "stored": good(data, 0),
            "huffman_only": good(data, 6, zlib.Z_HUFFMAN_ONLY)}


def corrupt_cases():
    """name -> [good, corrupt, good]: every corrupt member stands between two good ones."""
    if "corrupt" in _cache:
        return _cache["corrupt"]
    t = text()
    before, after = good(t[100000:101000]), good(t[200000:203000], 1)
    cases = {}
    for kind, (payload, crc, isize) in sorted(flip_sources().items()):
        for k in range(FLIPS):
            p = bytearray(payload)
            p[(k * 2654435761) % len(p)] ^= 1 << (k % 8)
            cases["flip_%s_%02d" % (kind, k)] = [before, (bytes(p), crc, isize), after]
    for name, member in sorted(handmade().items()):
        cases[name] = [before, member, after]
    _cache["corrupt"] = cases
    return cases


def first_bad(members):
    for i, m in enumerate(members):
        if not verdict(m)[0]:
            return i
    return -1
