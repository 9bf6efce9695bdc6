"""Device inflate (fq_inflate_members, fq_inflate_bgzf) on the inputs of inflate_cases.py, the same
bytes the host simulation has been through (test_inflate_cpu.py): every valid member must come back
OK and byte-identical to zlib; of the corrupt ones the device may accept only what zlib accepts, its
good neighbours stay intact, and nothing is written past the output.  One handle serves all cases, in
an order of decreasing and then increasing size, so state left behind by a larger input would show."""
import ctypes
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import e2e_util as E
import inflate_cases as C
from fqtool_amd import abi

pytestmark = pytest.mark.gpu

MAX_IN = 4 << 20
MAX_OUT = 4 << 20
MAX_MEMBERS = 4096
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.fixture(scope="module")
def handle(lib):
    h = ctypes.c_void_p()
    assert lib.fq_inflate_create(0, MAX_IN, MAX_OUT, MAX_MEMBERS, ctypes.byref(h)) == 0
    yield h
    lib.fq_inflate_destroy(h)


def descriptors(members):
    arr = (abi.FqInflateMember * max(1, len(members)))()
    pos = 0
    for i, (payload, crc, isize) in enumerate(members):
        arr[i].in_off, arr[i].in_len, arr[i].isize, arr[i].crc = pos + 18, len(payload), isize, crc & 0xFFFFFFFF
        arr[i].status, arr[i].produced = 77, 0xFFFFFFFF
        pos += 18 + len(payload) + 8
    return arr


def run_members(lib, h, members):
    """[(status, produced, bytes of the member's range)] through fq_inflate_members."""
    comp = np.frombuffer(C.chain(members), np.uint8).copy()
    total = sum(m[2] for m in members)
    out = np.full(total + GUARD, 0xA5, np.uint8)
    arr = descriptors(members)
    bad = ctypes.c_size_t(12345)
    assert lib.fq_inflate_members(h, comp.ctypes.data, comp.size, arr, len(members), out.ctypes.data, total, ctypes.byref(bad)) == 0
    assert (out[total:] == 0xA5).all(), "bytes after out_cap were written"
    res, at = [], 0
    for i, m in enumerate(members):
        assert arr[i].produced <= m[2]
        res.append((arr[i].status, arr[i].produced, out[at:at + m[2]].tobytes()))
        at += m[2]
    assert bad.value == sum(r[0] != abi.FQ_INFL_OK for r in res)
    return res


def run_bgzf(lib, h, members):
    """(first_bad, output bytes) through fq_inflate_bgzf."""
    comp = np.frombuffer(C.chain(members), np.uint8).copy()
    total = sum(m[2] for m in members)
    out = np.full(total + GUARD, 0xA5, np.uint8)
    got, fb = ctypes.c_size_t(12345), ctypes.c_int64(12345)
    assert lib.fq_inflate_bgzf(h, comp.ctypes.data, comp.size, out.ctypes.data, total, ctypes.byref(got), ctypes.byref(fb)) == 0
    assert got.value == total
    assert (out[total:] == 0xA5).all(), "bytes after out_cap were written"
    return fb.value, out[:total].tobytes()


def check_against_zlib(members, res, must_be_ok=False):
    differ = []
    for i, (m, (st, produced, got)) in enumerate(zip(members, res)):
        ok, want = C.verdict(m)
        if st == abi.FQ_INFL_OK:
            assert ok, "member %d: accepted, zlib rejects it" % i
            assert produced == m[2] and got == want, "member %d differs from zlib's bytes" % i
        elif ok:
            differ.append(i)
        if must_be_ok:
            assert ok and st == abi.FQ_INFL_OK, "member %d: status %d" % (i, st)
    return differ


def test_valid_members(lib, handle):
    valid = C.valid_members()
    for name in C.valid_order():
        m = valid[name]
        check_against_zlib([m], run_members(lib, handle, [m]), must_be_ok=True)
        fb, out = run_bgzf(lib, handle, [m])
        assert fb == -1 and out == C.verdict(m)[1], name


def test_mixed_chain(lib, handle):
    members = C.mixed_chain()
    assert len(members) <= MAX_MEMBERS and sum(m[2] for m in members) > 2_000_000
    check_against_zlib(members, run_members(lib, handle, members), must_be_ok=True)
    fb, out = run_bgzf(lib, handle, members)
    assert fb == -1 and out == b"".join(C.verdict(m)[1] for m in members)
    print("inflate kernel: %.3f ms for %d bytes" % (lib.fq_inflate_last_kernel_ms(handle), len(out)))


def test_corrupt_members(lib, handle):
    cases = C.corrupt_cases()
    stricter, st = [], {}
    for k in sorted(cases):
        ms = cases[k]
        rs = run_members(lib, handle, ms)
        differ = check_against_zlib(ms, rs)
        assert rs[0][0] == abi.FQ_INFL_OK and rs[2][0] == abi.FQ_INFL_OK, k  # the good neighbours, intact
        assert rs[0][2] == C.verdict(ms[0])[1] and rs[2][2] == C.verdict(ms[2])[1], k
        want = C.first_bad(ms)
        fb, out = run_bgzf(lib, handle, ms)
        assert fb == want or (fb >= 0 and (want < 0 or fb < want)), (k, fb, want)
        assert out[:ms[0][2]] == rs[0][2] and out[len(out) - ms[2][2]:] == rs[2][2], k
        if differ or fb != want:
            stricter.append(k)
        if not k.startswith("flip_"):
            assert not C.verdict(ms[1])[0] and rs[1][0] != abi.FQ_INFL_OK, k
        st[k] = rs[1][0]
    for kind in C.flip_sources():
        rejected = sum(not C.verdict(cases[k][1])[0] for k in cases if k.startswith("flip_%s_" % kind))
        assert rejected >= 60, (kind, rejected)  # (keeps the test from going vacuous)
    print("members the device rejects and zlib accepts:", stricter)
    assert stricter == []
    assert st["block_type_3"] == st["hlit_287"] == st["oversubscribed_code_lengths"] == st["repeat_first"] == abi.FQ_INFL_DATA
    assert st["stored_nlen"] == st["distance_before_start"] == st["cut_by_1"] == st["cut_by_half"] == abi.FQ_INFL_DATA
    assert st["isize_minus_1"] == abi.FQ_INFL_LONG and st["isize_plus_1"] == abi.FQ_INFL_SHORT
    assert st["wrong_crc"] == abi.FQ_INFL_CRC


def bgzf_file_members(data):
    members, pos = [], 0
    while pos < len(data):
        assert data[pos:pos + 4] == b"\x1f\x8b\x08\x04" and data[pos + 10:pos + 16] == b"\x06\x00BC\x02\x00"
        size = int.from_bytes(data[pos + 16:pos + 18], "little") + 1
        members.append((data[pos + 18:pos + size - 8], int.from_bytes(data[pos + size - 8:pos + size - 4], "little"),
                        int.from_bytes(data[pos + size - 4:pos + size], "little")))
        pos += size
    assert pos == len(data)
    return members


def inflate_file(lib, h, data):
    comp = np.frombuffer(data, np.uint8).copy()
    total = sum(m[2] for m in bgzf_file_members(data))
    out = np.full(total + GUARD, 0xA5, np.uint8)
    got, fb = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.fq_inflate_bgzf(h, comp.ctypes.data, comp.size, out.ctypes.data, total, ctypes.byref(got), ctypes.byref(fb)) == 0
    assert got.value == total and fb.value == -1 and (out[total:] == 0xA5).all()
    return out[:total].tobytes()


@pytest.mark.parametrize("level", [1, 3, 9])
def test_streams_of_the_device_compressor(lib, handle, level):
    text = C.text()[: 1 << 20]
    d = ctypes.c_void_p()
    assert lib.fq_deflate_create(0, len(text), ctypes.byref(d)) == 0
    try:
        src = np.frombuffer(text, np.uint8).copy()
        bound = lib.fq_deflate_bound(len(text))
        comp = np.zeros(bound, np.uint8)
        n = ctypes.c_size_t(0)
        assert lib.fq_deflate_bgzf(d, src.ctypes.data, len(text), level, comp.ctypes.data, bound, ctypes.byref(n)) == 0
    finally:
        lib.fq_deflate_destroy(d)
    stream = comp[: n.value].tobytes()
    assert gzip.decompress(stream) == text
    assert inflate_file(lib, handle, stream) == text


def test_stream_of_the_host_writer(lib, handle, tmp_path):
    p = subprocess.run(E.argv_for(abi.FQTOOL_BIN, "td_pe_gz", str(tmp_path)), capture_output=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for name in ("o1.fq.gz", "o2.fq.gz"):
        data = (tmp_path / name).read_bytes()
        assert len(data) <= MAX_IN
        assert inflate_file(lib, handle, data) == gzip.decompress(data)


def test_refusals(lib, handle):
    valid = C.valid_members()
    ms = [valid["len259"], valid["level6"], valid["len1"]]
    comp = np.frombuffer(C.chain(ms), np.uint8).copy()
    total = sum(m[2] for m in ms)
    out = np.full(total + GUARD, 0xA5, np.uint8)
    bad = ctypes.c_size_t(0)

    def call(arr, n=len(ms), comp_bytes=comp.size, cap=total):
        return lib.fq_inflate_members(handle, comp.ctypes.data, comp_bytes, arr, n, out.ctypes.data, cap, ctypes.byref(bad))

    for field, value in (("in_len", abi.FQ_INFLATE_MAX + 1), ("isize", abi.FQ_INFLATE_MAX + 1), ("in_off", comp.size),
                         ("in_off", 1 << 40)):
        arr = descriptors(ms)
        setattr(arr[1], field, value)
        assert call(arr) == abi.FQ_E_INVALID, field
        assert arr[0].status == 77 and arr[1].status == 77
    arr = descriptors(ms)
    arr[2].in_off = comp.size - arr[2].in_len + 1  # the last payload one byte past the buffer
    assert call(arr) == abi.FQ_E_INVALID
    assert call(descriptors(ms), cap=total - 1) == abi.FQ_E_INVALID  # out_cap below the sum of ISIZE
    assert call(descriptors(ms), comp_bytes=MAX_IN + 1) == abi.FQ_E_INVALID
    many = (abi.FqInflateMember * (MAX_MEMBERS + 1))()
    assert call(many, n=MAX_MEMBERS + 1) == abi.FQ_E_INVALID
    big = (abi.FqInflateMember * 65)()  # 65 * 65536 > MAX_OUT
    for d in big:
        d.in_off, d.in_len, d.isize = 18, 2, 65536
    bigout = np.full(65 * 65536, 0xA5, np.uint8)
    assert lib.fq_inflate_members(handle, comp.ctypes.data, comp.size, big, 65, bigout.ctypes.data, bigout.size,
                                  ctypes.byref(bad)) == abi.FQ_E_INVALID
    # not an exact BGZF chain: a byte too many, a byte too few, a member without the BC field
    got, fb = ctypes.c_size_t(0), ctypes.c_int64(0)
    chain = C.chain(ms)
    for data in (chain + b"\0", chain[:-1], gzip.compress(b"plain gzip member, no extra field" * 3)):
        buf = np.frombuffer(data, np.uint8).copy()
        assert lib.fq_inflate_bgzf(handle, buf.ctypes.data, buf.size, out.ctypes.data, total, ctypes.byref(got),
                                   ctypes.byref(fb)) == abi.FQ_E_INVALID
    buf = np.frombuffer(chain, np.uint8).copy()
    assert lib.fq_inflate_bgzf(handle, buf.ctypes.data, buf.size, out.ctypes.data, total - 1, ctypes.byref(got),
                               ctypes.byref(fb)) == abi.FQ_E_INVALID
    assert (out == 0xA5).all() and (bigout == 0xA5).all(), "a refused call wrote something"
    # the handle still works
    check_against_zlib(ms, run_members(lib, handle, ms), must_be_ok=True)
