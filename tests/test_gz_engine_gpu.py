"""fq_engine_set_gz_out: text packs and raw packs whose output text is compressed on the device.

The drivers of test_text_gpu.py and test_raw_gpu.py run unchanged over a proxy of the library whose
fq_engine_create also turns gz output on, so everything they return (records, accumulators, adapter
strings) is compared with the oracle exactly as the plain tests do, and the output bytes, now BGZF
members, must inflate to the plain tests' expected text.  For the merged stream (-m) the reference
is the same driver's plain output (the merged text itself is checked by the end-to-end suite)."""
import ctypes
import gzip
import random
import struct
import zlib

import numpy as np
import pytest

from batch_util import config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi
from test_raw_gpu import adapter_strings, plain_fastq, run_raw
from test_text_gpu import expected_out, fastq_text, run_text

pytestmark = pytest.mark.gpu


class GzLib:
    """The engine library with gz output switched on in every engine it creates."""

    def __init__(self, lib, level=3):
        self._lib, self._level = lib, level

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def fq_engine_create(self, params, device, max_batch, max_stride, out):
        rc = self._lib.fq_engine_create(params, device, max_batch, max_stride, out)
        if rc == 0:
            assert self._lib.fq_engine_set_gz_out(out._obj, self._level) == 0
        return rc


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


def inflate_device_members(data):
    """Inflates a chain of BGZF members, every one of which the device must have written (XFL 4)."""
    pos, parts = 0, []
    while pos < len(data):
        h = data[pos:pos + 18]
        assert h[:4] == b"\x1f\x8b\x08\x04" and h[12:14] == b"BC", (pos, h)
        assert h[8] == 4, "member not written by the device"
        size = struct.unpack("<H", h[16:18])[0] + 1
        d = zlib.decompressobj(31)
        parts.append(d.decompress(data[pos:pos + size]))
        assert d.eof and d.unused_data == b""
        pos += size
    assert pos == len(data)
    plain = b"".join(parts)
    assert gzip.decompress(data) == plain
    return plain


@pytest.mark.parametrize("cfg", ["C3", "SE_all"])
@pytest.mark.parametrize("source", ["synth", "edge"])
def test_text_pack_gz(lib, oracle, cfg, source):
    paired = cfg != "SE_all"
    p = config(cfg, max_cycles=512)
    pk = synth_pack(oracle, 6000, paired, first=91) if source == "synth" else edge_pack(3000, paired)
    rng = random.Random(5)
    texts = [fastq_text(pk, m, rng) for m in ((1, 2) if paired else (1,))]
    res_o, acc_o = run_oracle(oracle, p, pk)
    res, acc, got = run_text(GzLib(lib), p, pk, texts)
    assert np.array_equal(res, res_o)
    assert np.array_equal(acc, acc_o)
    exp = expected_out(pk, res_o, paired, texts)
    for m in range(len(got)):
        assert source != "synth" or len(exp[m]) > 65280, "more than one member"
        assert inflate_device_members(got[m]) == exp[m], f"mate {m + 1}: inflated output differs"


@pytest.mark.parametrize("cfg", ["C3", "C2", "C4"])
@pytest.mark.parametrize("max_batch", [4096, 97])
def test_raw_stream_gz(lib, oracle, cfg, max_batch):
    paired = cfg != "C2"
    p = config(cfg, max_cycles=512)
    pk = synth_pack(oracle, 3000, paired, first=17)
    seed = zlib.crc32(("%s/%d" % (cfg, max_batch)).encode())
    texts = [plain_fastq(pk, m, random.Random(seed)) for m in ((1, 2) if paired else (1,))]
    res_o, acc_o = run_oracle(oracle, p, pk)
    packs, outs, ads, acc, stop = run_raw(GzLib(lib), p, [t[0] for t in texts], max_batch, 160, random.Random(seed))
    assert sum(packs) == pk.n and max(packs) <= max_batch, packs
    assert stop[0] is False
    assert np.array_equal(acc, acc_o)
    if cfg == "C4":  # the merged stream: the same windows with gz off
        _, exp, ads_plain, _, _ = run_raw(lib, p, [t[0] for t in texts], max_batch, 160, random.Random(seed))
        assert len(exp[0]) > 0 and exp[1] == b""
        assert ads == ads_plain
    else:
        exp = expected_out(pk, res_o, paired, [(None, None, t[2], t[3]) for t in texts])
    for m in range(len(outs)):
        assert inflate_device_members(outs[m]) == exp[m], f"mate {m + 1}: inflated output differs"
    want = adapter_strings(res_o, pk, p, paired)
    for m in range(len(ads)):
        assert ads[m] == want[m], f"mate {m + 1}: adapter strings differ"


def submit_text(lib, h, pk, texts, paired, seq_no, keep):
    tb = abi.FqTextBatch()
    tb.n, tb.stride = pk.n, pk.stride
    out = abi.FqTextOut()
    bufs = []
    for m in range(2 if paired else 1):
        text, recs = texts[m][0], texts[m][1]
        tb.text[m], tb.text_bytes[m], tb.rec[m] = text.ctypes.data, text.size, recs.ctypes.data
        ob = np.zeros(lib.fq_deflate_bound(text.size + 16), np.uint8)
        bufs.append(ob)
        out.text[m] = ob.ctypes.data
    res = pk.result_array()
    keep += [tb, out, bufs, res]
    assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), seq_no) == 0, \
        lib.fq_engine_last_error(h).decode()
    return out, bufs, res


def poll(lib, h, seq_no):
    seq = ctypes.c_uint64()
    assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
    assert seq.value == seq_no


def test_set_gz_out_rules_and_level_0(lib, oracle):
    """Refused while a pack is pending and for a bad level; level 0 gives plain text again on the
    same engine, and a later level compresses again."""
    p = config("C3", max_cycles=512)
    pk = synth_pack(oracle, 700, True, first=5)
    rng = random.Random(11)
    texts = [fastq_text(pk, m, rng) for m in (1, 2)]
    res_o, _ = run_oracle(oracle, p, pk)
    exp = expected_out(pk, res_o, True, texts)
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, pk.n, pk.stride, ctypes.byref(h)) == 0
    keep = []
    try:
        assert lib.fq_engine_set_gz_out(h, 10) == abi.FQ_E_INVALID
        assert lib.fq_engine_set_gz_out(h, -1) == abi.FQ_E_INVALID
        for k, level in enumerate((0, 3, 0, 9)):
            assert lib.fq_engine_set_gz_out(h, level) == 0
            out, bufs, res = submit_text(lib, h, pk, texts, True, k, keep)
            assert lib.fq_engine_set_gz_out(h, 1) == abi.FQ_E_INVALID  # a pack is pending
            poll(lib, h, k)
            assert np.array_equal(res, res_o)
            for m in range(2):
                got = bufs[m][: out.bytes[m]].tobytes()
                assert (inflate_device_members(got) if level else got) == exp[m], (level, m)
    finally:
        lib.fq_engine_destroy(h)


def test_records_only_egress_refused_with_gz(lib, oracle):
    p = config("C3", max_cycles=512)
    pk = synth_pack(oracle, 300, True, first=2)
    rng = random.Random(3)
    texts = [plain_fastq(pk, m, rng)[0] for m in (1, 2)]
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, 512, 160, ctypes.byref(h)) == 0
    try:
        assert lib.fq_engine_set_gz_out(h, 3) == 0
        wcap = max(t.size for t in texts)
        assert lib.fq_engine_raw_begin(h, wcap, 4096) == 0
        w = abi.FqRawWindow()
        for m in range(2):
            w.bytes[m], w.n[m] = texts[m].ctypes.data, texts[m].size
        assert lib.fq_engine_raw_enqueue(h, ctypes.byref(w)) == 0
        assert lib.fq_engine_set_gz_out(h, 0) == abi.FQ_E_INVALID  # a window is enqueued
        r, o = abi.FqRawResult(), abi.FqRawOut()
        results = np.zeros(2 * 512, np.dtype(abi.RESULT_DTYPE_FIELDS))
        recs = [np.zeros(512, np.dtype(abi.TEXT_REC_DTYPE)) for _ in range(2)]
        o.results = results.ctypes.data
        for m in range(2):
            o.rec[m] = recs[m].ctypes.data
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), 0) == abi.FQ_E_INVALID
        assert b"records-only" in lib.fq_engine_last_error(h)
        # the window is still there: with output buffers it runs
        o = abi.FqRawOut()
        bufs = [np.zeros(lib.fq_deflate_bound(4096 + wcap + 4 * 512 + 64), np.uint8) for _ in range(2)]
        for m in range(2):
            o.text.text[m] = bufs[m].ctypes.data
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), 0) == 0, lib.fq_engine_last_error(h).decode()
        poll(lib, h, 0)
        assert r.pairs == pk.n
        for m in range(2):
            assert inflate_device_members(bufs[m][: o.text.bytes[m]].tobytes()).count(b"\n") % 4 == 0
        assert lib.fq_engine_raw_end(h) == 0
    finally:
        lib.fq_engine_destroy(h)
