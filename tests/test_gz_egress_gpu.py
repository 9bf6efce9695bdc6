"""fq_engine_set_gz_out on the routed egress: every open stream of a routed text pack and of a routed
raw pack comes back as BGZF members the device compressed (one multi-span launch per pack).

The drivers of test_egress_gpu.py, test_egress_raw_gpu.py and test_umi_egress_gpu.py run unchanged
over a proxy of the library whose fq_engine_create turns gz output on and whose fq_egress_bound(_umi)
is the bound of the stream's members, fq_deflate_bound(fq_egress_bound(_umi)(...)): records,
accumulators and adapter entries are compared with the oracle exactly as the plain tests do, and every
stream's bytes must be a chain of device members (XFL 4, ISIZE <= 65280) that inflates to the Python
model's text.  The drivers' own refusal checks (a buffer one byte below the bound) then test the
bound of the members."""
import ctypes
import random
import struct

import numpy as np
import pytest

import egress_util as G
import umi_util as U
from batch_util import config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi
from test_egress_gpu import CONFIGS, create, expected, out_buffers, params, run_routed, text_batch
from test_egress_raw_gpu import corrected_pack, run_raw_routed
from test_gz_engine_gpu import GzLib, inflate_device_members
from test_raw_gpu import adapter_strings, plain_fastq
from test_text_gpu import fastq_text
from test_umi_egress_gpu import submit_routed

pytestmark = pytest.mark.gpu

LEVELS = [1, 6]
PAIR = G.mask(G.OUT1, G.OUT2)


class GzEgressLib(GzLib):
    """GzLib whose routed bounds are those of the streams' members."""

    def fq_egress_bound(self, s, t1, t2, n):
        return self._lib.fq_deflate_bound(self._lib.fq_egress_bound(s, t1, t2, n))

    def fq_egress_bound_umi(self, s, t1, t2, n, u):
        return self._lib.fq_deflate_bound(self._lib.fq_egress_bound_umi(s, t1, t2, n, u))


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.fixture(scope="module")
def packs(oracle):
    """(source, paired) -> (pack, its FASTQ text per mate): built once, never changed.  synth: about
    1,500 pairs of 150 bp, 0.5 MB a mate, so the pair streams span several members."""
    cache = {}

    def get(source, paired):
        key = (source, paired)
        if key not in cache:
            pk = synth_pack(oracle, 1500, paired, first=91) if source == "synth" else edge_pack(3000, paired)
            rng = random.Random(5)
            cache[key] = (pk, [fastq_text(pk, m, rng) for m in ((1, 2) if paired else (1,))])
        return cache[key]
    return get


@pytest.fixture(scope="module")
def oracle_runs(oracle, packs):
    """(config name, source) -> (params, open mask, the oracle's records and accumulator, the model's streams)."""
    cache = {}

    def get(name, source):
        if (name, source) not in cache:
            p, open_mask = params(name)
            pk, texts = packs(source, bool(p.paired))
            res_o, acc_o = run_oracle(oracle, p, pk)
            cache[(name, source)] = (p, open_mask, res_o, acc_o, expected(pk, texts, p, res_o, open_mask))
        return cache[(name, source)]
    return get


def members_of(data):
    """(XFL, ISIZE) of every member of a BGZF chain."""
    pos, out = 0, []
    while pos < len(data):
        size = struct.unpack("<H", data[pos + 16:pos + 18])[0] + 1
        out.append((data[pos + 8], struct.unpack("<I", data[pos + size - 4:pos + size])[0]))
        pos += size
    assert pos == len(data)
    return out


def check_streams(got, exp, open_mask, what):
    for s in range(G.STREAMS):
        name = "%s: stream %s" % (what, G.STREAM_NAMES[s])
        if not exp[s]:
            assert got[s] == b"", name + " has bytes though nothing was routed to it"
            continue
        assert (open_mask >> s) & 1, name
        assert inflate_device_members(got[s]) == exp[s], name + ": inflated text differs"  # (valid chain, XFL 4)
        mem = members_of(got[s])
        assert all(x == 4 and 0 < n <= 65280 for x, n in mem), name
        assert len(mem) == (len(exp[s]) + 65279) // 65280, name
        assert len(got[s]) <= len(exp[s]) + 31 * len(mem), name


# all five non-merged streams, -c, -m --discard_unmerged, single end with --failed_out
TEXT_CONFIGS = ["PE_all+failed+unpaired", "PE_correct", "C4+discard+all", "SE_all+failed"]


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", TEXT_CONFIGS)
def test_routed_text_pack_gz(lib, oracle_runs, packs, name, level):
    assert name in CONFIGS
    several, short = False, False
    for source in ("synth", "edge"):
        p, open_mask, res_o, acc_o, exp = oracle_runs(name, source)
        pk, texts = packs(source, bool(p.paired))
        res, acc, got = run_routed(GzEgressLib(lib, level), p, pk, texts, open_mask)
        assert np.array_equal(res, res_o), source
        assert np.array_equal(acc, acc_o), source
        check_streams(got, exp, open_mask, "%s, %s, level %d" % (name, source, level))
        several = several or any(len(x) > 2 * 65280 for x in exp)
        short = short or any(0 < len(x) < 65280 for x in exp)
    assert several and short  # streams of several members and of less than one, in one pack


@pytest.mark.parametrize("level", LEVELS)
def test_routed_text_pack_gz_umi(lib, oracle, packs, level):
    """One UMI location (per_read: the tag comes from both reads' bases) on the paired config with
    the pair, unpaired and failed streams."""
    cfg, open_mask = "PE_umi", U.SYNTH_MASK["PE_umi"]
    p, u = U.synth_params(cfg, 6, 0, 0)
    gz = GzEgressLib(lib, level)
    for source in ("synth", "edge"):
        pk, texts = packs(source, True)
        res_o, acc_o = run_oracle(oracle, p, pk)
        reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(2)]
        exp = U.model(reads, res_o, True, bool(p.merge_enabled), False, open_mask, u)
        h = create(gz, p, pk)
        try:
            eg = abi.FqEgress(open_mask, 0)
            assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0, lib.fq_engine_last_error(h).decode()
            assert lib.fq_engine_set_umi(h, ctypes.byref(U.fq_umi(u))) == 0, lib.fq_engine_last_error(h).decode()
            res, got = submit_routed(gz, h, pk, texts, open_mask, u, 7)
            acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
            assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
        finally:
            lib.fq_engine_destroy(h)
        assert np.array_equal(res, res_o) and np.array_equal(acc, acc_o), source
        assert any(b" OX:Z:" in x for x in exp)
        check_streams(got, exp, open_mask, "%s, %s, level %d" % (cfg, source, level))


# ---- the raw stream ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_pack(oracle):
    pk = synth_pack(oracle, 3000, True, first=17)
    rng = random.Random(11)
    return pk, [plain_fastq(pk, m, rng) for m in (1, 2)]


@pytest.mark.parametrize("cfg,open_mask", [
    ("PE_correct", PAIR | G.mask(G.UNPAIRED1, G.UNPAIRED2, G.FAILED)),
    ("PE_all", PAIR | G.mask(G.UNPAIRED1, G.UNPAIRED2, G.FAILED)),
])
def test_routed_raw_stream_gz(lib, oracle, raw_pack, cfg, open_mask):
    """Random-cut windows: the members of each stream over the packs, concatenated, inflate to the
    model's stream; the adapter entries stay uncompressed in their own buffers.  (The driver also
    checks that a buffer one byte below the members' bound is refused with the window left enqueued.)"""
    p = config(cfg, max_cycles=512)
    pk, texts = raw_pack
    res_o, acc_o = run_oracle(oracle, p, pk)
    rng = random.Random(13)
    packs, got, ads, acc, carry_max = run_raw_routed(GzEgressLib(lib, 6), p, [t[0] for t in texts], open_mask, 4096, pk.stride,
                                                      rng, wcap=max(t[0].size for t in texts) // 2 + 2000)
    assert sum(packs) == pk.n and sum(1 for n in packs if n) >= 2 and carry_max > 0  # two windows with a carry
    assert np.array_equal(acc, acc_o)
    reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(2)]
    exp = G.model(reads, res_o, True, False, False, open_mask)
    assert exp[G.OUT1] and exp[G.OUT2] and exp[G.FAILED] and exp[G.UNPAIRED1]
    for s in range(G.STREAMS):
        name = "stream %s" % G.STREAM_NAMES[s]
        assert not exp[s] or (open_mask >> s) & 1, name
        assert (inflate_device_members(got[s]) if exp[s] else got[s]) == exp[s], name
        assert all(x == 4 and 0 < n <= 65280 for x, n in members_of(got[s])), name
    corrected = bool((res_o["flags"] & abi.FQ_RF_CORRECTED).any())
    assert corrected == bool(p.correction_enabled)
    want = adapter_strings(res_o, corrected_pack(pk, res_o) if corrected else pk, p, True)
    assert sum(want[0].values()) > 0 and sum(want[1].values()) > 0
    assert ads == want


# ---- refusals ---------------------------------------------------------------------------------------
def test_text_pack_buffer_below_the_members_bound_is_refused(lib, packs):
    p, open_mask = params("PE_all+failed+unpaired")
    pk, texts = packs("edge", True)
    gz = GzEgressLib(lib, 3)
    h = create(gz, p, pk)
    try:
        eg = abi.FqEgress(open_mask, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        tb = text_batch(pk, texts)
        res = pk.result_array()
        for s in (G.OUT1, G.UNPAIRED2, G.FAILED):  # one byte under fq_deflate_bound(fq_egress_bound(...))
            small, keep = out_buffers(gz, pk, texts, open_mask, shrink=s)
            assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(small), 1) == abi.FQ_E_INVALID
            assert lib.fq_engine_pending(h) == 0, G.STREAM_NAMES[s]
        # (buffers of the text's bound alone are too small as well)
        plain, keep = out_buffers(lib, pk, texts, open_mask)
        assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(plain), 1) == abi.FQ_E_INVALID
        assert lib.fq_engine_pending(h) == 0
    finally:
        lib.fq_engine_destroy(h)


def test_records_only_egress_stays_refused_with_an_egress_set(lib, raw_pack):
    p = config("PE_all", max_cycles=512)
    pk, texts = raw_pack
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, 4096, pk.stride, ctypes.byref(h)) == 0
    try:
        assert lib.fq_engine_set_gz_out(h, 3) == 0
        eg = abi.FqEgress(PAIR | G.mask(G.FAILED), 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        assert lib.fq_engine_raw_begin(h, max(t[0].size for t in texts), 4096) == 0, lib.fq_engine_last_error(h).decode()
        w = abi.FqRawWindow()
        for m in range(2):
            w.bytes[m], w.n[m] = texts[m][0].ctypes.data, texts[m][0].size
        assert lib.fq_engine_raw_enqueue(h, ctypes.byref(w)) == 0
        r, o = abi.FqRawResult(), abi.FqRawOut()
        results = np.zeros(2 * 4096, np.dtype(abi.RESULT_DTYPE_FIELDS))
        recs = [np.zeros(4096, np.dtype(abi.TEXT_REC_DTYPE)) for _ in range(2)]
        o.results = results.ctypes.data
        for m in range(2):
            o.rec[m] = recs[m].ctypes.data
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), 0) == abi.FQ_E_INVALID
        assert b"records-only" in lib.fq_engine_last_error(h)
        assert lib.fq_engine_pending(h) == 0
        assert lib.fq_engine_raw_end(h) == 0
    finally:
        lib.fq_engine_destroy(h)
