"""UMI (-u) on the routed egress, on the GPU: with an egress and a UMI description set
(fq_engine_set_umi) routed text packs and the routed raw stream take the UMI configs; records equal
the oracle's and all six streams the Python model (tests/umi_util.py, pinned to the reference by
tests/test_umi_egress_cpu.py) byte for byte, on the synthetic pack of hostile names, for every
location and both flags.  Refusals come before anything is launched.  The binary takes the device
route on every UMI case of both golden manifests and writes the reference's outputs and reports."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import egress_util as G
import umi_util as U
from batch_util import run_oracle
from fqtool_amd import abi
from test_egress_gpu import create, text_batch
from test_egress_raw_gpu import corrected_pack, run_raw_routed
from test_raw_gpu import adapter_strings

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.fixture(scope="module")
def packs():
    """(paired, raw) -> (pack, its FASTQ text per mate): built once, never changed."""
    cache = {}

    def get(paired, raw=False):
        """raw: the raw stream's variant, lines ending in "\n" only and no empty read."""
        if (paired, raw) not in cache:
            cache[(paired, raw)] = U.synth_pack_and_texts(paired, crlf=not raw, min_len=1 if raw else 0)
        return cache[(paired, raw)]
    return get


@pytest.fixture(scope="module")
def records(oracle, packs):
    """(config, location, not_trim) -> (params, the oracle's records and accumulator), once per key."""
    cache = {}

    def get(cfg, loc, not_trim):
        key = (cfg, loc, not_trim)
        if key not in cache:
            p, _ = U.synth_params(cfg, loc, 0, not_trim)
            cache[key] = (p,) + tuple(run_oracle(oracle, p, packs(bool(p.paired))[0]))
        return cache[key]
    return get


def bounds(lib, texts, n, u):
    t1 = texts[0][0].size
    t2 = texts[1][0].size if len(texts) == 2 else 0
    return [lib.fq_egress_bound_umi(s, t1, t2, n, ctypes.byref(U.fq_umi(u)) if u else None) for s in range(G.STREAMS)]


def out_buffers(lib, texts, n, open_mask, u, shrink=None):
    """A buffer of exactly fq_egress_bound_umi per open stream (one byte less for `shrink`)."""
    out, keep = abi.FqEgressOut(), []
    for s, need in enumerate(bounds(lib, texts, n, u)):
        if not (open_mask >> s) & 1:
            continue
        cap = need - 1 if s == shrink else need
        buf = np.zeros(max(cap, 1), np.uint8)
        keep.append(buf)
        out.text[s], out.cap[s] = buf.ctypes.data, cap
    return out, keep


def submit_routed(lib, h, pk, texts, open_mask, u, seq_no):
    tb = text_batch(pk, texts)
    out, keep = out_buffers(lib, texts, pk.n, open_mask, u)
    res = pk.result_array()
    assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), seq_no) == 0, \
        lib.fq_engine_last_error(h).decode()
    seq = ctypes.c_uint64()
    assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
    assert seq.value == seq_no
    got = []
    for s in range(G.STREAMS):
        assert out.bytes[s] <= out.cap[s]
        got.append(ctypes.string_at(out.text[s], out.bytes[s]) if out.bytes[s] else b"")
    return res, got


# ---- 1. text packs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("loc", range(1, 7))
@pytest.mark.parametrize("cfg", U.SYNTH_CONFIGS)
def test_routed_text_pack_matches_model(lib, packs, records, cfg, loc):
    """Both flags at one location: records and accumulator the oracle's, every stream the model's."""
    open_mask = U.SYNTH_MASK[cfg]
    seen = [False] * G.STREAMS
    for not_trim in (0, 1):
        p, res_o, acc_o = records(cfg, loc, not_trim)
        pk, texts = packs(bool(p.paired))
        reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
        h = create(lib, p, pk)
        try:
            eg = abi.FqEgress(open_mask, 0)
            assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0, lib.fq_engine_last_error(h).decode()
            for k, drop in enumerate((0, 1)):
                _, u = U.synth_params(cfg, loc, drop, not_trim)
                assert lib.fq_engine_set_umi(h, ctypes.byref(U.fq_umi(u))) == 0, lib.fq_engine_last_error(h).decode()
                res, got = submit_routed(lib, h, pk, texts, open_mask, u, 7 + k)
                assert np.array_equal(res, res_o)
                exp = U.model(reads, res_o, bool(p.paired), bool(p.merge_enabled), False, open_mask, u)
                for s in range(G.STREAMS):
                    assert got[s] == exp[s], "%s, location %d, drop %d, not_trim %d: stream %s differs" % (
                        cfg, loc, drop, not_trim, G.STREAM_NAMES[s])
                    seen[s] = seen[s] or bool(exp[s])
                if k == 0:
                    acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
                    assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
                    assert np.array_equal(acc, acc_o)
        finally:
            lib.fq_engine_destroy(h)
    for s in range(G.STREAMS):
        assert seen[s] == bool((open_mask >> s) & 1), G.STREAM_NAMES[s]


# ---- 2. the raw stream ------------------------------------------------------------------------------
class UmiLib:
    """The engine library as tests/test_egress_raw_gpu.py's driver calls it, with the UMI description
    attached wherever an egress is set and the buffers sized by fq_egress_bound_umi."""

    def __init__(self, lib, u):
        self._lib, self._u = lib, U.fq_umi(u)

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def fq_engine_set_egress(self, h, eg):
        rc = self._lib.fq_engine_set_egress(h, eg)
        if rc == 0 and eg is not None:
            rc = self._lib.fq_engine_set_umi(h, ctypes.byref(self._u))
        return rc

    def fq_egress_bound(self, s, t1, t2, n):
        return self._lib.fq_egress_bound_umi(s, t1, t2, n, ctypes.byref(self._u))


# (location, drop_comment, not_trim): all four combinations where the location cuts reads (3, 4, 6), so
# that a NULL read's cut and location 6's cut-dependent quality part cross the windows' seam with the
# trim on and off; both values of each flag at the index locations
RAW_UMIS = [(loc, d, k) for loc in range(1, 7) for d in (0, 1) for k in (0, 1) if loc in (3, 4, 6) or d == k]


@pytest.mark.parametrize("loc,drop,not_trim", RAW_UMIS, ids=["%d-drop%d-keep%d" % t for t in RAW_UMIS])
@pytest.mark.parametrize("cfg", U.SYNTH_CONFIGS)
def test_routed_raw_stream_matches_model(lib, oracle, packs, cfg, loc, drop, not_trim):
    """The same reads (the empty ones given one base: the raw stream takes no empty line) through
    fq_engine_raw_begin ... fq_engine_raw_launch_routed: the first window
    holds about half the text, so a pair straddles the windows (the device carry); the driver also
    checks that a buffer one byte under the bound is refused and leaves the window enqueued."""
    p, u = U.synth_params(cfg, loc, drop, not_trim)
    paired = bool(p.paired)
    pk, texts = packs(paired, raw=True)
    res_o, acc_o = run_oracle(oracle, p, pk)
    # (the driver's refusal check shrinks OUT1's buffer: the pair streams are open in every config)
    open_mask = U.SYNTH_MASK[cfg] | (U.PAIR if paired else 0)
    rng = random.Random(11)
    packs_n, got, ads, acc, carry_max = run_raw_routed(UmiLib(lib, u), p, [t[0] for t in texts], open_mask, 4096, pk.stride, rng,
                                                       wcap=max(t[0].size for t in texts) // 2 + 2000)
    assert sum(packs_n) == pk.n and sum(1 for n in packs_n if n) >= 2 and carry_max > 0
    assert np.array_equal(acc, acc_o)
    reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
    exp = U.model(reads, res_o, paired, bool(p.merge_enabled), False, open_mask, u)
    for s in range(G.STREAMS):
        assert got[s] == exp[s], "stream %s differs" % G.STREAM_NAMES[s]
    corrected = bool((res_o["flags"] & abi.FQ_RF_CORRECTED).any())
    want = adapter_strings(res_o, corrected_pack(pk, res_o) if corrected else pk, p, paired)
    assert ads == want[:len(texts)]


# ---- 3. refusals ------------------------------------------------------------------------------------
def test_refusals(lib, packs, records):
    """No kernel is launched for a refused call: nothing is pending afterwards."""
    cfg, loc = "PE_umi", 6
    p, res_o, _ = records(cfg, loc, 0)
    _, u = U.synth_params(cfg, loc, 0, 0)
    pk, texts = packs(True)
    open_mask = U.SYNTH_MASK[cfg]
    h = create(lib, p, pk)
    try:
        tb = text_batch(pk, texts)
        res = pk.result_array()

        def routed(out):
            rc = lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), 1)
            assert lib.fq_engine_pending(h) == 0
            return rc
        full, keep = out_buffers(lib, texts, pk.n, open_mask, u)
        # a description without an egress: the routed calls and the raw stream refuse
        assert lib.fq_engine_set_umi(h, ctypes.byref(U.fq_umi(u))) == 0, lib.fq_engine_last_error(h).decode()
        assert routed(full) == abi.FQ_E_INVALID
        assert lib.fq_engine_raw_begin(h, 1 << 20, 1 << 16) == abi.FQ_E_INVALID
        eg = abi.FqEgress(open_mask, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        # descriptions that disagree with the params' umi_front1/2, or are out of range
        for bad in (U.Umi(6, u.length + 1, u.skip, 0, 0), U.Umi(3, u.length, u.skip, 0, 0), U.Umi(6, u.length, u.skip, 0, 1),
                    U.Umi(1, 0, 0, 0, 0), U.Umi(0, u.length, u.skip, 0, 0), U.Umi(7, u.length, u.skip, 0, 0),
                    U.Umi(6, -1, u.length + u.skip + 1, 0, 0)):
            assert lib.fq_engine_set_umi(h, ctypes.byref(U.fq_umi(bad))) == abi.FQ_E_INVALID, bad
        # (a refused description leaves the one set before in place)
        for s in (G.OUT1, G.UNPAIRED2, G.FAILED):  # one byte under fq_egress_bound_umi
            small, keep_s = out_buffers(lib, texts, pk.n, open_mask, u, shrink=s)
            assert routed(small) == abi.FQ_E_INVALID, G.STREAM_NAMES[s]
        # the plain calls keep refusing
        plain = abi.FqTextOut()
        bufs = [np.zeros(texts[m][0].size + 16, np.uint8) for m in range(2)]
        for m in range(2):
            plain.text[m] = bufs[m].ctypes.data
        assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(plain), 1) == abi.FQ_E_INVALID
        # inside a raw stream the description cannot change
        assert lib.fq_engine_raw_begin(h, 1 << 20, 1 << 16) == 0, lib.fq_engine_last_error(h).decode()
        assert lib.fq_engine_set_umi(h, None) == abi.FQ_E_INVALID
        assert lib.fq_engine_set_umi(h, ctypes.byref(U.fq_umi(u))) == abi.FQ_E_INVALID
        assert lib.fq_engine_raw_end(h) == 0
        # the pack still goes through, then without the description the old refusal is back
        got_res, got = submit_routed(lib, h, pk, texts, open_mask, u, 9)
        assert np.array_equal(got_res, res_o)
        assert lib.fq_engine_set_umi(h, None) == 0
        assert routed(full) == abi.FQ_E_INVALID
        assert b"take no UMI options" in lib.fq_engine_last_error(h)
        assert lib.fq_engine_raw_begin(h, 1 << 20, 1 << 16) == abi.FQ_E_INVALID
    finally:
        lib.fq_engine_destroy(h)


# ---- 4. the binary ----------------------------------------------------------------------------------
def run_tool(case, outdir, extra=()):
    p = subprocess.run(U.argv_for(abi.FQTOOL_BIN, case, str(outdir)) + list(extra), capture_output=True, cwd=outdir, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1, err[-2000:]
    return closing[0]


# (index filter + UMI stays on host packs)
TOOL_CASES = [c for c in U.ALL_CASES if "--enable_index_filter" not in U.entry(c)["args"]]


@pytest.mark.parametrize("case", TOOL_CASES, ids=["%s-%s" % c for c in TOOL_CASES])
def test_fqtool_takes_the_device_route(case, tmp_path):
    """The closing log line names the raw stream or text packs as what carried the UMI run (host packs
    before), and the outputs and reports are the reference's."""
    closing = run_tool(case, tmp_path)
    assert "(raw stream" in closing or "(text packs" in closing, closing
    # -u without --umi_location (location 0) tags and cuts nothing: it is routed only for its other outputs
    args = U.case_args(case)
    other = {"-c", "--failed_out", "--unpaired_read1", "--unpaired_read2", "--discard_unmerged"} & set(args)
    assert ("routed egress of" in closing) == bool(U.case_umi(case).location or other), closing
    U.check_outputs(case, str(tmp_path))


def test_fqtool_text_packs_on_two_engines(tmp_path):
    """Two engines share the run out as routed text packs of 777 pairs."""
    case = ("umi", "td_pe_umi_perread_comment")
    closing = run_tool(case, tmp_path, ["--devices", "0,0", "--pack_pairs", "777"])
    assert "(text packs" in closing and "routed egress of" in closing, closing
    U.check_outputs(case, str(tmp_path))
