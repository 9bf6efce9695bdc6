"""Routed text packs (fq_engine_set_egress + fq_engine_submit_text_routed) against the oracle and
the Python model of the six output streams (tests/egress_util.py, pinned to the reference by
tests/test_egress_cpu.py): records and accumulator bit-exact, every stream byte-identical, on the
ragged / CRLF / named-strand-line text of tests/test_text_gpu.py; -c pairs come back from the
corrected rows of the tile planes.  Validation: buffers below fq_egress_bound and open streams
without a buffer are refused before launch, and without an egress the old refusals stand.
The raw-stream variant is in tests/test_egress_raw_gpu.py."""
import ctypes
import random

import numpy as np
import pytest

import egress_util as G
from batch_util import config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi
from test_text_gpu import fastq_text

pytestmark = pytest.mark.gpu

PAIR = G.mask(G.OUT1, G.OUT2)
UNP = G.mask(G.UNPAIRED1, G.UNPAIRED2)
FAIL = G.mask(G.FAILED)
MRG = G.mask(G.MERGED)

# name -> (config, --discard_unmerged, the streams with a writer)
CONFIGS = {
    "PE_all+failed": ("PE_all", 0, PAIR | FAIL),
    "PE_all+failed+unpaired": ("PE_all", 0, PAIR | FAIL | UNP),
    "PE_all+unpaired1": ("PE_all", 0, PAIR | G.mask(G.UNPAIRED1)),
    "C4+discard+all": ("C4", 1, PAIR | MRG | FAIL | UNP),
    "PE_correct": ("PE_correct", 0, PAIR),
    "PE_correct+all": ("PE_correct", 0, PAIR | FAIL | UNP),
    "PE_correct_x": ("PE_correct_x", 0, PAIR),
    "PE_correct_x+all": ("PE_correct_x", 0, PAIR | FAIL | UNP),
    "PE_correct_merge": ("PE_correct_merge", 0, MRG | FAIL | UNP),
    "PE_correct_merge+discard": ("PE_correct_merge", 1, PAIR | MRG | FAIL | UNP),
    "SE_all+failed": ("SE_all", 0, G.mask(G.OUT1) | FAIL),
}


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.fixture(scope="module")
def packs(oracle):
    """(source, paired) -> (pack, its FASTQ text per mate): built once, never changed."""
    cache = {}

    def get(source, paired):
        key = (source, paired)
        if key not in cache:
            pk = synth_pack(oracle, 6000, paired, first=91) if source == "synth" else edge_pack(3000, paired)
            rng = random.Random(5)
            cache[key] = (pk, [fastq_text(pk, m, rng) for m in ((1, 2) if paired else (1,))])
        return cache[key]
    return get


def params(name):
    cfg, discard, open_mask = CONFIGS[name]
    p = config(cfg, max_cycles=512)
    p.discard_unmerged = discard
    return p, open_mask


def expected(pk, texts, p, res, open_mask):
    reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
    return G.model(reads, res, bool(p.paired), bool(p.merge_enabled), bool(p.discard_unmerged), open_mask)


def text_batch(pk, texts):
    tb = abi.FqTextBatch()
    tb.n, tb.stride = pk.n, pk.stride
    for m in range(len(texts)):
        tb.text[m], tb.text_bytes[m], tb.rec[m] = texts[m][0].ctypes.data, texts[m][0].size, texts[m][1].ctypes.data
    return tb


def bounds(lib, pk, texts):
    t1 = texts[0][0].size
    t2 = texts[1][0].size if len(texts) == 2 else 0
    return [lib.fq_egress_bound(s, t1, t2, pk.n) for s in range(G.STREAMS)]


def out_buffers(lib, pk, texts, open_mask, shrink=None, drop=None):
    """The descriptor with a buffer of exactly the bound per open stream (one byte less for `shrink`,
    none for `drop`)."""
    out = abi.FqEgressOut()
    keep = []
    for s, need in enumerate(bounds(lib, pk, texts)):
        if not (open_mask >> s) & 1 or s == drop:
            continue
        cap = need - 1 if s == shrink else need
        buf = np.zeros(max(cap, 1), np.uint8)
        keep.append(buf)
        out.text[s], out.cap[s] = buf.ctypes.data, cap
    return out, keep


def create(lib, p, pk):
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, max(pk.n, 1), pk.stride, ctypes.byref(h)) == 0, \
        lib.fq_engine_last_error(None).decode()
    return h


def run_routed(lib, p, pk, texts, open_mask, seq_no=7):
    h = create(lib, p, pk)
    try:
        eg = abi.FqEgress(open_mask, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0, lib.fq_engine_last_error(h).decode()
        tb = text_batch(pk, texts)
        out, keep = out_buffers(lib, pk, texts, open_mask)
        res = pk.result_array()
        assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), seq_no) == 0, \
            lib.fq_engine_last_error(h).decode()
        seq = ctypes.c_uint64()
        assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
        assert seq.value == seq_no
        acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
        assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
        got = []
        for s in range(G.STREAMS):
            assert out.bytes[s] <= out.cap[s]
            got.append(ctypes.string_at(out.text[s], out.bytes[s]) if out.bytes[s] else b"")
        return res, acc, got
    finally:
        lib.fq_engine_destroy(h)


def check(lib, oracle, packs, name):
    """Both sources: records, accumulator and every stream; each open stream non-empty at least once."""
    p, open_mask = params(name)
    seen, corrected = [False] * G.STREAMS, False
    for source in ("synth", "edge"):
        pk, texts = packs(source, bool(p.paired))
        res_o, acc_o = run_oracle(oracle, p, pk)
        res, acc, got = run_routed(lib, p, pk, texts, open_mask)
        assert np.array_equal(res, res_o), source
        assert np.array_equal(acc, acc_o), source
        exp = expected(pk, texts, p, res_o, open_mask)
        for s in range(G.STREAMS):
            assert got[s] == exp[s], "%s, %s: stream %s differs" % (name, source, G.STREAM_NAMES[s])
            seen[s] = seen[s] or bool(exp[s])
        corrected = corrected or bool((res_o["flags"] & abi.FQ_RF_CORRECTED).any())
    assert corrected == bool(p.correction_enabled and p.paired)  # (-c configs do read rows back from the planes)
    for s in range(G.STREAMS):
        assert seen[s] == bool((open_mask >> s) & 1), "%s: stream %s" % (name, G.STREAM_NAMES[s])


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_routed_text_pack_matches_model(lib, oracle, packs, name):
    check(lib, oracle, packs, name)


@pytest.mark.parametrize("mode", ["fast", "general"])
def test_routed_correction_in_both_dispatch_modes(lib, oracle, packs, monkeypatch, mode):
    monkeypatch.setenv("FQ_ENGINE_GENERAL_ONLY", "1" if mode == "general" else "0")
    check(lib, oracle, packs, "PE_correct_x+all")


def test_last_record_without_terminator(lib, oracle, packs):
    """An input whose last line lacks its terminator: each stream still ends its records with one."""
    p, open_mask = params("PE_all+failed+unpaired")
    pk, texts = packs("edge", True)
    texts = list(texts)
    for m in range(2):  # drop the final "\n" (and a "\r" before it)
        t = texts[m][0]
        cut = 2 if t.size >= 2 and t[-2] == 13 else 1
        texts[m] = (t[:-cut].copy(),) + texts[m][1:]
    res_o, _ = run_oracle(oracle, p, pk)
    res, _, got = run_routed(lib, p, pk, texts, open_mask)
    assert np.array_equal(res, res_o)
    assert got == expected(pk, texts, p, res_o, open_mask)


def test_empty_pack(lib, oracle, packs):
    p, open_mask = params("PE_all+failed")
    pk, _ = packs("edge", True)
    h = create(lib, p, pk)
    try:
        eg = abi.FqEgress(open_mask, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        tb = abi.FqTextBatch()
        tb.n, tb.stride = 0, pk.stride
        out = abi.FqEgressOut()
        keep = [np.zeros(16, np.uint8) for _ in range(G.STREAMS)]
        for s in range(G.STREAMS):
            out.text[s], out.cap[s], out.bytes[s] = keep[s].ctypes.data, 16, 99
        res = pk.result_array()
        assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), 3) == 0
        seq = ctypes.c_uint64()
        assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1 and seq.value == 3
        assert list(out.bytes) == [0] * G.STREAMS
    finally:
        lib.fq_engine_destroy(h)


def test_validation(lib, oracle, packs):
    """Refusals come before anything is launched or copied: nothing is pending afterwards."""
    p, open_mask = params("PE_correct+all")
    pk, texts = packs("edge", True)
    h = create(lib, p, pk)
    try:
        tb = text_batch(pk, texts)
        res = pk.result_array()

        def routed(out):
            rc = lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), 1)
            assert lib.fq_engine_pending(h) == 0
            return rc
        full, keep = out_buffers(lib, pk, texts, open_mask)
        assert routed(full) == abi.FQ_E_INVALID  # no egress set
        eg = abi.FqEgress(open_mask, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        for s in (G.OUT1, G.UNPAIRED2, G.FAILED):  # one byte under the bound
            small, keep_s = out_buffers(lib, pk, texts, open_mask, shrink=s)
            assert routed(small) == abi.FQ_E_INVALID, G.STREAM_NAMES[s]
        nobuf, keep_n = out_buffers(lib, pk, texts, open_mask, drop=G.FAILED)  # an open stream without a buffer
        assert routed(nobuf) == abi.FQ_E_INVALID
        bad = abi.FqEgress(1 << G.STREAMS, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(bad)) == abi.FQ_E_INVALID
        # with the egress set the plain text-pack call refuses -c as before while the raw stream takes it
        # (for fq_engine_raw_launch_routed, tests/test_egress_raw_gpu.py); after NULL the old refusals are back
        plain = abi.FqTextOut()
        bufs = [np.zeros(texts[m][0].size + 16, np.uint8) for m in range(2)]
        for m in range(2):
            plain.text[m] = bufs[m].ctypes.data
        assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(plain), 1) == abi.FQ_E_INVALID
        assert lib.fq_engine_raw_begin(h, 1 << 20, 1 << 16) == 0
        assert lib.fq_engine_raw_end(h) == 0
        assert lib.fq_engine_set_egress(h, None) == 0
        assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(plain), 1) == abi.FQ_E_INVALID
        assert lib.fq_engine_raw_begin(h, 1 << 20, 1 << 16) == abi.FQ_E_INVALID
        assert routed(full) == abi.FQ_E_INVALID
    finally:
        lib.fq_engine_destroy(h)


def test_umi_is_still_refused(lib, oracle, packs):
    p = config("PE_umi", max_cycles=512)
    pk, texts = packs("edge", True)
    h = create(lib, p, pk)
    try:
        eg = abi.FqEgress(PAIR | FAIL, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        tb = text_batch(pk, texts)
        out, keep = out_buffers(lib, pk, texts, PAIR | FAIL)
        res = pk.result_array()
        assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), 1) == abi.FQ_E_INVALID
    finally:
        lib.fq_engine_destroy(h)


# ---- the binary ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["td_pe_correct", "td_pe_all", "td_pe_merge_discard"])
def test_fqtool_takes_the_device_route(case, tmp_path):
    """-c with --failed_out, the failed + unpaired outputs and -m --discard_unmerged: the tool's
    closing log line names the raw stream or text packs as what carried the run (these runs went
    through host packs before), and the outputs and reports are the reference's."""
    import subprocess

    import e2e_util as E
    p = subprocess.run(E.argv_for(abi.FQTOOL_BIN, case, str(tmp_path)), capture_output=True, cwd=tmp_path, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1, err[-2000:]
    assert "(raw stream" in closing[0] or "(text packs" in closing[0], closing[0]
    E.check_outputs(case, str(tmp_path))
