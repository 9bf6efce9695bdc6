"""k-mer statistics on the GPU (fq_kstat_*, fqtool_amd/csrc/kstat.hip) against the numpy model of the
reference's counting (tests/kmer_util.py, pinned to the reference's reports by tests/test_kstat_cpu.py).

Bit-exact: the four tables [pre-R1 | pre-R2 | post-R1 | post-R2] must equal the model's.  The post
tables' expectation comes from the ORACLE's records of the same pack, never from the engine's own."""
import ctypes
import random

import numpy as np
import pytest

import kmer_util as K
from batch_util import Pack, config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi

pytestmark = pytest.mark.gpu

BELOW, ABOVE = K.LDS_MAX_K, K.LDS_MAX_K + 1  # last k on the LDS path, first k on the global-atomics path


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


def make_kstat(lib, k):
    h = ctypes.c_void_p()
    assert lib.fq_kstat_create(0, k, ctypes.byref(h)) == 0
    return h


def read_tables(lib, ks):
    t = np.zeros(lib.fq_kstat_words(ks), np.uint64)
    assert lib.fq_kstat_read(ks, t.ctypes.data, t.size) == 0
    return t


def make_engine(lib, p, packs):
    h = ctypes.c_void_p()
    rc = lib.fq_engine_create(ctypes.byref(p), 0, max(max(pk.n for pk in packs), 1), max(pk.stride for pk in packs),
                              ctypes.byref(h))
    assert rc == 0, lib.fq_engine_last_error(None)
    return h


def run_pack(lib, h, pk, entry="process", seq_no=0, merge=False):
    """One pack through an entry point; returns its records."""
    res = pk.result_array()
    if entry == "process":
        assert lib.fq_engine_process(h, ctypes.byref(pk.batch()), res.ctypes.data) == 0, lib.fq_engine_last_error(h)
    elif entry == "submit":
        assert lib.fq_engine_submit(h, ctypes.byref(pk.batch()), res.ctypes.data, seq_no) == 0, lib.fq_engine_last_error(h)
        assert lib.fq_engine_poll(h, 1, None) == 1, lib.fq_engine_last_error(h)
    elif entry in ("device", "device_norecords"):
        import torch
        hb = pk.batch()
        dev = torch.device("cuda:0")
        keep = {k: torch.from_numpy(v).to(dev) for k, v in pk._tiled.items()}
        lens = [torch.from_numpy(pk.len1.view(np.int16)).to(dev)]
        if pk.paired:
            lens.append(torch.from_numpy(pk.len2.view(np.int16)).to(dev))
        res_d = torch.zeros(res.size * 16, dtype=torch.uint8, device=dev)
        b = abi.FqBatch()
        b.n, b.stride = hb.n, hb.stride
        b.seq1, b.qual1, b.len1 = keep["seq1"].data_ptr(), keep["qual1"].data_ptr(), lens[0].data_ptr()
        if pk.paired:
            b.seq2, b.qual2, b.len2 = keep["seq2"].data_ptr(), keep["qual2"].data_ptr(), lens[1].data_ptr()
        if pk.flags is not None:
            flags = torch.from_numpy(pk.flags).to(dev)
            b.flags = flags.data_ptr()
        torch.cuda.synchronize()
        out = res_d.data_ptr() if entry == "device" else None
        assert lib.fq_engine_process_device(h, ctypes.byref(b), out, None) == 0, lib.fq_engine_last_error(h)
        assert lib.fq_engine_sync(h) == 0, lib.fq_engine_last_error(h)
        res = res_d.cpu().numpy().view(res.dtype) if entry == "device" else None
    elif entry == "text":
        from test_text_gpu import fastq_text
        rng = random.Random(5)
        tb, out, bufs = abi.FqTextBatch(), abi.FqTextOut(), []
        tb.n, tb.stride = pk.n, pk.stride
        texts = [fastq_text(pk, m + 1, rng)[:2] for m in range(2 if pk.paired else 1)]
        for m, (text, recs) in enumerate(texts):
            # (-m: mate 0's buffer takes the merged stream, include/fqengine.h fq_engine_submit_text)
            cap = sum(t.size for t, _ in texts) + 24 * pk.n + 16 if merge and m == 0 else text.size + 16
            ob = np.zeros(cap, np.uint8)
            bufs.append((text, recs, ob))
            tb.text[m], tb.text_bytes[m], tb.rec[m], out.text[m] = text.ctypes.data, text.size, recs.ctypes.data, ob.ctypes.data
        assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), seq_no) == 0, \
            lib.fq_engine_last_error(h)
        assert lib.fq_engine_poll(h, 1, None) == 1, lib.fq_engine_last_error(h)
    else:
        raise KeyError(entry)
    return res


def engine_tables(lib, p, packs, k, entry="process", n_tables=1):
    """Packs dealt round-robin over n_tables engines, each with its own tables; the tables summed."""
    engines, kstats = [], []
    try:
        for _ in range(n_tables):
            engines.append(make_engine(lib, p, packs))
            kstats.append(make_kstat(lib, k))
            assert lib.fq_engine_set_kstat(engines[-1], kstats[-1]) == 0
        for i, pk in enumerate(packs):
            run_pack(lib, engines[i % n_tables], pk, entry, i, merge=bool(p.merge_enabled))
        return sum(read_tables(lib, ks) for ks in kstats)
    finally:
        for h in engines:
            lib.fq_engine_destroy(h)
        for ks in kstats:
            lib.fq_kstat_destroy(ks)


def model_tables(oracle, p, packs, k):
    t = K.Tables(k)
    for pk in packs:
        res, _ = run_oracle(oracle, p, pk)
        K.model_pack(pk, p, res, k, t)
    return t.array()


def check(want, got):
    if not np.array_equal(want, got):
        bad = np.nonzero(want != got)[0]
        size = want.size // 4
        raise AssertionError("%d counters differ; first: table %d key %d: model %d engine %d" % (
            len(bad), bad[0] // size, bad[0] % size, want[bad[0]], got[bad[0]]))


def test_create_limits(lib):
    h = ctypes.c_void_p()
    for k in (0, K.MIN_K - 1, K.MAX_K + 1, 16):
        assert lib.fq_kstat_create(0, k, ctypes.byref(h)) == abi.FQ_E_INVALID
    ks = make_kstat(lib, 6)
    try:
        assert lib.fq_kstat_k(ks) == 6 and lib.fq_kstat_words(ks) == 4 * 4 ** 6
        assert not read_tables(lib, ks).any()
        small = np.zeros(16, np.uint64)
        assert lib.fq_kstat_read(ks, small.ctypes.data, small.size) == abi.FQ_E_INVALID
    finally:
        lib.fq_kstat_destroy(ks)


@pytest.mark.parametrize("k", [4, 5, BELOW, ABOVE])
@pytest.mark.parametrize("paired", [True, False])
def test_lengths_and_bad_bytes(lib, oracle, k, paired):
    """Reads of length 0 .. k + 1 and around the chunk boundaries; an N, a lower-case and an IUPAC
    byte at every position of a 2k-long read."""
    p = config("C3" if paired else "C2", max_cycles=256)
    pk = K.length_pack(k, paired)
    want = model_tables(oracle, p, [pk], k)
    assert want.reshape(4, -1)[0].sum() > 0 and want.reshape(4, -1)[2].sum() > 0
    check(want, engine_tables(lib, p, [pk], k))


def test_largest_k(lib, oracle):
    """FQ_KSTAT_MAX_K once: 4 tables of 4^12 counters."""
    p = config("C3", max_cycles=256)
    pk = K.length_pack(K.MAX_K, True)
    check(model_tables(oracle, p, [pk], K.MAX_K), engine_tables(lib, p, [pk], K.MAX_K))


@pytest.mark.parametrize("k", [5, BELOW, ABOVE])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 3001])
def test_pack_sizes(lib, oracle, n, k):
    """Part of a tile, one tile, several tiles, several workgroups."""
    p = config("C3", max_cycles=256)
    pk = edge_pack(n, True, seed=n)
    check(model_tables(oracle, p, [pk], k), engine_tables(lib, p, [pk], k))


@pytest.mark.parametrize("k", [5, BELOW, ABOVE])
def test_contention_on_one_bin(lib, oracle, k):
    """2048 reads of 150 A: every increment of a table lands in bin 0."""
    p = config("C2", max_cycles=256)
    pk = Pack(2048, 160, False)
    for i in range(pk.n):
        pk.set(i, 1, b"A" * 150, b"I" * 150)
    want = model_tables(oracle, p, [pk], k)
    assert want[0] == 2048 * (150 - k + 1) and want.sum() == 2 * want[0]
    check(want, engine_tables(lib, p, [pk], k))


VARIANTS = [("C2", 160), ("SE_all", 320), ("SE_umi", 160), ("C3", 160), ("C5", 320), ("PE_all", 160), ("C4", 160),
            ("C4", 320), ("PE_merge_discard", 160), ("PE_merge_q", 160), ("PE_umi", 160), ("PE_umi_merge", 160),
            ("PE_correct", 160), ("PE_correct_umi_merge", 160), ("PE_correct_all", 320)]


@pytest.mark.parametrize("name,stride", VARIANTS)
def test_pack_variants(lib, oracle, name, stride):
    """SE, PE, -m (merged / unmerged / discarded), UMI front trims, -c (the post pass reads the
    corrected planes, the pre pass the original ones), index-filtered pairs, both row strides."""
    p = config(name, max_cycles=1024)
    paired = bool(p.paired)
    packs = [edge_pack(2500, paired, stride=stride, seed=3), synth_pack(oracle, 1500, paired, first=77, stride=stride)]
    for pk in packs:
        pk.flags = (np.random.default_rng(2).random(pk.n) < 0.1).astype(np.uint8) * abi.FQ_BF_INDEX_FILTERED
    want = model_tables(oracle, p, packs, 6)
    assert want.reshape(4, -1)[0].sum() > 0
    check(want, engine_tables(lib, p, packs, 6))


def test_merged_junction(lib, oracle):
    """Merged reads whose windows over the junction hold an N that the complement produced."""
    p = config("C4", max_cycles=512)
    pk = K.junction_pack()
    res, _ = run_oracle(oracle, p, pk)
    merged = (res["flags"][0::2] & abi.FQ_RF_MERGED) != 0
    assert merged.sum() > pk.n // 2 and (res["m_len2"][0::2][merged] > 0).all()
    for k in (6, ABOVE):
        check(model_tables(oracle, p, [pk], k), engine_tables(lib, p, [pk], k))


@pytest.mark.parametrize("entry", ["submit", "device", "device_norecords", "text"])
@pytest.mark.parametrize("name", ["C3", "C2", "C4"])
def test_entry_points(lib, oracle, entry, name):
    """Every way into the engine passes through the same launch: asynchronous host packs, device
    batches (with and without a record buffer of the caller's) and FASTQ-text packs."""
    p = config(name, max_cycles=512)
    packs = [edge_pack(1200, bool(p.paired), seed=21), synth_pack(oracle, 900, bool(p.paired), first=5)]
    check(model_tables(oracle, p, packs, 5), engine_tables(lib, p, packs, 5, entry=entry))


def test_object_behaviour(lib, oracle):
    """Several packs accumulate; two engines with two tables fed alternate packs sum to the same;
    reset clears; a detached table stops counting."""
    p = config("C3", max_cycles=256)
    packs = [synth_pack(oracle, 1000 + 100 * i, True, first=3000 * i) for i in range(4)]
    want = model_tables(oracle, p, packs, 5)
    check(want, engine_tables(lib, p, packs, 5))
    check(want, engine_tables(lib, p, packs, 5, n_tables=2))
    h, ks = make_engine(lib, p, packs), make_kstat(lib, 5)
    try:
        assert lib.fq_engine_set_kstat(h, ks) == 0
        run_pack(lib, h, packs[0])
        first = read_tables(lib, ks)
        check(model_tables(oracle, p, packs[:1], 5), first)
        assert lib.fq_kstat_last_kernel_ms(ks) > 0
        assert lib.fq_kstat_reset(ks) == 0
        assert not read_tables(lib, ks).any()
        run_pack(lib, h, packs[0])
        check(first, read_tables(lib, ks))
        assert lib.fq_engine_set_kstat(h, None) == 0
        run_pack(lib, h, packs[1])
        check(first, read_tables(lib, ks))
    finally:
        lib.fq_engine_destroy(h)
        lib.fq_kstat_destroy(ks)


@pytest.mark.parametrize("name", ["C3", "PE_correct_umi_merge", "SE_all"])
def test_no_side_effect(lib, oracle, name):
    """The same pack with and without tables attached: identical records and accumulator (the
    oracle's)."""
    p = config(name, max_cycles=512)
    pk = edge_pack(2000, bool(p.paired), seed=9)
    res_o, acc_o = run_oracle(oracle, p, pk)
    for attach in (False, True):
        h, ks = make_engine(lib, p, [pk]), make_kstat(lib, ABOVE)
        try:
            if attach:
                assert lib.fq_engine_set_kstat(h, ks) == 0
            res = run_pack(lib, h, pk)
            acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
            assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
            assert np.array_equal(res, res_o) and np.array_equal(acc, acc_o), attach
            assert read_tables(lib, ks).any() == attach
        finally:
            lib.fq_engine_destroy(h)
            lib.fq_kstat_destroy(ks)
