"""The device ingest and the pack cuts on the GPU (include/fqengine.h: fq_engine_set_index_filter,
fq_engine_set_phred64, fq_engine_set_cuts / fq_engine_next_cuts): on the synthetic pack of hostile
names, records and accumulator equal the oracle's run with the model's flags / on the host-converted
pack, the output text equals the Python model (tests/ingest_util.py, pinned to the reference by
tests/test_ingest_cpu.py) on plain and routed text packs and on the raw stream across a window seam,
and every piece of a cut table equals the model's.  Refusals leave nothing pending.  The binary takes
the device route on every index-filter, phred64 and split fixture and writes the reference's files."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import e2e_util as E
import egress_util as G
import ingest_util as I
import umi_util as U
from batch_util import config, run_oracle
from fqtool_amd import abi
from test_egress_gpu import create, text_batch
from test_egress_raw_gpu import run_raw_routed
from test_umi_egress_gpu import submit_routed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


@pytest.fixture(scope="module")
def packs():
    """(paired, raw) -> (pack, its FASTQ text per mate, its reads): built once, never changed.  raw: the
    raw stream's variant, lines ending in "\\n" only and no empty read."""
    cache = {}

    def get(paired, raw=False):
        if (paired, raw) not in cache:
            pk, texts = U.synth_pack_and_texts(paired, crlf=not raw, min_len=1 if raw else 0)
            reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
            cache[(paired, raw)] = (pk, texts, reads)
        return cache[(paired, raw)]
    return get


@pytest.fixture(scope="module")
def filtered(oracle, packs):
    """(paired, raw, list name) -> (params, the model's flags, the oracle's records and accumulator
    under them), once per key."""
    cache = {}
    lists = dict(I.SYNTH_LISTS, big=(I.big_list(), [], 0))

    def get(paired, raw, name):
        key = (paired, raw, name)
        if key not in cache:
            pk, texts, reads = packs(paired, raw)
            p = config(I.SYNTH_CFG[paired], max_cycles=512)
            flags = I.index_flags(reads, *lists[name])
            pk.flags = flags
            try:
                res, acc = run_oracle(oracle, p, pk)
            finally:
                pk.flags = None
            cache[key] = (p, lists[name], flags, res, acc)
        return cache[key]
    return get


def pair_mask(paired):
    return G.mask(G.OUT1, G.OUT2) if paired else G.mask(G.OUT1)


def check_condition(name, paired, flags):
    """A pack that is all dropped or none dropped would hide a wrong kernel."""
    count, n = int(np.count_nonzero(flags)), len(flags)
    if name in I.DEGENERATE:
        assert count == (n if I.DEGENERATE[name] == "all" else 0)
    elif name == "list2only1" and not paired:
        assert count == 0  # single end uses list 1 only
    else:
        assert 0 < count < n, (name, paired, count)


def set_filter(lib, h, lst):
    f, keep = I.fq_index_filter(*lst)
    assert lib.fq_engine_set_index_filter(h, ctypes.byref(f)) == 0, lib.fq_engine_last_error(h).decode()


def submit_text(lib, h, pk, texts, seq_no, n=None, cuts=None):
    """One plain text pack (its first n records), polled: (records, output text per mate)."""
    tb = text_batch(pk, texts)
    if n is not None:
        tb.n = n
    out, bufs = abi.FqTextOut(), []
    for m in range(len(texts)):
        bufs.append(np.zeros(texts[m][0].size + 16, np.uint8))
        out.text[m] = bufs[m].ctypes.data
    res = pk.result_array()
    if cuts is not None:
        first, table = cuts
        assert lib.fq_engine_next_cuts(h, first, table.ctypes.data, table.size) == 0, lib.fq_engine_last_error(h).decode()
    assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), seq_no) == 0, \
        lib.fq_engine_last_error(h).decode()
    seq = ctypes.c_uint64()
    assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
    assert seq.value == seq_no
    return res[:tb.n * len(texts)], [bufs[m][:out.bytes[m]].tobytes() for m in range(len(texts))]


def read_acc(lib, h):
    acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
    assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
    return acc


def run_raw_plain(lib, h, texts, max_batch, wcap, ccap=600000, cuts_every=0, first_item=0):
    """The plain raw stream over windows of wcap bytes (then empty ones that drain the carry), one pack in
    flight: per pack (pairs, output text per mate, its cut table or None, the largest carry after it)."""
    mates = len(texts)
    assert lib.fq_engine_raw_begin(h, wcap, ccap) == 0, lib.fq_engine_last_error(h).decode()
    pos, out_packs, k, taken = [0] * mates, [], 0, first_item
    while True:
        w = abi.FqRawWindow()
        for m in range(mates):
            n = min(wcap, texts[m].size - pos[m])
            w.bytes[m] = texts[m].ctypes.data + pos[m] if n else None
            w.n[m] = n
            pos[m] += n
        assert lib.fq_engine_raw_enqueue(h, ctypes.byref(w)) == 0, lib.fq_engine_last_error(h).decode()
        r, o, bufs = abi.FqRawResult(), abi.FqRawOut(), []
        for m in range(mates):
            bufs.append(np.zeros(ccap + wcap + 4 * max_batch + 64, np.uint8))
            o.text.text[m] = bufs[m].ctypes.data
        table = None
        if cuts_every:
            table = np.zeros(lib.fq_cuts_bound(cuts_every, max_batch), np.dtype(abi.CUT_DTYPE))
            assert lib.fq_engine_next_cuts(h, taken, table.ctypes.data, table.size) == 0, lib.fq_engine_last_error(h).decode()
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), k) == 0, lib.fq_engine_last_error(h).decode()
        seq = ctypes.c_uint64()
        assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
        assert seq.value == k and not r.stop
        if table is not None:
            table = table[:lib.fq_cuts_count(cuts_every, taken, max(r.pairs, 0))]
        out_packs.append((r.pairs, [bufs[m][:o.text.bytes[m]].tobytes() for m in range(mates)], table,
                          max(r.carry[m] for m in range(mates))))
        taken += max(r.pairs, 0)
        k += 1
        sent = all(pos[m] == texts[m].size for m in range(mates))
        if sent and (r.pairs == 0 or not any(r.carry[m] for m in range(mates))):
            break
    assert lib.fq_engine_raw_end(h) == 0
    return out_packs


def as_cuts(table):
    return [I.Cut(int(c["bytes"][0]), int(c["bytes"][1]), int(c["items"]), int(c["passed"])) for c in table]


# ---- 1. the index filter ------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_index_filter_on_text_packs(lib, packs, filtered, paired):
    """Every list (thresholds 0, 1 and 10, the empty lists, an empty entry, the list above 32 KiB that
    takes the non-LDS path) on one engine, detached at the end."""
    pk, texts, reads = packs(paired)
    h = None
    try:
        for k, name in enumerate(list(I.SYNTH_LISTS) + ["big"]):
            p, lst, flags, res_o, acc_o = filtered(paired, False, name)
            if name != "big":
                check_condition(name, paired, flags)
            h = h or create(lib, p, pk)
            set_filter(lib, h, lst)
            assert lib.fq_engine_reset_acc(h) == 0
            res, got = submit_text(lib, h, pk, texts, 3 + k)
            assert np.array_equal(res, res_o), name
            assert np.array_equal(read_acc(lib, h), acc_o), name
            exp = G.model(reads, res_o, paired, False, False, pair_mask(paired))
            for m in range(len(texts)):
                assert got[m] == exp[m], "%s: mate %d" % (name, m + 1)
        # detached: nothing is dropped
        assert lib.fq_engine_set_index_filter(h, None) == 0
        res, _ = submit_text(lib, h, pk, texts, 99)
        assert not (res["flags"] & abi.FQ_RF_INDEX_FILTERED).any()
    finally:
        if h:
            lib.fq_engine_destroy(h)


@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_index_filter_on_routed_text_packs(lib, packs, filtered, paired):
    """FAILED open: dropped records reach no stream."""
    pk, texts, reads = packs(paired)
    open_mask = pair_mask(paired) | G.mask(G.FAILED)
    h = None
    try:
        for k, name in enumerate(["exact0", "high1", "big"]):
            p, lst, flags, res_o, acc_o = filtered(paired, False, name)
            h = h or create(lib, p, pk)
            set_filter(lib, h, lst)
            eg = abi.FqEgress(open_mask, 0)
            assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
            res, got = submit_routed(lib, h, pk, texts, open_mask, None, 5 + k)
            assert np.array_equal(res, res_o), name
            exp = G.model(reads, res_o, paired, False, False, open_mask)
            for s in range(G.STREAMS):
                assert got[s] == exp[s], "%s: stream %s" % (name, G.STREAM_NAMES[s])
            assert exp[G.FAILED] and exp[G.OUT1]
    finally:
        if h:
            lib.fq_engine_destroy(h)


@pytest.mark.parametrize("name", ["exact0", "big"])
@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_index_filter_on_the_raw_stream(lib, packs, filtered, paired, name):
    """The first window holds about half the text, so a pair straddles the seam (the device carry)."""
    pk, texts, reads = packs(paired, raw=True)
    p, lst, flags, res_o, acc_o = filtered(paired, True, name)
    h = create(lib, p, pk)
    try:
        set_filter(lib, h, lst)
        arrs = [t[0] for t in texts]
        out = run_raw_plain(lib, h, arrs, pk.n, max(a.size for a in arrs) // 2 + 2000)
        assert sum(o[0] for o in out) == pk.n and sum(1 for o in out if o[0]) >= 2 and max(o[3] for o in out) > 0
        assert np.array_equal(read_acc(lib, h), acc_o)
        exp = G.model(reads, res_o, paired, False, False, pair_mask(paired))
        for m in range(len(texts)):
            assert b"".join(o[1][m] for o in out) == exp[m], "mate %d" % (m + 1)
    finally:
        lib.fq_engine_destroy(h)


class FilterLib:
    """The engine library as tests/test_egress_raw_gpu.py's driver calls it, with the filter attached
    wherever an egress is set."""

    def __init__(self, lib, lst):
        self._lib, (self._f, self._keep) = lib, I.fq_index_filter(*lst)

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def fq_engine_set_egress(self, h, eg):
        rc = self._lib.fq_engine_set_egress(h, eg)
        if rc == 0 and eg is not None:
            rc = self._lib.fq_engine_set_index_filter(h, ctypes.byref(self._f))
        return rc


@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_index_filter_on_the_routed_raw_stream(lib, packs, filtered, paired):
    pk, texts, reads = packs(paired, raw=True)
    p, lst, flags, res_o, acc_o = filtered(paired, True, "high1")
    open_mask = pair_mask(paired) | G.mask(G.FAILED)
    arrs = [t[0] for t in texts]
    packs_n, got, ads, acc, carry_max = run_raw_routed(FilterLib(lib, lst), p, arrs, open_mask, 4096, pk.stride, random.Random(11),
                                                       wcap=max(a.size for a in arrs) // 2 + 2000)
    assert sum(packs_n) == pk.n and sum(1 for n in packs_n if n) >= 2 and carry_max > 0
    assert np.array_equal(acc, acc_o)
    exp = G.model(reads, res_o, paired, False, False, open_mask)
    for s in range(G.STREAMS):
        assert got[s] == exp[s], "stream %s differs" % G.STREAM_NAMES[s]


# ---- 2. --phred64 -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def phred(oracle):
    """(paired, raw) -> (the pack as the input holds it, its texts, params, the oracle's records and
    accumulator on the host-converted pack, the model's output text)."""
    cache = {}

    def get(paired, raw):
        if (paired, raw) not in cache:
            src, texts, conv = I.phred64_pack(paired, raw)
            p = config(I.SYNTH_CFG[paired], max_cycles=512)
            res, acc = run_oracle(oracle, p, conv)
            reads = [G.reads_of_pack(conv, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
            exp = G.model(reads, res, paired, False, False, pair_mask(paired))
            assert exp[G.OUT1]
            # (the conversion matters: the unconverted pack gives other records)
            assert not np.array_equal(run_oracle(oracle, p, src)[0], res)
            cache[(paired, raw)] = (src, texts, p, res, acc, exp)
        return cache[(paired, raw)]
    return get


@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_phred64_on_text_packs(lib, phred, paired):
    src, texts, p, res_o, acc_o, exp = phred(paired, False)
    h = create(lib, p, src)
    try:
        assert lib.fq_engine_set_phred64(h, 1) == 0, lib.fq_engine_last_error(h).decode()
        before = [t[0].copy() for t in texts]
        res, got = submit_text(lib, h, src, texts, 4)
        assert np.array_equal(res, res_o)
        assert np.array_equal(read_acc(lib, h), acc_o)
        for m in range(len(texts)):
            assert got[m] == exp[m], "mate %d" % (m + 1)
            assert np.array_equal(texts[m][0], before[m])  # (the caller's text is not touched)
        # off again: the records of the unconverted pack
        assert lib.fq_engine_set_phred64(h, 0) == 0
        res, _ = submit_text(lib, h, src, texts, 5)
        assert not np.array_equal(res, res_o)
    finally:
        lib.fq_engine_destroy(h)


@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_phred64_on_the_raw_stream(lib, phred, paired):
    """Across a seam: the carry's records come out converted exactly once (a second conversion would
    move every quality down again, and the text would differ)."""
    src, texts, p, res_o, acc_o, exp = phred(paired, True)
    h = create(lib, p, src)
    try:
        assert lib.fq_engine_set_phred64(h, 1) == 0, lib.fq_engine_last_error(h).decode()
        arrs = [t[0] for t in texts]
        out = run_raw_plain(lib, h, arrs, src.n, max(a.size for a in arrs) // 2 + 2000)
        assert sum(o[0] for o in out) == src.n and sum(1 for o in out if o[0]) >= 2 and max(o[3] for o in out) > 0
        assert np.array_equal(read_acc(lib, h), acc_o)
        for m in range(len(texts)):
            assert b"".join(o[1][m] for o in out) == exp[m], "mate %d" % (m + 1)
    finally:
        lib.fq_engine_destroy(h)


# ---- 3. pack cuts -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain(oracle, packs):
    """(paired, raw) -> (params, the oracle's records, the model's per-record output sizes and streams)."""
    cache = {}

    def get(paired, raw):
        if (paired, raw) not in cache:
            pk, texts, reads = packs(paired, raw)
            p = config(I.SYNTH_CFG[paired], max_cycles=512)
            res, _ = run_oracle(oracle, p, pk)
            sizes = I.out_sizes(reads, res)
            exp = G.model(reads, res, paired, False, False, pair_mask(paired))
            assert 0 < np.count_nonzero(sizes[0]) < pk.n and [int(z.sum()) for z in sizes] == [len(exp[m]) for m in range(len(texts))]
            cache[(paired, raw)] = (p, res, sizes, exp)
        return cache[(paired, raw)]
    return get


def check_pieces(table, want, got_text, mates):
    """Every piece equals the model's, and the pieces re-assemble to the uncut streams."""
    assert as_cuts(table) == want
    for m in range(mates):
        assert sum((c.bytes0, c.bytes1)[m] for c in want) == len(got_text[m])
    if mates == 1:
        assert all(c.bytes1 == 0 for c in want)


@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_cuts_on_text_packs(lib, packs, plain, paired):
    pk, texts, reads = packs(paired)
    p, res_o, sizes, exp = plain(paired, False)
    mates = len(texts)
    h = create(lib, p, pk)
    try:
        k = 0
        for every in (1, 7, pk.n, pk.n + 1):
            assert lib.fq_engine_set_cuts(h, every) == 0, lib.fq_engine_last_error(h).decode()
            for first in (0, 5):
                table = np.zeros(lib.fq_cuts_bound(every, pk.n), np.dtype(abi.CUT_DTYPE))
                res, got = submit_text(lib, h, pk, texts, 10 + k, cuts=(first, table))
                k += 1
                assert np.array_equal(res, res_o)
                assert got == [exp[m] for m in range(mates)]
                want = I.cut_table(sizes, every, first)
                assert len(want) == lib.fq_cuts_count(every, first, pk.n) <= table.size
                check_pieces(table[:len(want)], want, got, mates)
                if every == 7 and first == 5:
                    assert want[0].items == 2  # (the first piece is short)
        # a pack whose last piece is empty of passing records: it ends with a record that writes nothing,
        # which a cut falls right in front of
        i0 = int(np.flatnonzero(sizes[0] == 0)[-1])
        first = (7 - i0 % 7) % 7
        assert lib.fq_engine_set_cuts(h, 7) == 0
        table = np.zeros(lib.fq_cuts_bound(7, i0 + 1), np.dtype(abi.CUT_DTYPE))
        res, got = submit_text(lib, h, pk, texts, 40, n=i0 + 1, cuts=(first, table))
        want = I.cut_table([z[:i0 + 1] for z in sizes], 7, first)
        assert want[-1] == I.Cut(0, 0, 1, 0)
        check_pieces(table[:len(want)], want, got, mates)
        # a pack without fq_engine_next_cuts gets no table, and cuts go off again
        res, got = submit_text(lib, h, pk, texts, 41)
        assert got == [exp[m] for m in range(mates)]
        assert lib.fq_engine_set_cuts(h, 0) == 0
        assert lib.fq_engine_next_cuts(h, 0, table.ctypes.data, table.size) == abi.FQ_E_INVALID
    finally:
        lib.fq_engine_destroy(h)


@pytest.mark.parametrize("every,first", [(1, 0), (7, 5), (700, 0), (701, 5)])
@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_cuts_on_the_raw_stream(lib, packs, plain, paired, every, first):
    """Two windows: the second pack's first_item is the first pack's pairs past the stream's."""
    pk, texts, reads = packs(paired, raw=True)
    assert pk.n == 700
    p, res_o, sizes, exp = plain(paired, True)
    mates = len(texts)
    h = create(lib, p, pk)
    try:
        assert lib.fq_engine_set_cuts(h, every) == 0, lib.fq_engine_last_error(h).decode()
        arrs = [t[0] for t in texts]
        out = run_raw_plain(lib, h, arrs, pk.n, max(a.size for a in arrs) // 2 + 2000, cuts_every=every, first_item=first)
        assert sum(o[0] for o in out) == pk.n and sum(1 for o in out if o[0]) >= 2
        at = 0
        for pairs, text, table, _ in out:
            want = I.cut_table([z[at:at + pairs] for z in sizes], every, first + at)
            check_pieces(table, want, text, mates)
            at += pairs
        for m in range(mates):
            assert b"".join(o[1][m] for o in out) == exp[m]
    finally:
        lib.fq_engine_destroy(h)


# ---- 4. refusals --------------------------------------------------------------------------------------
def test_refusals(lib, packs, plain):
    """No kernel is launched for a refused call: nothing is pending afterwards."""
    pk, texts, reads = packs(True)
    p, res_o, sizes, exp = plain(True, False)
    h = create(lib, p, pk)
    try:
        tb = text_batch(pk, texts)
        res = pk.result_array()
        out, bufs = abi.FqTextOut(), [np.zeros(texts[m][0].size + 16, np.uint8) for m in range(2)]
        for m in range(2):
            out.text[m] = bufs[m].ctypes.data
        # the filter's description
        for bad in (([b"AC"], [], -1),):
            f, keep = I.fq_index_filter(*bad)
            assert lib.fq_engine_set_index_filter(h, ctypes.byref(f)) == abi.FQ_E_INVALID
        f, keep = I.fq_index_filter([b"A" * 65536], [], 0)
        assert lib.fq_engine_set_index_filter(h, ctypes.byref(f)) == abi.FQ_E_INVALID
        f, keep = I.fq_index_filter([b"A" * 65535], [], 0)
        assert lib.fq_engine_set_index_filter(h, ctypes.byref(f)) == 0
        assert lib.fq_engine_set_index_filter(h, None) == 0
        assert lib.fq_engine_set_phred64(h, 2) == abi.FQ_E_INVALID
        # a table one below the bound
        assert lib.fq_engine_set_cuts(h, 7) == 0
        need = lib.fq_cuts_bound(7, pk.n)
        assert need == pk.n // 7 + 2
        table = np.zeros(need, np.dtype(abi.CUT_DTYPE))
        assert lib.fq_engine_next_cuts(h, 5, table.ctypes.data, need - 1) == 0
        assert lib.fq_engine_submit_text(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(out), 1) == abi.FQ_E_INVALID
        assert lib.fq_engine_pending(h) == 0
        # cuts on a routed call (the table stays armed until a plain pack takes it)
        eg = abi.FqEgress(pair_mask(True), 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0
        assert lib.fq_engine_next_cuts(h, 5, table.ctypes.data, need) == 0
        routed, keep = abi.FqEgressOut(), []
        for s in (G.OUT1, G.OUT2):
            cap = lib.fq_egress_bound(s, texts[0][0].size, texts[1][0].size, pk.n)
            keep.append(np.zeros(cap, np.uint8))
            routed.text[s], routed.cap[s] = keep[-1].ctypes.data, cap
        assert lib.fq_engine_submit_text_routed(h, ctypes.byref(tb), res.ctypes.data, ctypes.byref(routed), 1) == abi.FQ_E_INVALID
        assert b"pack cuts" in lib.fq_engine_last_error(h)
        assert lib.fq_engine_pending(h) == 0
        assert lib.fq_engine_set_egress(h, None) == 0
        # device BGZF and cuts exclude each other
        assert lib.fq_engine_set_gz_out(h, 4) == abi.FQ_E_INVALID
        # the setters inside a raw stream; a small table leaves the window enqueued
        assert lib.fq_engine_raw_begin(h, 1 << 20, 1 << 16) == 0, lib.fq_engine_last_error(h).decode()
        f, keep = I.fq_index_filter([b"AC"], [], 0)
        assert lib.fq_engine_set_index_filter(h, ctypes.byref(f)) == abi.FQ_E_INVALID
        assert lib.fq_engine_set_index_filter(h, None) == abi.FQ_E_INVALID
        assert lib.fq_engine_set_phred64(h, 1) == abi.FQ_E_INVALID
        assert lib.fq_engine_set_cuts(h, 0) == abi.FQ_E_INVALID
        assert lib.fq_engine_raw_end(h) == 0
        assert lib.fq_engine_pending(h) == 0
        # the armed pack still goes through
        got_res, got = submit_text(lib, h, pk, texts, 9)
        assert np.array_equal(got_res, res_o) and got == [exp[0], exp[1]]
        assert as_cuts(table[:lib.fq_cuts_count(7, 5, pk.n)]) == I.cut_table(sizes, 7, 5)
    finally:
        lib.fq_engine_destroy(h)
    # cuts with -m
    pm = config("C4", max_cycles=512)
    h = create(lib, pm, pk)
    try:
        assert lib.fq_engine_set_cuts(h, 7) == abi.FQ_E_INVALID
        assert lib.fq_engine_set_cuts(h, 0) == 0
    finally:
        lib.fq_engine_destroy(h)


def test_raw_refusals(lib, packs, plain):
    """A table below the bound is refused before the launch and leaves the window enqueued; the
    records-only egress takes neither cuts nor --phred64."""
    pk, texts, reads = packs(True, raw=True)
    p, res_o, sizes, exp = plain(True, True)
    h = create(lib, p, pk)
    try:
        assert lib.fq_engine_set_cuts(h, 7) == 0
        assert lib.fq_engine_set_phred64(h, 1) == 0
        wcap = max(t[0].size for t in texts) + 16
        assert lib.fq_engine_raw_begin(h, wcap, 1 << 16) == 0, lib.fq_engine_last_error(h).decode()
        w = abi.FqRawWindow()
        for m in range(2):
            w.bytes[m], w.n[m] = texts[m][0].ctypes.data, texts[m][0].size
        assert lib.fq_engine_raw_enqueue(h, ctypes.byref(w)) == 0
        r, o = abi.FqRawResult(), abi.FqRawOut()
        bufs = [np.zeros((1 << 16) + wcap + 4 * pk.n + 64, np.uint8) for _ in range(2)]
        for m in range(2):
            o.text.text[m] = bufs[m].ctypes.data
        need = lib.fq_cuts_bound(7, pk.n)
        table = np.zeros(need, np.dtype(abi.CUT_DTYPE))
        assert lib.fq_engine_next_cuts(h, 0, table.ctypes.data, need - 1) == 0
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), 0) == abi.FQ_E_INVALID
        assert lib.fq_engine_pending(h) == 0
        recs = abi.FqRawOut()
        rr = pk.result_array()
        trec = [np.zeros(pk.n, np.dtype(abi.TEXT_REC_DTYPE)) for _ in range(2)]
        recs.results = rr.ctypes.data
        for m in range(2):
            recs.rec[m] = trec[m].ctypes.data
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(recs), 0) == abi.FQ_E_INVALID
        assert lib.fq_engine_pending(h) == 0
        # the window is still there: the launch with a table of the bound takes it
        assert lib.fq_engine_next_cuts(h, 0, table.ctypes.data, need) == 0
        assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), 0) == 0, lib.fq_engine_last_error(h).decode()
        seq = ctypes.c_uint64()
        assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
        assert r.pairs == pk.n
        assert sum(int(c["items"]) for c in table[:lib.fq_cuts_count(7, 0, pk.n)]) == pk.n
        assert lib.fq_engine_raw_end(h) == 0
    finally:
        lib.fq_engine_destroy(h)


# ---- 5. the binary ------------------------------------------------------------------------------------
def run_tool(case, outdir, extra=(), env=None, workers="1"):
    argv = E.argv_for(abi.FQTOOL_BIN, case, str(outdir))
    argv[argv.index("-w") + 1] = workers
    p = subprocess.run(argv + list(extra), capture_output=True, cwd=outdir, timeout=300, env=dict(os.environ, **(env or {})))
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1, err[-2000:]
    return closing[0]


def suffix_of(case):
    return ("; index filter on the device" if case in I.INDEX_CASES else
            "; phred64 on the device" if case in I.PHRED64_CASES else " pack cuts")


@pytest.mark.parametrize("case", I.INDEX_CASES + I.PHRED64_CASES + I.SPLIT_CASES)
def test_fqtool_takes_the_device_route(case, tmp_path):
    """The closing log line names the raw stream or text packs plus what the device did besides (these
    runs went through host packs before), and the outputs and reports are the reference's."""
    closing = run_tool(case, tmp_path)
    assert "(raw stream" in closing or "(text packs" in closing, closing
    assert suffix_of(case) in closing, closing
    if case in I.SPLIT_CASES:
        assert "; 0 pack cuts" not in closing and "routed egress" not in closing, closing
    E.check_outputs(case, str(tmp_path))


@pytest.mark.parametrize("case", ["td_pe_split_num", "td_pe_index"])
def test_fqtool_text_packs_on_two_engines(case, tmp_path):
    """Two engines share the run out as text packs of 777 pairs (a split run's cuts count from each
    pack's first global record, which the reader hands the engines)."""
    closing = run_tool(case, tmp_path, ["--devices", "0,0", "--pack_pairs", "777"])
    assert "(text packs" in closing and suffix_of(case) in closing, closing
    E.check_outputs(case, str(tmp_path))


def test_fqtool_split_with_three_workers(tmp_path):
    """-w 3 deals the reference packs over three file sequences; the reference is deterministic at
    -w 1 only, so the device route is compared with the same binary's host packs (FQ_TEXT_MODE=0)."""
    case = "td_se_split_num_many"
    dev, hostd = tmp_path / "dev", tmp_path / "host"
    dev.mkdir()
    hostd.mkdir()
    closing = run_tool(case, dev, workers="3")
    assert ("(raw stream" in closing or "(text packs" in closing) and " pack cuts" in closing, closing
    closing = run_tool(case, hostd, workers="3", env={"FQ_TEXT_MODE": "0"})
    assert "(raw stream" not in closing and "(text packs" not in closing, closing
    names = sorted(n for n in os.listdir(dev) if not n.startswith("report."))
    assert names == sorted(n for n in os.listdir(hostd) if not n.startswith("report.")) and len(names) >= 9
    for n in names:
        assert E.digest(str(dev / n)) == E.digest(str(hostd / n)), n
