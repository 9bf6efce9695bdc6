"""The fast kernels' polyG tail scan (polyg_bits, fqtool_amd/csrc/pe_fast.hip) against the CPU
restatement: records and the whole accumulator, word for word.

The scan walks a read's tail in groups of 16 scan indices taken from a stream of column words (read 2's
column in column order, read 1's downwards and bit-reversed), and decides a group's non-G bases from
the allowance at the group's two ends and one position mask per allowance step inside it
(tests/test_polyg_model_cpu.py restates the rule).  The packs here put G tails of every length on
either mate, non-G bases around the allowance steps and the group seams, N and lowercase bytes in the
tail, and very short reads; the configs with cut_right end the window ahead of the row end (a
low-quality stretch behind the tail).  Every pack is a few thousand pairs built on the CPU, and the
builder's own restatement of the reference loop (src/polyx.cpp:14-38) says how many reads and bases
the oracle must count as polyG-trimmed.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from fqtool_amd import abi
from batch_util import Pack, config

pytestmark = pytest.mark.gpu

# (compare_req, max_mismatch, one_mismatch_per); the last: per > 256, the scan's division path
PARAM_SETS = [(1, 10, 10), (10, 1, 10), (10, 5, 8), (5, 0, 8), (1, 3, 1), (20, 10, 300)]
SEAMS = [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
SHORT = [0, 1, 2, 15, 16, 17, 31, 32, 33]


@pytest.fixture(scope="module")
def eng_lib():
    return abi.load_engine()


def ref_polyg(seq, compare_req, max_mm, per):
    """PolyX::trimPolyG on one read: (new length, bases counted or None)."""
    rlen, mismatch, first_g, i = len(seq), 0, len(seq) - 1, 0
    while i < rlen:
        if seq[rlen - i - 1] != ord("G"):
            mismatch += 1
        else:
            first_g = rlen - i - 1
        if mismatch > min(max_mm, max(1, (i + 1) // per)):
            break
        i += 1
    if i + 1 >= compare_req:
        return (first_g if first_g >= 0 else rlen), rlen - first_g
    return rlen, None


def ref_cut_right(qual, w, q):
    """Filter::trimAndCut with cut_right as its only option (src/filter.cpp:124-152, 183): the kept
    length, or None for a read that comes back NULL."""
    l = len(qual)
    if l - w <= 0:
        return None
    rlen, s, found = l, 0, False
    while s + w < l:
        if sum(qual[s:s + w]) / w < 33 + q:
            found = True
            break
        s += 1
    if found:
        while s < l - 1 and qual[s] >= 33 + q:
            s += 1
        rlen = s
    return None if rlen <= 0 or l <= 1 else rlen


def non_g(rng):
    return rng.choice(b"ACT")


def tail_read(rng, L, T, planted=(), byte=None):
    """L bases ending in a tail of T: G except at the scan indices `planted` (index 0 = the last
    base), which get another base or `byte`; the base ahead of the tail is not a G."""
    seq = bytearray(rng.choice(b"ACGT") for _ in range(L))
    for i in range(T):
        seq[L - 1 - i] = ord("G")
    if T < L:
        seq[L - 1 - T] = non_g(rng)
    for i in planted:
        if i < L:
            seq[L - 1 - i] = byte if byte is not None else non_g(rng)
    return bytes(seq)


def plain(rng, L):
    s = bytearray(rng.choice(b"ACGT") for _ in range(L))
    if L:
        s[-1] = non_g(rng)
    return bytes(s)


@functools.lru_cache(maxsize=None)
def build_rows(L, per, seed):
    """(read 1, read 2, low-quality suffix lengths) rows."""
    rng = random.Random(seed)
    rows = []
    # a tail of every length on read 1 only, read 2 only, and both
    for T in range(L + 1):
        rows.append((tail_read(rng, L, T), plain(rng, L)))
        rows.append((plain(rng, L), tail_read(rng, L, T)))
        rows.append((tail_read(rng, L, T), tail_read(rng, L, rng.choice([T, rng.randrange(L + 1)]))))
    # 1 .. 12 non-G bases at scan indices around the allowance steps and the group seams
    steps = sorted({k * per + d for k in range(1, 13) for d in (-1, 0, 1) if 0 <= k * per + d < L - 1})
    spots = sorted(set(steps) | set(SEAMS)) or SEAMS
    for cnt in range(1, 13):
        for rep in range(24):
            pool = spots if rep % 3 else sorted(set(spots) | set(range(0, 70)))
            idx = rng.sample(pool, min(cnt, len(pool)))
            T = min(L, max(idx) + rng.choice([1, 2, 5, 17, 40]))
            rd = tail_read(rng, L, T, planted=idx)
            rows.append((rd, plain(rng, L)) if rep % 2 else (plain(rng, L), rd))
    # odd bytes inside the tail: N, lowercase g, another lowercase letter
    for byte in b"Ngac":
        for rep in range(24):
            T = rng.randrange(12, 80)
            idx = rng.sample(range(T), rng.choice([1, 1, 2, 3]))
            rd = tail_read(rng, L, T, planted=idx, byte=byte)
            rows.append((rd, plain(rng, L)) if rep % 2 else (plain(rng, L), rd))
    # very short reads: all G, all G but one base, random; against a short or a full-length mate
    for n in SHORT:
        for m in SHORT + [L]:
            for kind in range(3):
                a = b"G" * n if kind == 0 else tail_read(rng, n, n, planted=[rng.randrange(n)] if n else []) if kind == 1 \
                    else bytes(rng.choice(b"ACGT") for _ in range(n))
                b = tail_read(rng, m, rng.randrange(m + 1))
                rows.append((a, b) if kind != 1 else (b, a))
    rng.shuffle(rows)
    return rows


@functools.lru_cache(maxsize=None)
def build_pack(L, stride, per, lowq, paired):
    """The rows as a pack.  lowq: every other read longer than 40 gives its last 5 .. 24 bases a quality
    of 2, so cut_right ends the window there, and a G tail is moved to end just ahead of them."""
    rows = build_rows(L, per, seed=L * 1000 + per)
    rng = random.Random(L + per + lowq)
    pk = Pack(len(rows), stride, paired)
    for i, pair in enumerate(rows):
        for m in ((1, 2) if paired else (1,)):
            seq = pair[m - 1]
            qual = bytearray(33 + rng.randint(30, 40) for _ in seq)
            if lowq and len(seq) > 40 and rng.random() < 0.5:
                k = rng.randrange(5, 25)
                seq = seq[k:] + bytes(rng.choice(b"ACGT") for _ in range(k))
                qual[len(seq) - k:] = bytes([33 + 2]) * k
            pk.set(i, m, seq, bytes(qual))
    return pk


def expected_counts(p, pk):
    """polyG-trimmed reads and bases by the reference loop on each read's window (polyG runs only on
    pairs whose two reads both survive trimAndCut, src/peprocessor.cpp:283-299)."""
    reads = bases = 0
    for i in range(pk.n):
        wins = []
        for m in ((1, 2) if pk.paired else (1,)):
            n = int(getattr(pk, "len%d" % m)[i])
            seq = bytes(getattr(pk, "seq%d" % m)[i, :n])
            if p.cut_right:
                n = ref_cut_right(bytes(getattr(pk, "qual%d" % m)[i, :n]), p.cut_right_window, p.cut_right_quality)
            wins.append(None if n is None else seq[:n])
        if any(w is None for w in wins):
            continue
        for w in wins:
            _, b = ref_polyg(w, p.polyg_compare_req, p.polyg_max_mismatch, p.polyg_one_mismatch_per)
            if b is not None:
                reads, bases = reads + 1, bases + b
    return reads, bases


def run_engine(lib, p, pk):
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, pk.n, pk.stride, ctypes.byref(h)) == 0, lib.fq_engine_last_error(None)
    try:
        res = pk.result_array()
        assert lib.fq_engine_process(h, ctypes.byref(pk.batch()), res.ctypes.data) == 0, lib.fq_engine_last_error(h)
        acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
        assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0, lib.fq_engine_last_error(h)
        return res, acc
    finally:
        lib.fq_engine_destroy(h)


def run_oracle(oracle, p, pk):
    res = pk.result_array()
    acc = np.zeros(abi.acc_words(p.insert_size_max, p.max_cycles), np.uint64)
    assert oracle.orc_process_batch(ctypes.byref(p), ctypes.byref(pk.batch()), res.ctypes.data, acc.ctypes.data) == 0
    return res, acc


def params(name, pset):
    if name == "SE":  # single-end, -q with polyG on
        p = abi.default_params(paired=False, max_cycles=512)
        p.qual_filter_enabled = 1
        p.polyg_enabled = 1
    else:
        p = config(name, max_cycles=512)
    p.polyg_compare_req, p.polyg_max_mismatch, p.polyg_one_mismatch_per = pset
    return p


def check(eng_lib, oracle, name, L, stride, pset):
    p = params(name, pset)
    pk = build_pack(L, stride, pset[2], bool(p.cut_right), name != "SE")
    res_o, acc_o = run_oracle(oracle, p, pk)
    reads, bases = expected_counts(p, pk)
    assert reads > pk.n // 3
    acc_g = acc_o
    if p.polyx_enabled:  # (polyX counts its own G tails in the same cells: the polyG counts come from a run without it)
        pg = type(p).from_buffer_copy(p)
        pg.polyx_enabled = 0
        acc_g = run_oracle(oracle, pg, pk)[1]
    assert (int(acc_g[abi.FQ_ACC_POLYX_READS + 3]), int(acc_g[abi.FQ_ACC_POLYX_BASES + 3])) == (reads, bases)
    res_e, acc_e = run_engine(eng_lib, p, pk)
    bad = np.nonzero(res_o != res_e)[0]
    assert bad.size == 0, f"{bad.size} result records differ; first #{bad[0]}: oracle={res_o[bad[0]]} engine={res_e[bad[0]]}"
    bad = np.nonzero(acc_o != acc_e)[0]
    assert bad.size == 0, f"{bad.size} accumulator words differ; first idx {bad[:8]}: oracle={acc_o[bad[:8]]} engine={acc_e[bad[:8]]}"


@pytest.mark.parametrize("pset", PARAM_SETS, ids=lambda s: "req%d_mm%d_per%d" % s)
@pytest.mark.parametrize("name", ["C3", "C4", "C5", "SE"])
@pytest.mark.parametrize("L,stride", [(150, 160), (144, 144)])
def test_polyg_tails(eng_lib, oracle, name, L, stride, pset):
    """2x150 in a stride-160 batch and the !FIX twin (144 on a stride-144 batch): LEAN (C3), merge (C4),
    FULL with cut_right ending the window early (C5; C4 cuts too) and a single-end config."""
    check(eng_lib, oracle, name, L, stride, pset)


@pytest.mark.parametrize("pset", [PARAM_SETS[0], PARAM_SETS[2], (1, 30, 10)], ids=lambda s: "req%d_mm%d_per%d" % s)
@pytest.mark.parametrize("name", ["C3", "C5", "SE"])
def test_polyg_tails_long_build(eng_lib, oracle, name, pset):
    """The 320-position build (2x300 on a stride-304 batch): tails of up to 19 groups, more than one
    row of 16 lanes takes in a turn; with an allowance of up to 30 the scan of a sparse tail runs on
    past group 15."""
    check(eng_lib, oracle, name, 300, 304, pset)
