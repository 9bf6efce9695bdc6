"""The fast kernels' overlap candidate scan (ov_candidates, fqtool_amd/csrc/pe_fast.hip) against the
CPU restatement: records and the whole accumulator, word for word.

The scan takes a column's candidate offsets 32 at a time (bit planes, carry-save counts of the first
16 compared positions against the threshold), so the packs here put true overlaps, adapter copies
and near-threshold decoys at the seams of those blocks, with read lengths that end the scan after 2,
3 and 4 blocks (6 and 7 in the 320-position build).  Every pack is at most a few thousand pairs built
on the CPU.

The build whose rows may be shorter than the column (the `!FIX` instantiations) runs for a batch
stride below 160: the stride is a multiple of 16, so the longest read there is 144, not 147, and
the seam offsets past its scan (cnt = 114) do not exist.
"""
import ctypes
import random

import numpy as np
import pytest

from fqtool_amd import abi
from batch_util import AD1, AD2, Pack, config, run_oracle

pytestmark = pytest.mark.gpu

SEAMS = [0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 94, 95, 96, 97, 118, 119]
COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")


@pytest.fixture(scope="module")
def eng_lib():
    return abi.load_engine()


def rand_seq(rng, n):
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def other_base(rng, b):
    return rng.choice([x for x in b"ACGT" if x != (b & 0xDF)])


def near_copy(rng, src, mism, extra):
    """src (16 bases) with exactly `mism` code mismatches (substitutions), plus, at a matching position,
    a lowercase copy of the base (extra 'lower': the same 2-bit code, another byte) or an N over a G
    (extra 'N': N shares G's code)."""
    w = bytearray(src)
    pos = rng.sample(range(16), mism)
    for k in pos:
        w[k] = other_base(rng, w[k])
    free = [k for k in range(16) if k not in pos]
    if extra == "lower":
        k = rng.choice(free)
        w[k] |= 0x20
    elif extra == "N":
        g = [k for k in free if w[k] == ord("G")]
        if g:
            w[rng.choice(g)] = ord("N")
    return w


def overlap_pair(rng, L1, L2, off, subs=0, decoys=()):
    """Reads whose true overlap offset is `off`: read 1 covers template positions [0, L1), the reverse
    complement of read 2 covers [off, off + L2); `subs` substitutions inside the overlap.  decoys:
    (d, mism, extra) -- the 16 positions from d of the moving window (read 1 for off >= 0, read 2's
    reverse complement for off < 0), all outside the overlap, made a near copy of the fixed window's
    first 16, so the scan meets a window with exactly `mism` code mismatches before the true offset."""
    lo, hi = min(0, off), max(L1, off + L2)
    t = rand_seq(rng, hi - lo)
    # no G at either read's end: polyG trimming would shorten the read and with it the scan
    t[L1 - 1 - lo] = rng.choice(b"ACT")
    t[off - lo] = rng.choice(b"AGT")
    r1 = bytearray(t[-lo:-lo + L1])
    rc2 = bytearray(t[off - lo:off - lo + L2])
    o0, o1 = max(0, off), min(L1, off + L2)  # the overlap, in read 1's coordinates
    for _ in range(subs):
        k = rng.randrange(o0, min(o1, L1 - 1))
        r1[k] = other_base(rng, r1[k])
    for d, mism, extra in decoys:
        assert d + 16 <= abs(off)
        if off >= 0:
            r1[d:d + 16] = near_copy(rng, rc2[:16], mism, extra)
        else:
            rc2[d:d + 16] = near_copy(rng, r1[:16], mism, extra)
    return bytes(r1), bytes(rc2).translate(COMP)[::-1]


def put(pk, i, r1, r2, rng):
    pk.set(i, 1, r1, bytes(33 + rng.randint(30, 40) for _ in r1))
    pk.set(i, 2, r2, bytes(33 + rng.randint(30, 40) for _ in r2))


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


def overlapped_pairs(p, acc):
    """Pairs the overlap analysis found overlapping: the insert-size histogram without its last cell
    (pairs of unknown insert size)."""
    return int(acc[abi.FQ_ACC_INSERT:abi.FQ_ACC_INSERT + p.insert_size_max].sum())


def check(eng_lib, oracle, p, pk, min_overlaps=0, min_adseq=0):
    """The pack does what it was built for (the oracle finds its overlaps / adapters), and the engine's
    records and accumulator equal the oracle's."""
    res_o, acc_o = run_oracle(oracle, p, pk)
    assert overlapped_pairs(p, acc_o) >= min_overlaps
    assert int(((res_o["flags"] & abi.FQ_RF_AD_SEQ) != 0).sum()) >= min_adseq
    res_e, acc_e = run_engine(eng_lib, p, pk)
    bad = np.nonzero(res_o != res_e)[0]
    assert bad.size == 0, f"{bad.size} result records differ; first #{bad[0]}: oracle={res_o[bad[0]]} engine={res_e[bad[0]]}"
    bad = np.nonzero(acc_o != acc_e)[0]
    assert bad.size == 0, f"{bad.size} accumulator words differ; first idx {bad[:8]}: oracle={acc_o[bad[:8]]} engine={acc_e[bad[:8]]}"


def params(name, limit=5):
    """Config `name` (batch_util.config; a "_no_polyg" suffix switches polyG trimming off: it takes
    the last base off nearly every read and with it the scan's last offset) with the given
    overlap_diff_limit."""
    p = config(name.split("_")[0], max_cycles=512)
    p.overlap_diff_limit = limit
    if name.endswith("_no_polyg"):
        p.polyg_enabled = 0
    return p


def seam_pack(L, stride, seams, seed, reps=3):
    """True overlaps at every seam offset of both phases (offset and -offset), `reps` pairs each with
    0 .. 2 substitutions, between pairs that do not overlap at all."""
    rng = random.Random(seed)
    offs = [o for o in seams if o <= L - 30 - 1]
    offs = offs + [-o for o in offs if o]
    rows = []
    for off in offs:
        for r in range(reps):
            rows.append(overlap_pair(rng, L, L, off, subs=r))
    for _ in range(len(rows) // 4):
        rows.append((bytes(rand_seq(rng, L)), bytes(rand_seq(rng, L))))
    rng.shuffle(rows)
    pk = Pack(len(rows), stride, True)
    for i, (r1, r2) in enumerate(rows):
        put(pk, i, r1, r2, rng)
    return pk, len(offs) * reps


@pytest.mark.parametrize("name", ["C3", "C3_no_polyg", "C5", "C4"])
@pytest.mark.parametrize("L,stride", [(150, 160), (144, 144)])
def test_true_overlaps_at_every_seam(eng_lib, oracle, name, L, stride):
    """2x150 in a stride-160 batch (offsets up to 119) and the !FIX twin on a stride-144 batch, with the
    LEAN (C3), FULL (C5) and merge (C4: the second analysis) variants.  polyG trimming takes the last
    base off nearly every read, which puts the last offsets (118, 119) just past the scan: found
    without it (C3_no_polyg), masked off with it."""
    pk, planted = seam_pack(L, stride, SEAMS, seed=L * 7 + len(name))
    p = params(name)
    check(eng_lib, oracle, p, pk, min_overlaps=planted if p.polyg_enabled == 0 else planted * 9 // 10)


# cnt = length - 30 (a base less once polyG trimming took the last one): 16, 32, 64, 96 and 120 --
# 2, 2, 2, 3 and 4 blocks, the exact multiples of 32 reached with and without that trimming
LENGTHS = [46, 47, 62, 63, 94, 95, 126, 127, 150]


def mixed_length_pack(seed):
    """Tiles of 32 pairs of one read length with a single pair of another (every ordered choice of the
    two): the tile's block count is set by one lane only.  Each pair overlaps at a random offset of
    either phase, or at the last offset its length allows."""
    rng = random.Random(seed)
    tiles = [(a, b) for a in LENGTHS for b in LENGTHS]
    pk = Pack(32 * len(tiles), 160, True)
    for t, (base, odd) in enumerate(tiles):
        lane = rng.randrange(32)
        for k in range(32):
            L = odd if k == lane else base
            L2 = L if rng.random() < 0.7 else rng.choice(LENGTHS)
            cnt1, cnt2 = L - 32, L2 - 32  # (polyG trimming takes a base or two off each read)
            u = rng.random()
            if u < 0.4:
                off = rng.randrange(0, cnt1)
            elif u < 0.5:
                off = cnt1 - 1
            elif u < 0.9:
                off = -rng.randrange(1, cnt2)
            else:
                off = -(cnt2 - 1)
            put(pk, 32 * t + k, *overlap_pair(rng, L, L2, off, subs=rng.randrange(3)), rng)
    return pk


@pytest.mark.parametrize("name", ["C3", "C3_no_polyg", "C5", "C4"])
def test_block_counts(eng_lib, oracle, name):
    pk = mixed_length_pack(seed=len(name) + 11)
    check(eng_lib, oracle, params(name), pk, min_overlaps=pk.n * 9 // 10)


def decoy_pack(seed, L=150, stride=160, spots=(3, 31, 32, 45, 63, 64, 80, 96, 101), last=117):
    """Windows with exactly 4 and exactly 5 code mismatches in their first 16 positions (and, for a
    threshold of 3 or 9, 2 / 3 and 8 / 9) in each block and at the seams, ahead of the true offset, in
    both phases; plain, with a lowercase base and with an N inside the compared window."""
    rng = random.Random(seed)
    rows = []
    for d in spots:
        for mism in (2, 3, 4, 5, 8, 9):
            for extra in (None, "lower", "N"):
                for sign in (1, -1):
                    off = rng.choice([d + 16, rng.randrange(d + 16, last + 1), last])
                    decoys = [(d, mism, extra)]
                    if d >= 32 and rng.random() < 0.5:  # a second decoy in an earlier block
                        decoys.append((rng.randrange(0, d - 16), rng.choice([4, 5]), None))
                    rows.append(overlap_pair(rng, L, L, sign * off, subs=rng.randrange(2), decoys=decoys))
    rng.shuffle(rows)
    pk = Pack(len(rows), stride, True)
    for i, (r1, r2) in enumerate(rows):
        put(pk, i, r1, r2, rng)
    return pk


@pytest.mark.parametrize("name,limit", [("C3", 5), ("C3", 3), ("C3", 9), ("C5", 5), ("C4", 5), ("C4", 9)])
def test_decoys_around_the_threshold(eng_lib, oracle, name, limit):
    """overlap_diff_limit 5 (the shortcut compare), 3 and 9 (the bit-sliced compare against K)."""
    pk = decoy_pack(seed=limit * 31 + len(name))
    check(eng_lib, oracle, params(name, limit), pk, min_overlaps=pk.n * 8 // 10)


def adapter_seam_pack(ads, lengths, stride, seams, seed, reps=2):
    """Independent mates (no overlap) holding a copy of their adapter at every seam position of the
    by-sequence scan (cnt = length - 15), some behind a decoy: the adapter's first 16 bases with
    about as many mismatches as the scan's bound (adapter length / 8 + 1) allows."""
    rng = random.Random(seed)
    rows = []
    for L in lengths:
        for pos in [s for s in seams if s <= L - 16] + [L - 16, L - 17]:
            for r in range(reps):
                pair = []
                for m in (0, 1):
                    ad = ads[m].encode()
                    K = len(ad) // 8 + 1
                    seq = rand_seq(rng, L)
                    piece = bytearray(ad[:L - pos])
                    for _ in range(r):
                        k = rng.randrange(len(piece))
                        piece[k] = rng.choice([other_base(rng, piece[k]), ord("N"), piece[k] | 0x20])
                    seq[pos:pos + len(piece)] = piece
                    if pos >= 16 and rng.random() < 0.6:
                        d = rng.choice([x for x in (0, pos - 16, min(31, pos - 16), min(32, pos - 16), rng.randrange(pos - 15))])
                        seq[d:d + 16] = near_copy(rng, ad[:16], rng.choice([K - 1, K]), rng.choice([None, "lower", "N"]))
                    pair.append(bytes(seq))
                rows.append(tuple(pair))
    rng.shuffle(rows)
    pk = Pack(len(rows), stride, True)
    for i, (r1, r2) in enumerate(rows):
        put(pk, i, r1, r2, rng)
    return pk


@pytest.mark.parametrize("ads", [(AD1, AD2), (AD1[:20], AD2[:21]), (AD1 + AD2, AD2 + AD1)])
def test_adapters_by_sequence_at_every_seam(eng_lib, oracle, ads):
    """C3 with explicit adapters: adseq_search's use of the scan, with its own bound (5, 3 and 9 for
    these adapter lengths) and cnt."""
    p = params("C3b")
    abi.set_adapter(p, 1, ads[0])
    abi.set_adapter(p, 2, ads[1])
    pk = adapter_seam_pack(ads, [47, 79, 111, 150], 160, SEAMS + [133, 134], seed=len(ads[0]))
    check(eng_lib, oracle, p, pk, min_adseq=pk.n)


LONG_SEAMS = SEAMS + [127, 128, 159, 160, 161, 190, 191, 192, 193, 219, 220, 223]


@pytest.mark.parametrize("name", ["C3", "C5"])
@pytest.mark.parametrize("L", [222, 250, 254])
def test_long_build_true_overlaps(eng_lib, oracle, name, L):
    """The 320-position build on a stride-256 batch: lengths 222 and 254 end the scan after 6 and 7
    blocks, 2x250 inside the seventh; true offsets up to the last one of the last block."""
    seams = LONG_SEAMS + [L - 33, L - 31]
    pk, planted = seam_pack(L, 256, seams, seed=L + len(name), reps=2)
    check(eng_lib, oracle, params(name), pk, min_overlaps=planted * 9 // 10)


def test_long_build_decoys_and_adapters(eng_lib, oracle):
    pk = decoy_pack(seed=5, L=250, stride=256, spots=(3, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 200), last=217)
    check(eng_lib, oracle, params("C3"), pk, min_overlaps=pk.n * 8 // 10)
    p = params("C3b")
    pk = adapter_seam_pack((AD1, AD2), [222, 254], 256, LONG_SEAMS + [238], seed=9)
    check(eng_lib, oracle, p, pk, min_adseq=pk.n)
