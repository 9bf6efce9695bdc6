"""The removed-mode Stats pass's chunk set-up (fqtool_amd/csrc/pe_fast.hip) against the CPU
restatement: every result record and every accumulator word.

The pass counts read 2's bases from its reverse-complemented column under relabelled slots
(`rem_slot`; tests/test_stats_relabel_cpu.py has the chain) and adds an N's + 5 from flags spread to
nibbles the way the codes are.  A wrong label, a flag taken from the wrong bit of a field or a flush
that reads the rows unpermuted moves counts between the A C G T N cells of a cycle, in read 2's pre
or post block only, which the per-cycle accumulator words show.

Packs of 1 to 97 pairs; the mates' lengths differ and sit at the chunk seams.  Read 2 holds every one
of A C G T N at every position of a chunk, inside kept windows and inside removed tails: G tails of
10-60 bases with a stray base (polyG), inserts shorter than the reads (adapter read-through), reads
that fail -q (removed whole) or the N limit, several N in one chunk and N in the first and the last
chunk, lowercase a c g t and an IUPAC byte kept and removed.  `test_pack_covers_the_cases` checks
that on the CPU.  The -c packs hold overlapping pairs with 1-5 mismatches of Q >= 30 against
Q <= 14, so the correction rewrites read 2's cells.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from fqtool_amd import abi
from batch_util import AD1, AD2, Pack, run_oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 64, 97]
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 143, 144, 145, 159, 160]
STRIDES = [160, 144, 48, 256, 304]
# C2: no read 2 (control); C3_umi8: the pre/post-mode pass (control)
CONFIGS = ["C2", "C3", "C4", "C5", "C3_umi8"]
COMP = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


@pytest.fixture(scope="module")
def eng_lib():
    return abi.load_engine()


def params(name):
    import bench

    p = bench.config_params(abi, name.split("_")[0], max_cycles=640)
    if name.endswith("_umi8"):
        p.umi_front1 = p.umi_front2 = 8
    if name.endswith("_c"):
        p.correction_enabled = 1
    return p


def lengths_for(stride):
    ls = {l for l in LENGTHS if l <= stride}
    ls |= {stride - d for d in (0, 1, 15, 16, 17)}
    return sorted(ls)


def rand_bases(rng, n, n_rate=0.02):
    return bytearray(ord("N") if rng.random() < n_rate else rng.choice(b"ACGT") for _ in range(n))


def good_qual(rng, n):
    return bytearray(33 + rng.randint(20, 40) for _ in range(n))


def overlapping(rng, l1, l2, insert):
    """A pair cut from one fragment of `insert` bases; past the fragment each read runs into its
    adapter and then random bases (read-through: the tail is removed)."""
    frag = bytes(rng.choice(b"ACGT") for _ in range(insert))
    s1 = (frag + AD1.encode() + bytes(rand_bases(rng, l1, 0.05)))[:l1]
    s2 = (frag.translate(COMP)[::-1] + AD2.encode() + bytes(rand_bases(rng, l2, 0.05)))[:l2]
    return bytearray(s1), bytearray(s2)


@functools.lru_cache(maxsize=None)
def build_pack(n, stride, paired, correct=False):
    rng = random.Random(n * 1000 + stride + (7 if paired else 0) + (13 if correct else 0))
    ls = lengths_for(stride)
    long_ls = [l for l in ls if l >= 31]
    pk = Pack(n, stride, paired)
    for i in range(n):
        kind = rng.randrange(8) if n < 8 else i % 8
        if correct:
            kind = (1, 4, 4, 5)[i % 4]
        l1 = ls[(i // 8 + rng.randrange(2)) % len(ls)] if kind in (0, 3, 7) else rng.choice(long_ls)
        l2 = rng.choice([l for l in (ls if kind in (0, 3, 7) else long_ls) if l != l1])
        s1, s2 = rand_bases(rng, l1), rand_bases(rng, l2)
        q1, q2 = good_qual(rng, l1), good_qual(rng, l2)
        if kind == 1 or (kind == 5 and i % 16 >= 8):  # insert shorter than the reads
            s1, s2 = overlapping(rng, l1, l2, rng.randint(min(30, min(l1, l2) - 1), min(l1, l2) - 1))
        elif kind == 2:  # G tails of 10-60 bases, half of them with one other base inside
            for s in (s1, s2):
                t = min(rng.randint(10, 60), len(s) - 1)
                s[len(s) - t:] = b"G" * t
                if t >= 20 and rng.random() < 0.5:
                    s[len(s) - t + rng.randint(8, t - 9)] = rng.choice(b"ACTN")
        elif kind == 3:  # read 2 fails -q
            q2 = bytearray(33 + rng.randint(2, 12) for _ in range(l2))
            s2 = rand_bases(rng, l2, 0.03)
        elif kind == 4:  # overlapping, no read-through; with -c: mismatches that get corrected
            lo, hi = max(l1, l2), l1 + l2 - (60 if l1 + l2 - 60 >= max(l1, l2) else 30)
            ins = rng.randint(lo, max(lo, hi))
            s1, s2 = overlapping(rng, l1, l2, ins)
            ol = l1 + l2 - ins
            if correct and ol >= 30:
                for _ in range(rng.randint(1, 5 if ol >= 50 else 2)):
                    k = rng.randrange(ol)  # overlap index: read 1 at l1 - ol + k, read 2 at l2 - 1 - k
                    p1, p2 = l1 - ol + k, l2 - 1 - k
                    if not (0 <= p1 < l1 and 0 <= p2 < l2):
                        continue
                    if rng.random() < 0.7:  # read 2 takes read 1's base
                        s2[p2] = rng.choice([b for b in b"ACGT" if b != s2[p2]])
                        q1[p1], q2[p2] = 33 + rng.randint(30, 40), 33 + rng.randint(2, 14)
                    else:
                        s1[p1] = rng.choice([b for b in b"ACGTN" if b != s1[p1]])
                        q1[p1], q2[p2] = 33 + rng.randint(2, 14), 33 + rng.randint(30, 40)
        if kind == 5:  # lowercase and an IUPAC byte in read 2, early (kept) and late (removed or kept)
            for p, b in zip((1, 2, 3, 4, 6), b"acgtR"):
                if p < l2:
                    s2[p] = b
            for p, b in zip((l2 - 2, l2 - 3, l2 - 5, l2 - 6, l2 - 8), b"tgcaR"):
                if p > 8:
                    s2[p] = b
            if i % 16 < 8 and i % 32 >= 16:
                q2 = bytearray(33 + rng.randint(2, 12) for _ in range(l2))
        elif kind == 6:  # several N in one chunk; N in the first and the last chunk (within the N limit)
            s2 = bytearray(rng.choice(b"ACGT") for _ in range(l2))
            j = (i // 8) % 16
            for p in (j, j + 2, 16 * ((l2 - 1) // 16) + min(j, (l2 - 1) % 16), l2 - 1):
                if 0 <= p < l2:
                    s2[p] = ord("N")
        elif kind == 7:  # every base at every position of a chunk; over the N limit: removed whole
            s2 = bytearray(b"ACGTN"[(p + i // 8) % 5] for p in range(l2))
        pk.set(i, 1, bytes(s1), bytes(q1))
        if paired:
            pk.set(i, 2, bytes(s2), bytes(q2))
    return pk


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


def check(lib, oracle, p, pk):
    res_o, acc_o = run_oracle(oracle, p, pk)
    assert int(acc_o.sum()) > 0
    res_e, acc_e = run_engine(lib, p, pk)
    bad = np.nonzero(res_o != res_e)[0]
    assert bad.size == 0, f"{bad.size} result records differ; first #{bad[0]}: oracle={res_o[bad[0]]} engine={res_e[bad[0]]}"
    bad = np.nonzero(acc_o != acc_e)[0]
    assert bad.size == 0, f"{bad.size} accumulator words differ; first idx {bad[:8]}: oracle={acc_o[bad[:8]]} engine={acc_e[bad[:8]]}"
    return res_o


def test_pack_covers_the_cases(oracle):
    """(CPU only, the oracle's records) read 2 of the 97-pair packs under C3: each of A C G T N at each
    position of a chunk, kept and removed; lowercase and the IUPAC byte kept and removed; a read with
    several N in one chunk and N in its first and last chunk that passes."""
    p = params("C3")
    seen, exotic, n_read = set(), set(), False
    for stride in (160, 144):
        pk = build_pack(97, stride, True)
        res, _ = run_oracle(oracle, p, pk)
        for i in range(pk.n):
            r = res[2 * i + 1]
            L = int(pk.len2[i])
            kept_to = int(r["start"]) + int(r["len"]) if r["code"] == 0 else 0
            s = bytes(pk.seq2[i, :L])
            for pos, b in enumerate(s):
                if b in b"ACGTN":
                    seen.add((chr(b), pos % 16, pos < kept_to))
                else:
                    exotic.add((chr(b), pos < kept_to))
            ns = [pos for pos, b in enumerate(s) if b == ord("N") and pos < kept_to]  # (a last-base N is trimmed)
            if len(ns) >= 3 and ns[0] < 16 and ns[-1] >= 16 * ((L - 1) // 16) and \
                    any(b - a <= 2 for a, b in zip(ns, ns[1:])):
                n_read = True
    missing = [(b, m, k) for b in "ACGTN" for m in range(16) for k in (False, True) if (b, m, k) not in seen]
    assert not missing, missing
    missing = [(b, k) for b in "acgtR" for k in (False, True) if (b, k) not in exotic]
    assert not missing, missing
    assert n_read


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", CONFIGS)
def test_stats_chunks(eng_lib, oracle, name, stride, n):
    check(eng_lib, oracle, params(name), build_pack(n, stride, name != "C2"))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("stride", [160, 144, 48])
@pytest.mark.parametrize("name", ["C3_c", "C4_c"])
def test_stats_chunks_corrected(eng_lib, oracle, name, stride, n):
    p = params(name)
    res = check(eng_lib, oracle, p, build_pack(n, stride, True, correct=True))
    if n >= 31 and stride >= 144:  # the packs do what they are for: read 2 of some pair was corrected
        assert any(res[2 * i + 1]["flags"] & abi.FQ_RF_CORRECTED for i in range(n))
