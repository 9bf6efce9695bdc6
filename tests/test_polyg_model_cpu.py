"""Host-side model of the fast kernels' polyG tail scan (pe_fast.hip `polyg_bits`).

The kernel walks the scan indices of PolyX::trimPolyG (src/polyx.cpp:14-38) in groups of 16 and
never evaluates the allowance per base.  Per group g it takes two wave-uniform numbers, the
allowance at the group's first and last index (a0, a1).  The k-th non-G base of the read cannot break
the scan for k <= a0, always breaks it for k > a1, and for a0 < k <= a1 breaks it exactly when it sits
at a group position below k*per - 1 - 16g.  So a lane drops its a0 - (non-G bases before the group)
lowest non-G bits, tests one lowest bit per k in (a0, a1] against that k's position mask, and the
first bit left after those breaks.  (i+1)/per is ((i+1)*inv) >> 16 with inv = ceil(65536/per) while
per * 161 < 65536.

This restates that rule on the same spaced bit masks, with the kernel's stream addressing of both
mates' columns (read 2's column holds the reverse complement; read 1's words are bit-reversed), and
checks it against the oracle's restatement of the reference loop (orc_trim_polyg): exhaustively over
every non-G pattern of up to 14 bases, and on random reads of up to 160 bases.  The GPU parity of
the kernel itself is tests/test_polyg_scan_gpu.py.
"""
import ctypes
import itertools
import random

KMAXLEN = 160
KCHUNKS = KMAXLEN // 16
M32 = 0xFFFFFFFF

# (compare_req, max_mismatch, one_mismatch_per)
PARAM_SETS = [(1, 10, 10), (10, 1, 10), (10, 5, 8), (5, 0, 8), (1, 3, 1), (20, 10, 300)]


def posmask(n):
    return 0x55555555 if n >= 16 else 0 if n <= 0 else ((1 << (2 * n)) - 1) & 0x55555555


BREV16 = [int(f"{x:016b}"[::-1], 2) for x in range(1 << 16)]


def brev32(x):
    return BREV16[x & 0xFFFF] << 16 | BREV16[x >> 16]


def column(seq, rc):
    """The code and N / lowercase words of a read's column (staging's encoding): codes A C T G =
    0 1 2 3 from (byte >> 1) & 3, N bit for every byte outside ACGTacgt (its code reads as G's),
    flag bit for a lowercase letter; read 2's column holds the reverse complement of the whole row."""
    cw, nw = [0] * (KCHUNKS + 2), [0] * (KCHUNKS + 2)
    for i, b in enumerate(seq):
        up = b & ~0x20
        if up in b"ACGT":
            code, nbits = (up >> 1) & 3, 2 if b & 0x20 else 0
        else:
            code, nbits = 3, 3 if (b & 0x20 and chr(up).isalpha()) else 1
        pos = KMAXLEN - 1 - i if rc else i
        if rc:
            code ^= 2
        cw[pos >> 4] |= code << (2 * (pos & 15))
        nw[pos >> 4] |= nbits << (2 * (pos & 15))
    return cw, nw


def kernel_polyg(col, rc, st, n, compare_req, max_mm, per):
    """polyg_bits on the window [st, st + n) of the read whose column is col: (new length, bases or -1)."""
    cw, nw = col
    inv = (65536 + per - 1) // per if per * (KMAXLEN + 1) < 65536 else 0

    def allowed(x):
        return min(max_mm, max(1, (x * inv) >> 16 if inv else x // per))

    e = st + n - 1
    iend, last_g = n, -1
    if max_mm < 0:
        iend = 0
    else:
        gx = 0x55555555 if rc else M32
        sh = 2 * (~e & 15)
        step = 1 if rc else -1
        w = max(KCHUNKS - 1 - (e >> 4) if rc else e >> 4, 0)

        def sword(w):
            t = (cw[w] ^ gx) | nw[w]
            return t if rc else brev32(t)

        s0 = sword(w)
        w = max(w + step, 0)
        cum, i0 = 0, 0
        is_open = n > 0
        while is_open:
            a0, a1 = allowed(i0 + 1), allowed(i0 + 16)
            s1 = sword(w)
            al = (((s1 << 32) | s0) >> sh) & M32
            xg = (al | (al >> 1)) & 0x55555555
            s0 = s1
            w = max(w + step, 0)
            valid = posmask(n - i0)
            x = xg & valid
            gm = ~xg & valid
            pc = bin(x).count("1")
            if cum + pc > a0:
                m = x
                for _ in range(a0 - cum):
                    m &= m - 1
                brk = 0
                for k in range(a0 + 1, a1 + 1):
                    low = m & -m
                    if not brk and low & posmask(k * per - 1 - i0):
                        brk = low
                    m &= m - 1
                if not brk:
                    brk = m & -m
                if brk:
                    iend = i0 + (brk.bit_length() - 1) // 2
                    gm &= brk - 1
            cum += pc
            if gm:
                last_g = i0 + (gm.bit_length() - 1) // 2
            is_open = iend == n and i0 + 16 < n
            i0 += 16
    if iend + 1 < compare_req:
        return n, -1
    first_g = e - last_g - st if last_g >= 0 else n - 1
    return (n if first_g < 0 else first_g), n - first_g


def oracle_polyg(oracle, seq, compare_req, max_mm, per):
    bases = ctypes.c_int(0)
    n = oracle.orc_trim_polyg(bytes(seq), len(seq), compare_req, max_mm, per, ctypes.byref(bases))
    return n, bases.value


def test_every_non_g_pattern_up_to_14(oracle):
    """All 2^L placements of non-G bases for L <= 14 (L = 14: 16,384 reads), as read 1 and as read 2,
    with per small enough that the allowance steps inside the pattern."""
    small_per = [(1, 7, 2), (1, 7, 3), (1, 4, 5), (3, 2, 4)]
    for L in range(0, 15):
        # (L = 13, 14 are three quarters of the patterns: the extra sets run up to L = 12 only)
        sets = PARAM_SETS + small_per if L <= 12 else PARAM_SETS
        for bits in itertools.product(b"GA", repeat=L):
            seq = bytes(bits)
            cols = [column(seq, False), column(seq, True)]
            for cr, mm, per in sets:
                want = oracle_polyg(oracle, seq, cr, mm, per)
                for rc in (False, True):
                    assert kernel_polyg(cols[rc], rc, 0, L, cr, mm, per) == want, (seq, rc, cr, mm, per)


def test_random_reads_up_to_160(oracle):
    """G tails of every kind of length with sparse non-G bases, N, lowercase g and other lowercase
    letters in them, on windows that start past 0 (front trimming) and end before the read does."""
    rng = random.Random(20261020)
    sets = PARAM_SETS + [(1, 7, 1), (1, 7, 2), (1, 7, 3), (1, 6, 5), (1, 10, 16), (1, 0, 1)]
    for it in range(4000):
        L = rng.choice([rng.randrange(0, 161), 160, 150, rng.randrange(0, 40)])
        seq = bytearray(rng.choice(b"ACGT") for _ in range(L))
        T = min(L, rng.choice([0, 1, 5, rng.randrange(0, 161), rng.randrange(10, 70)]))
        rate = rng.choice([0.0, 0.03, 0.08, 0.15, 0.3])
        for i in range(L - T, L):
            seq[i] = rng.choice(b"ACTNgat") if rng.random() < rate else ord("G")
        st = rng.choice([0, 0, rng.randrange(0, L + 1)])
        n = rng.choice([L - st, L - st, rng.randrange(0, L - st + 1)])
        if rng.random() < 0.5 and n > 0:  # a G tail that ends where the window does
            for i in range(max(st, st + n - T), st + n):
                if rng.random() >= rate:
                    seq[i] = ord("G")
        cols = [column(bytes(seq), False), column(bytes(seq), True)]
        for cr, mm, per in rng.sample(sets, 4):
            want = oracle_polyg(oracle, seq[st:st + n], cr, mm, per)
            for rc in (False, True):
                got = kernel_polyg(cols[rc], rc, st, n, cr, mm, per)
                assert got == want, (bytes(seq), rc, st, n, cr, mm, per, got, want)
