"""The fast kernels' row requests (staging and the Stats pass's quality re-reads,
fqtool_amd/csrc/pe_fast.hip) against the CPU restatement: records and the whole accumulator, word for
word.

A wave asks for its rows chunk by chunk (16 bytes per lane, 512 bytes per 32-row tile block and
plane), some chunks ahead of their use and clamped to the row's last chunk.  However those requests
are shaped -- per lane, as shipped, or by half-waves that each fetch one chunk of a chunk pair for
the rows of both halves and swap (tried, not kept: DESIGN.md) -- a chunk that lands in the wrong lane
half, the wrong buffer or the wrong mate, a bad clamp at an odd chunk count, or an address taken
from a tile that the pack does not have moves bases and qualities to other cycles or other reads,
which the per-cycle Stats cells and the records show.

The packs are as small as the cases allow: 1 to 97 pairs (single-end: reads), so the last tile is
partial and a single-end wave's upper 32-row tile is absent (1-32), partial (33-63, 65-95) or whole;
read lengths at the chunk seams and the row end, differing between the mates of a pair; random bases
and qualities, so no two chunks of a pack agree.  Row strides 160 (rows of exactly the column
length), 144 and 48 (9 and 3 chunks) and, for the 320-position build, 256 and 304 (16 and 19 chunks).
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from fqtool_amd import abi
from batch_util import Pack, run_oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 63, 64, 65, 97]
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 143, 144, 145, 159, 160]
STRIDES = [160, 144, 48, 256, 304]
# the BASELINE configs (LEAN single-end, LEAN, merge, FULL) and the -c / UMI / -e instantiation
CONFIGS = ["C2", "C3", "C4", "C5", "C3_umi8"]


@pytest.fixture(scope="module")
def eng_lib():
    return abi.load_engine()


def params(name):
    import bench

    p = bench.config_params(abi, name.split("_")[0], max_cycles=640)
    if name == "C3_umi8":
        p.umi_front1 = p.umi_front2 = 8
    return p


def lengths_for(stride):
    """The seam lengths that fit the row, and the same seams at the end of a longer row."""
    ls = {l for l in LENGTHS if l <= stride}
    ls |= {stride - d for d in (0, 1, 15, 16, 17) if stride - d >= 0}
    return sorted(ls)


@functools.lru_cache(maxsize=None)
def build_pack(n, stride, paired):
    rng = random.Random(n * 1000 + stride + (7 if paired else 0))
    ls = lengths_for(stride)
    pk = Pack(n, stride, paired)
    for i in range(n):
        # every length comes up within a tile's rows; the mates' lengths differ
        l1 = ls[(i + rng.randrange(2)) % len(ls)] if n >= len(ls) else rng.choice(ls)
        l2 = rng.choice([l for l in ls if l != l1])
        for m, L in ((1, l1), (2, l2)) if paired else ((1, l1),):
            seq = bytes(rng.choice(b"ACGTACGTACGTACGTN") for _ in range(L))
            qual = bytes(33 + rng.randint(2, 41) for _ in range(L))
            pk.set(i, m, seq, qual)
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


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", CONFIGS)
def test_staged_rows(eng_lib, oracle, name, stride, n):
    p = params(name)
    pk = build_pack(n, stride, name != "C2")
    res_o, acc_o = run_oracle(oracle, p, pk)
    assert int(acc_o.sum()) > 0
    res_e, acc_e = run_engine(eng_lib, p, pk)
    bad = np.nonzero(res_o != res_e)[0]
    assert bad.size == 0, f"{bad.size} result records differ; first #{bad[0]}: oracle={res_o[bad[0]]} engine={res_e[bad[0]]}"
    bad = np.nonzero(acc_o != acc_e)[0]
    assert bad.size == 0, f"{bad.size} accumulator words differ; first idx {bad[:8]}: oracle={acc_o[bad[:8]]} engine={acc_e[bad[:8]]}"
