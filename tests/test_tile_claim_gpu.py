"""The fast kernels' tile hand-out on the GPU (fqtool_amd/csrc/tile_claim.h, pe_fast.hip): tiles below
T0 go round the grid's W waves in a fixed stride, the launch's last tiles are claimed from a device
counter that the engine clears before every launch.  Every record and the whole accumulator against
the CPU restatement, for batches of one tile, just over one tile, one tile short of and one pair past a
round of the grid (all claimed), and ten rounds and a ragged tile (eight strided rounds, then the
claimed tail).  A tile run twice or not at all, or a claim past the last tile, shows in the records
and in the accumulator's sums.

W = 16 waves per CU (every fast-kernel layout of the 160-position build); a tile is 32 pairs, or 64
single-end reads."""
import ctypes
import functools

import numpy as np
import pytest

from fqtool_amd import abi
from batch_util import config
from sample_parity import device_batch, engine_run, first_diff, host_copy, oracle_parallel

pytestmark = pytest.mark.gpu

STRIDE, L, SEED = 160, 150, 20261015
REC = np.dtype(abi.RESULT_DTYPE_FIELDS)


@pytest.fixture(scope="module")
def eng_lib():
    return abi.load_engine()


@functools.lru_cache(maxsize=None)
def grid_waves():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 16


def sizes(paired):
    T, W = (32 if paired else 64), grid_waves()
    return [1, T + 1, T * W - 1, T * W + 1, T * (10 * W) + 17]


@functools.lru_cache(maxsize=2)
def synth(n, paired, exotic_every=0):
    """A synthetic device batch and its host copy (shared by the configs run at one size)."""
    import torch

    lib = abi.load_engine()
    dev = torch.device("cuda:0")
    planes = [torch.empty(abi.batch_bytes(n, STRIDE), dtype=torch.uint8, device=dev) for _ in range(4 if paired else 2)]
    lens = [torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2 if paired else 1)]
    b = device_batch(planes, lens, n, STRIDE, paired)
    assert lib.fq_synth_fill_device(ctypes.byref(b), SEED, 5 * 10**9, L, None) == 0
    if exotic_every:  # a lowercase base at position 5 of read 1: the pair goes to the general kernel
        i = torch.arange(0, n, exotic_every, device=dev, dtype=torch.int64)
        planes[0][(i // 32) * 32 * STRIDE + (i % 32) * 16 + 5] = ord("a")
    torch.cuda.synchronize()
    return planes, lens, host_copy(torch, planes, lens, paired)


def params(name):
    return config(name, max_cycles=320 if name == "C4" else 256)


def check(lib, oracle, name, n, exotic_every=0):
    import torch

    p = params(name)
    paired = bool(p.paired)
    planes, lens, (hp, l1, l2) = synth(n, paired, exotic_every)
    eres, eacc = engine_run(lib, torch, p, planes, lens, n, STRIDE, paired, 0)
    got = eres.cpu().numpy().view(REC)
    ores, oacc = oracle_parallel(oracle, p, hp, l1, l2, n, STRIDE)
    nbad, i = first_diff(got, ores)
    assert nbad == 0, f"{nbad} records differ; first #{i}: oracle={ores[i]} engine={got[i]}"
    nbad, i = first_diff(eacc, oacc)
    assert nbad == 0, f"{nbad} accumulator words differ; first word {i}: oracle={oacc[i]} engine={eacc[i]}"
    assert int(oacc[abi.FQ_ACC_FILTER:abi.FQ_ACC_FILTER + 32].sum()) == n * (2 if paired else 1)
    return oacc


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("name", ["C3", "C2"])
def test_every_tile_once(eng_lib, oracle, name, k):
    check(eng_lib, oracle, name, sizes(name != "C2")[k])


@pytest.mark.parametrize("name", ["C4", "C5"])
def test_other_variants_ten_rounds(eng_lib, oracle, name):
    check(eng_lib, oracle, name, sizes(True)[-1])


def test_counter_cleared_every_launch(eng_lib):
    """Three launches on one handle, the accumulator zeroed in between: the same output each time
    (a counter left at the last launch's end would hand out no tile of the claimed part)."""
    import torch

    lib = eng_lib
    p = params("C3")
    n = 32 * (2 * grid_waves()) + 5  # one strided round, then a round and a ragged tile claimed
    planes, lens, _ = synth(n, True)
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, 0, 0, ctypes.byref(h)) == 0, lib.fq_engine_last_error(None)
    try:
        b = device_batch(planes, lens, n, STRIDE, True)
        outs = []
        for _ in range(3):
            assert lib.fq_engine_reset_acc(h) == 0, lib.fq_engine_last_error(h)
            res = torch.zeros(n * 32, dtype=torch.uint8, device=planes[0].device)
            assert lib.fq_engine_process_device(h, ctypes.byref(b), res.data_ptr(), None) == 0, lib.fq_engine_last_error(h)
            assert lib.fq_engine_sync(h) == 0, lib.fq_engine_last_error(h)
            acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
            assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0, lib.fq_engine_last_error(h)
            outs.append((res.cpu().numpy(), acc))
    finally:
        lib.fq_engine_destroy(h)
    assert int(outs[0][1][abi.FQ_ACC_FILTER:abi.FQ_ACC_FILTER + 32].sum()) == 2 * n
    for res, acc in outs[1:]:
        assert np.array_equal(res, outs[0][0])
        assert np.array_equal(acc, outs[0][1])


def test_hand_off_items_once(eng_lib, oracle):
    """One pair in a hundred holds a lowercase base and goes over to the general kernel through the
    hand-off list, whose slots the waves reserve as they meet such pairs, in the strided and in the
    claimed part: each is still processed exactly once."""
    n = 32 * (2 * grid_waves()) + 5
    check(eng_lib, oracle, "C3", n, exotic_every=100)
