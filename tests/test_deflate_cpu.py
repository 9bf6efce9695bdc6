"""Device BGZF, the parts that run without a GPU: the size bound, the kernels' Huffman length
builder run on the host (fq_deflate_code_lengths) against a plain package-merge written here, and
the tool's FQ_GZ_DEVICE=1 knob on an engine without the gz calls (build/cpuhost/fqtool: it falls
back to the host's compression, so every member carries XFL 0)."""
import ctypes
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import e2e_util as E
from fqtool_amd import abi


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


def test_bound(lib):
    for n, want in ((0, 0), (1, 32), (65280, 65311), (65281, 65343), (10 ** 7, 10 ** 7 + 31 * -(-10 ** 7 // 65280))):
        assert lib.fq_deflate_bound(n) == want
    assert abi.ENGINE_SYMBOLS.count("fq_deflate_bound") == 1


def package_merge(freq, max_len):
    """Optimal length-limited code lengths (Larmore & Hirschberg), the plain way: every item carries
    the list of its leaves."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    n = len(used)
    lens = [0] * len(freq)
    if n == 1:
        lens[used[0][1]] = 1
        return lens
    leaves = [(f, [s]) for f, s in used]
    prev = []
    for _ in range(max_len):
        merged = sorted(leaves + prev, key=lambda it: it[0])
        prev = [(merged[i][0] + merged[i + 1][0], merged[i][1] + merged[i + 1][1]) for i in range(0, len(merged) - 1, 2)]
        last = merged
    for _, syms in last[: 2 * n - 2]:
        for s in syms:
            lens[s] += 1
    return lens


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def fib_case(n_sym):
    freq = [0] * n_sym
    pos = np.random.default_rng(3).permutation(n_sym)[:22] if n_sym > 22 else range(n_sym)
    vals = fib(22) if n_sym > 22 else fib(n_sym)
    for p, v in zip(pos, vals):
        freq[int(p)] = v
    return freq


CASES = {
    "fib22_of_286": (fib_case(286), 15),  # an unlimited Huffman tree is 21 deep
    "fib19": (fib_case(19), 7),
    "one": ([0] * 100 + [5] + [0] * 185, 15),
    "two": ([0, 7, 0, 0, 1] + [0] * 25, 15),
    "equal286": ([3] * 286, 15),
    "equal19": ([1] * 19, 7),
    "equal30": ([9] * 30, 15),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_code_lengths(lib, name):
    freq, max_len = CASES[name]
    f = np.array(freq, np.uint32)
    out = np.full(f.size, 99, np.uint8)
    assert lib.fq_deflate_code_lengths(f.ctypes.data, f.size, max_len, out.ctypes.data) == 0
    used = [i for i, v in enumerate(freq) if v]
    for i, v in enumerate(freq):
        if v:
            assert 1 <= out[i] <= max_len, (i, out[i])
        else:
            assert out[i] == 0
    kraft = sum(Fraction(1, 2 ** int(out[i])) for i in used)
    assert kraft <= 1
    if len(used) >= 2:
        assert kraft == 1
    ref = package_merge(freq, max_len)
    assert all(1 <= ref[i] <= max_len for i in used) and sum(Fraction(1, 2 ** ref[i]) for i in used) <= 1
    cost = sum(int(out[i]) * freq[i] for i in used)
    assert cost <= sum(ref[i] * freq[i] for i in used), (cost, out[used].tolist(), [ref[i] for i in used])


def test_code_lengths_refusals(lib):
    f = np.ones(300, np.uint32)
    out = np.zeros(300, np.uint8)
    assert lib.fq_deflate_code_lengths(f.ctypes.data, 289, 15, out.ctypes.data) == abi.FQ_E_INVALID
    assert lib.fq_deflate_code_lengths(f.ctypes.data, 19, 16, out.ctypes.data) == abi.FQ_E_INVALID
    assert lib.fq_deflate_code_lengths(f.ctypes.data, 19, 4, out.ctypes.data) == abi.FQ_E_INVALID  # 19 > 2^4
    assert lib.fq_deflate_code_lengths(f.ctypes.data, 16, 4, out.ctypes.data) == 0
    assert out[:16].tolist() == [4] * 16


def bgzf_members(data):
    """(XFL, member bytes) along the chain of a BGZF file."""
    out, pos = [], 0
    while pos < len(data):
        h = data[pos:pos + 18]
        assert h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00", (pos, h)
        size = struct.unpack("<H", h[16:18])[0] + 1
        out.append((h[8], data[pos:pos + size]))
        pos += size
    assert pos == len(data)
    return out


def test_gz_device_knob_falls_back_without_the_calls(tmp_path):
    """The CPU stand-in engine has no fq_engine_set_gz_out: the tool links, runs and compresses on
    the host."""
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    binary = os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool")
    case = "td_pe_gz"
    argv = E.argv_for(binary, case, str(tmp_path))
    p = subprocess.run(argv, capture_output=True, cwd=tmp_path, timeout=300, env=dict(os.environ, FQ_GZ_DEVICE="1"))
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    E.check_outputs(case, str(tmp_path))
    seen = 0
    for name in os.listdir(tmp_path):
        if name.endswith(".gz"):
            for xfl, _ in bgzf_members(open(tmp_path / name, "rb").read()):
                assert xfl == 0
                seen += 1
    assert seen > 0
