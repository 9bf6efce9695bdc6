"""Device inflate, the parts that run without a GPU: the kernel's member routine
(fqtool_amd/csrc/inflate_core.h) compiled for the host by tools/micro/inflate_sim.cpp and run under
AddressSanitizer / UBSan over every input of inflate_cases.py, valid and corrupt (the payload, the
output and the stand-in for LDS are heap blocks of exact size there, so any access the kernel would
make out of bounds is a report, and a report fails the test); the ABI's symbol list; and the tool's
FQ_GZ_IN_DEVICE=1 knob on an engine without the inflate calls (build/cpuhost/fqtool: the host
inflates everything)."""
import gzip
import os
import re
import subprocess
import zlib

import pytest

import e2e_util as E
import inflate_cases as C
from fqtool_amd import abi
from test_host_e2e import bgzf

SIM_SRC = os.path.join(abi.REPO_DIR, "tools", "micro", "inflate_sim.cpp")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """The simulation built by the compile line in its own header."""
    head = open(SIM_SRC).read().split("#include")[0]
    line = next(l for l in head.splitlines() if "g++ " in l)
    argv = line[line.index("g++"):].split()
    assert argv[:6] == ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread"]
    binary = str(tmp_path_factory.mktemp("sim") / "inflate_sim")
    argv[argv.index("-o") + 1] = binary
    subprocess.run(argv, check=True, cwd=abi.REPO_DIR)
    return binary


def run_sim(sim, members, tmp_path, tag):
    """[(status, produced, bytes of the member's output range)] for a chain of members."""
    src, dst = tmp_path / (tag + ".bgzf"), tmp_path / (tag + ".out")
    src.write_bytes(C.chain(members))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sim, str(src), str(dst)], capture_output=True, timeout=600, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(members)
    out, at, res = dst.read_bytes(), 0, []
    for i, (line, m) in enumerate(zip(lines, members)):
        idx, st, produced, crc = line.split()
        assert int(idx) == i
        rng = out[at:at + m[2]]
        assert int(produced) <= m[2] and int(crc, 16) == zlib.crc32(rng[:int(produced)])
        assert rng[int(produced):] == b"\xA5" * (m[2] - int(produced)), "bytes after the produced ones were written"
        res.append((int(st), int(produced), rng))
        at += m[2]
    assert at == len(out)
    return res


def check_against_zlib(members, res, must_be_ok=False):
    """The assertions every case is held to; returns the members where the device and zlib differ."""
    differ = []
    for i, (m, (st, produced, got)) in enumerate(zip(members, res)):
        ok, want = C.verdict(m)
        assert produced <= m[2]
        if st == abi.FQ_INFL_OK:
            assert ok, "member %d: accepted, zlib rejects it" % i
            assert produced == m[2] and got == want, "member %d differs from zlib's bytes" % i
        elif ok:
            differ.append(i)
        if must_be_ok:
            assert ok and st == abi.FQ_INFL_OK, "member %d: status %d" % (i, st)
    return differ


def test_valid_members_in_the_simulation(sim, tmp_path):
    valid = C.valid_members()
    members = [valid[k] for k in C.valid_order()]
    check_against_zlib(members, run_sim(sim, members, tmp_path, "valid"), must_be_ok=True)


def test_mixed_chain_in_the_simulation(sim, tmp_path):
    members = C.mixed_chain()
    assert sum(m[2] for m in members) > 2_000_000
    check_against_zlib(members, run_sim(sim, members, tmp_path, "mixed"), must_be_ok=True)


def test_corrupt_members_in_the_simulation(sim, tmp_path):
    cases = C.corrupt_cases()
    names = sorted(cases)
    members = [m for k in names for m in cases[k]]
    res = run_sim(sim, members, tmp_path, "corrupt")
    stricter = []
    for j, k in enumerate(names):
        ms, rs = cases[k], res[3 * j:3 * j + 3]
        differ = check_against_zlib(ms, rs)
        assert rs[0][0] == abi.FQ_INFL_OK and rs[2][0] == abi.FQ_INFL_OK, k  # the good neighbours
        assert 0 not in differ and 2 not in differ
        if differ:
            stricter.append(k)
        if not k.startswith("flip_"):
            assert not C.verdict(ms[1])[0] and rs[1][0] != abi.FQ_INFL_OK, k
    for kind in C.flip_sources():
        rejected = sum(not C.verdict(cases[k][1])[0] for k in names if k.startswith("flip_%s_" % kind))
        assert rejected >= 60, (kind, rejected)  # (keeps the test from going vacuous)
    print("members the device rejects and zlib accepts:", stricter)
    assert stricter == []
    st = {k: res[3 * j + 1][0] for j, k in enumerate(names)}
    assert st["block_type_3"] == st["hlit_287"] == st["oversubscribed_code_lengths"] == st["repeat_first"] == abi.FQ_INFL_DATA
    assert st["stored_nlen"] == st["distance_before_start"] == st["cut_by_1"] == st["cut_by_half"] == abi.FQ_INFL_DATA
    assert st["isize_minus_1"] == abi.FQ_INFL_LONG and st["isize_plus_1"] == abi.FQ_INFL_SHORT
    assert st["wrong_crc"] == abi.FQ_INFL_CRC


def test_symbols_listed_once():
    for name in ("fq_inflate_create", "fq_inflate_destroy", "fq_inflate_members", "fq_inflate_bgzf",
                 "fq_inflate_last_kernel_ms"):
        assert abi.ENGINE_SYMBOLS.count(name) == 1
    lib = abi.load_engine()
    for name in abi.ENGINE_SYMBOLS:
        assert hasattr(lib, name), name
    assert abi.FQ_INFLATE_MAX == 65536


def device_members(stderr):
    """[(device, host)] member counts of the tool's FQ_TIMING log, one entry per BGZF input."""
    return [(int(a), int(b)) for a, b in re.findall(r"bgzf input [^\n]*?: (\d+) members inflated on the device, (\d+) on the host",
                                                     stderr)]


def test_gz_in_device_knob_falls_back_without_the_calls(sim, tmp_path):
    """The CPU stand-in engine has no fq_inflate_*: the tool links, runs, inflates on the host and
    says so; its own .gz outputs (the host writer's members) go through the simulation too."""
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    binary = os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool")
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    for name in ("r1.fq.gz", "r2.fq.gz"):
        (inp / name).write_bytes(bgzf(gzip.open(os.path.join(E.INPUTS, name)).read()))
    case = "td_pe_qag"
    argv = [a.replace(E.INPUTS, str(inp)) for a in E.argv_for(binary, case, str(out))]
    p = subprocess.run(argv, capture_output=True, cwd=out, timeout=300, env=dict(os.environ, FQ_GZ_IN_DEVICE="1", FQ_TIMING="1"))
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    E.check_outputs(case, str(out))
    counts = device_members(p.stderr.decode(errors="replace"))
    assert len(counts) == 2 and all(d == 0 and h > 0 for d, h in counts), p.stderr.decode(errors="replace")[-2000:]
    # the host writer's members
    gz = tmp_path / "gz"
    gz.mkdir()
    p = subprocess.run(E.argv_for(binary, "td_pe_gz", str(gz)), capture_output=True, cwd=gz, timeout=300)
    assert p.returncode == 0
    seen = 0
    for name in sorted(os.listdir(gz)):
        if name.endswith(".gz"):
            data, members, pos = (gz / name).read_bytes(), [], 0
            while pos < len(data):
                assert data[pos:pos + 16] == C.HEAD
                size = int.from_bytes(data[pos + 16:pos + 18], "little") + 1
                members.append((data[pos + 18:pos + size - 8], int.from_bytes(data[pos + size - 8:pos + size - 4], "little"),
                                int.from_bytes(data[pos + size - 4:pos + size], "little")))
                pos += size
            check_against_zlib(members, run_sim(sim, members, tmp_path, "host_" + name), must_be_ok=True)
            seen += len(members)
    assert seen > 0
