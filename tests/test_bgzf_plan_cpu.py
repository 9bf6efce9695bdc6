"""The BGZF window planner of the raw stream's device inflate (fqtool_amd/host/bgzf_plan.h,
FQ_GZ_IN_DEVICE=2), without a GPU: tools/micro/bgzf_plan_sim.cpp runs it under AddressSanitizer /
UBSan over BGZF files written here, and the windows are checked against this file's own walk of
each file.  A window's members are the non-empty members that hold one of its bytes, the empty
members between them, and the empty members at its end (at the stream's end: the EOF members).
Also the tool's knob on an engine without the new call (build/cpuhost/fqtool): today's route."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import e2e_util as E
from fqtool_amd import abi
from test_host_e2e import bgzf
from test_inflate_cpu import device_members

SIM_SRC = os.path.join(abi.REPO_DIR, "tools", "micro", "bgzf_plan_sim.cpp")
MIB = 1 << 20
HEAD = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0])


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """The program built by the compile line in its own header."""
    head = open(SIM_SRC).read().split("#include")[0]
    line = next(l for l in head.splitlines() if "g++ " in l)
    argv = line[line.index("g++"):].split()
    assert argv[:6] == ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread"]
    binary = str(tmp_path_factory.mktemp("plan") / "bgzf_plan_sim")
    argv[argv.index("-o") + 1] = binary
    subprocess.run(argv, check=True, cwd=abi.REPO_DIR)
    return binary


def text_of(n, seed=1):
    rng = random.Random(seed)
    line = bytes(rng.choice(b"ACGT") for _ in range(4096))
    return (line * (n // 4096 + 1))[:n]


def write_chain(path, text, sizes):
    """The text as BGZF members of the given inflated sizes (0: an empty member), in file order."""
    out, at = bytearray(), 0
    for s in sizes:
        blk = text[at:at + s]
        at += s
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        d = c.compress(blk) + c.flush()
        out += HEAD + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(blk), len(blk))
    assert at == len(text)
    path.write_bytes(bytes(out))


def walk(path):
    """[(payload offset, payload bytes, isize, crc, stream offset)] from the file's headers."""
    data, pos, at, ms = path.read_bytes(), 0, 0, []
    while pos < len(data):
        assert data[pos:pos + 16] == HEAD
        size = struct.unpack_from("<H", data, pos + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", data, pos + size - 8)
        ms.append((pos + 18, size - 26, isize, crc, at))
        at += isize
        pos += size
    return ms, at


def equal_sizes(total, msize, eof=True):
    return [msize] * (total // msize) + ([total % msize] if total % msize else []) + ([0] if eof else [])


def plan(sim, tmp_path, ms, call, cap, member_cap, want):
    tab = tmp_path / "members.txt"
    tab.write_text("".join("%d %d %d %d\n" % m[:4] for m in ms))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sim, str(tab), str(call), str(cap), str(member_cap), str(want)], capture_output=True, timeout=300, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    lines = p.stdout.decode().split("\n")[:-1]
    fits = lines[0] == "fits 1"
    assert fits or lines == ["fits 0"]
    return fits, [tuple(int(x) for x in l.split()) for l in lines[1:]]


def check_windows(ms, total, wins, call, cap, member_cap, want):
    at = 0
    for k, (start, n, first, end, skip, comp_off, comp_bytes) in enumerate(wins):
        last = k == len(wins) - 1
        assert start == at and n > 0, "the windows tile the stream"
        assert start % call == 0 and (last or n % call == 0)
        L = start + n
        # as many calls as the reader wants, unless the caps cut it short; never beyond the capacity
        assert n <= cap
        goal = min(total, -(-(start + want) // call) * call)
        assert L <= goal
        held = [i for i, m in enumerate(ms) if m[2] and m[4] < L and m[4] + m[2] > start]
        inside = [i for i, m in enumerate(ms) if not m[2] and start < m[4] <= L]
        assert sorted(held + inside) == list(range(first, end)), (k, first, end)
        assert ms[first][2] > 0 and skip == start - ms[first][4] and skip < ms[first][2]
        assert end - first <= member_cap
        assert comp_off == ms[first][0] and comp_bytes == ms[end - 1][0] + ms[end - 1][1] - comp_off and comp_bytes <= cap
        assert ms[end - 1][4] + ms[end - 1][2] - start <= cap
        if L < goal:  # cut short: one more call would not have fitted
            L2 = min(total, L + call) if L % call == 0 else None
            assert L2 is not None
            e2 = max(i for i, m in enumerate(ms) if m[2] and m[4] < L2) + 1
            while e2 < len(ms) and not ms[e2][2] and ms[e2][4] == L2:
                e2 += 1
            if L2 == total:
                e2 = len(ms)
            assert (e2 - first > member_cap or ms[e2 - 1][0] + ms[e2 - 1][1] - comp_off > cap or
                    ms[e2 - 1][4] + ms[e2 - 1][2] - start > cap)
        at = L
    assert at == total
    assert wins[-1][3] == len(ms), "the last window takes every remaining member"


def random_sizes(total, seed):
    rng = random.Random(seed)
    sizes, left = [], total
    while left:
        if rng.random() < 0.1:
            sizes.append(0)
            continue
        s = min(left, rng.choice([1, 17, 1000, 30000, 65280, rng.randint(1, 65536)]))
        sizes.append(s)
        left -= s
    return sizes + [0, 0, 0]


CHAINS = {
    "m65280": lambda: (4_500_000, equal_sizes(4_500_000, 65280)),
    "m30000": lambda: (4_500_000, equal_sizes(4_500_000, 30000)),
    "m1000": lambda: (4_500_000, equal_sizes(4_500_000, 1000)),
    "mixed": lambda: (4_500_000, random_sizes(4_500_000, 7)),
    "one_member": lambda: (5000, [5000]),
    "below_a_call": lambda: (300_000, equal_sizes(300_000, 30000)),
    "three_mib": lambda: (3 * MIB, equal_sizes(3 * MIB, 65280)),
    "member_ends_on_a_call": lambda: (2 * MIB + 70000, equal_sizes(2 * MIB + 70000, 32768)),
}


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    d = tmp_path_factory.mktemp("chains")
    out = {}
    for name, make in CHAINS.items():
        total, sizes = make()
        path = d / (name + ".gz")
        write_chain(path, text_of(total), sizes)
        ms, n = walk(path)
        assert n == total and [m[2] for m in ms] == sizes
        out[name] = (ms, total)
    return out


@pytest.mark.parametrize("name", sorted(CHAINS))
@pytest.mark.parametrize("cap", [4 * MIB, 48 * MIB])
@pytest.mark.parametrize("want", ["4096", "cap"])
def test_windows_tile_the_stream_in_whole_calls(sim, chains, tmp_path, name, cap, want):
    ms, total = chains[name]
    w = 4096 if want == "4096" else cap
    fits, wins = plan(sim, tmp_path, ms, MIB, cap, 8192, w)
    assert fits
    check_windows(ms, total, wins, MIB, cap, 8192, w)
    if name == "member_ends_on_a_call":
        assert any(m[4] + m[2] == MIB for m in ms)
    if w == 4096 and total > MIB:
        assert all(n == MIB for _, n, *_ in wins[:-1])
    if name == "m65280" and w == cap == 4 * MIB:
        # the member that holds the fourth call's last byte ends past the capacity: three calls
        assert wins[0][1] == 3 * MIB


def test_member_cap_cuts_windows_and_small_members_are_unfit(sim, chains, tmp_path):
    ms, total = chains["m1000"]  # 1049 or 1050 members a call
    fits, wins = plan(sim, tmp_path, ms, MIB, 48 * MIB, 2200, 48 * MIB)  # three calls have 3146
    assert fits and [w[1] for w in wins] == [2 * MIB, 2 * MIB, total - 4 * MIB]
    check_windows(ms, total, wins, MIB, 48 * MIB, 2200, 48 * MIB)
    assert plan(sim, tmp_path, ms, MIB, 48 * MIB, 1024, 4096) == (False, [])
    # a capacity of one call: the member that holds a call's last byte ends past it
    assert plan(sim, tmp_path, ms, MIB, MIB, 8192, 4096)[0] is False


def test_chain_of_100_byte_members_is_unfit(sim, tmp_path):
    total = MIB + 5000
    path = tmp_path / "tiny.gz"
    write_chain(path, text_of(total), equal_sizes(total, 100))
    ms, n = walk(path)
    assert n == total
    assert plan(sim, tmp_path, ms, MIB, 48 * MIB, 8192, 4096) == (False, [])


def test_knob_keeps_todays_route_without_the_call(tmp_path):
    """The CPU stand-in engine has no fq_engine_raw_enqueue_bgzf (bound weakly): FQ_GZ_IN_DEVICE=2
    runs today's route, the outputs are the reference's and no member is inflated on a device."""
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    binary = os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool")
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    for name in ("r1.fq.gz", "r2.fq.gz"):
        (inp / name).write_bytes(bgzf(gzip.open(os.path.join(E.INPUTS, name)).read()))
    case = "td_pe_qag"
    argv = [a.replace(E.INPUTS, str(inp)) for a in E.argv_for(binary, case, str(out))]
    p = subprocess.run(argv, capture_output=True, cwd=out, timeout=300, env=dict(os.environ, FQ_GZ_IN_DEVICE="2", FQ_TIMING="1"))
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err[-2000:]
    E.check_outputs(case, str(out))
    assert all(d == 0 for d, _ in device_members(err)), err[-2000:]
    assert "BGZF inputs inflated on the device" not in err
