"""The multi-span BGZF compressor's index arithmetic and its two walks (fqtool_amd/csrc/deflate_core.h:
fq_defl_spans_layout / fq_defl_spans_place, fq_deflate_spans_walk, fq_compact_spans_walk), compiled
for the host by tools/micro/deflate_sim.cpp's span mode and run under AddressSanitizer and UBSan as a
stand-alone program: 256 threads and a barrier stand in for the workgroup, and every span's buffer
is a heap block of exactly fq_deflate_bound(capacity) bytes, so a write past any buffer is caught.
Each span's stream must be a chain of members (XFL 4, ISIZE <= 65280) that inflates to its text."""
import os
import random
import struct
import subprocess
import zlib

import pytest

from fqtool_amd import abi

SIM_SRC = os.path.join(abi.REPO_DIR, "tools", "micro", "deflate_sim.cpp")
IN = 65280


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    """The simulation built by the compile line in its own header."""
    head = open(SIM_SRC).read().split("#include")[0]
    line = next(l for l in head.splitlines() if "g++ " in l)
    argv = line[line.index("g++"):].split()
    assert argv[:6] == ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread"]
    binary = str(tmp_path_factory.mktemp("sim") / "deflate_sim")
    argv[argv.index("-o") + 1] = binary
    subprocess.run(argv, check=True, cwd=abi.REPO_DIR)
    return binary


def fastq_like(n, seed):
    """n bytes that compress like FASTQ text (names with a counter, bases, quality runs)."""
    rng = random.Random(seed)
    out, i = bytearray(), 0
    while len(out) < n:
        length = rng.randint(30, 150)
        out += b"@read%d/1\n" % i + bytes(rng.choice(b"ACGT") for _ in range(length)) + b"\n+\n"
        out += bytes(rng.choice(b"FFFFF:,#") for _ in range(length)) + b"\n"
        i += 1
    return bytes(out[:n])


def bound(cap):
    return cap + 31 * ((cap + IN - 1) // IN)


def inflate_chain(data):
    pos, parts = 0, []
    while pos < len(data):
        h = data[pos:pos + 18]
        assert h[:4] == b"\x1f\x8b\x08\x04" and h[8] == 4 and h[10:16] == b"\x06\x00BC\x02\x00", (pos, h)
        size = struct.unpack("<H", h[16:18])[0] + 1
        d = zlib.decompressobj(31)
        plain = d.decompress(data[pos:pos + size])
        assert d.eof and d.unused_data == b""
        assert 0 < len(plain) <= IN
        parts.append(plain)
        pos += size
    assert pos == len(data)
    return parts


def run_spans(sim, tmp_path, tag, spans, members, level=6):
    """spans: up to six of None (no span) or (text bytes, length word, capacity).  Returns (each span's
    stream, the overflow flag)."""
    args = []
    for k, sp in enumerate(spans):
        if sp is None:
            args.append("-")
            continue
        text, word, cap = sp
        path = tmp_path / ("%s.%d.txt" % (tag, k))
        path.write_bytes(text)
        args.append("%s:%d:%d" % (path, word, cap))
    out = str(tmp_path / (tag + ".out"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sim, "--spans", str(level), str(members), out] + args, capture_output=True, timeout=600, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-3000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == 7 and lines[6] in ("overflow 0", "overflow 1"), lines
    streams = []
    for k in range(6):
        name, idx, total = lines[k].split()
        assert name == "span" and int(idx) == k
        data = open("%s.%d" % (out, k), "rb").read()
        assert len(data) == int(total)
        streams.append(data)
    return streams, lines[6] == "overflow 1"


def check(streams, spans):
    """Every span's stream inflates to its text (clamped to its capacity), member by member."""
    spans = list(spans) + [None] * (6 - len(spans))
    for k, sp in enumerate(spans):
        want = b"" if sp is None else sp[0][:min(sp[1], sp[2])]
        parts = inflate_chain(streams[k])
        assert b"".join(parts) == want, "span %d" % k
        assert [len(x) for x in parts] == [min(IN, len(want) - at) for at in range(0, len(want), IN)], "span %d" % k
        assert len(streams[k]) <= bound(len(want))


def span(n, seed, word=None, cap=None):
    return (fastq_like(n, seed), n if word is None else word, n if cap is None else cap)


def test_all_spans_empty(sim, tmp_path):
    spans = [span(0, k) for k in range(6)]
    streams, over = run_spans(sim, tmp_path, "empty", spans, 4)
    assert not over and streams == [b""] * 6
    streams, over = run_spans(sim, tmp_path, "absent", [None] * 6, 4)
    assert not over and streams == [b""] * 6


def test_one_byte_between_empty_spans(sim, tmp_path):
    spans = [span(0, 1), None, span(1, 2, cap=100), span(0, 3, cap=50), None, span(0, 4)]
    streams, over = run_spans(sim, tmp_path, "one", spans, 1)
    assert not over
    check(streams, spans)
    assert len(streams[2]) > 0


def test_member_boundaries(sim, tmp_path):
    """Exactly one member, one byte more, exactly two members: scratch of exactly their five members."""
    spans = [span(IN, 1), span(IN + 1, 2), span(2 * IN, 3)]
    streams, over = run_spans(sim, tmp_path, "edges", spans, 5)
    assert not over
    check(streams, spans)
    assert [len(inflate_chain(s)) for s in streams[:3]] == [1, 2, 2]


@pytest.mark.parametrize("level", [1, 6])
def test_six_mixed_spans(sim, tmp_path, level):
    """Sizes as a routed pack's: two streams of several members, short ones and an empty one; an
    incompressible span is stored (its members grow by their 31 bytes of framing)."""
    noise = random.Random(9).randbytes(70000)
    spans = [span(200000, 1), span(190001, 2), span(0, 3, cap=400000), span(777, 4, cap=200000), (noise, 70000, 70000),
             span(65279, 6, cap=400000)]
    streams, over = run_spans(sim, tmp_path, "mixed%d" % level, spans, 4 + 3 + 1 + 2 + 1, level)
    assert not over
    check(streams, spans)
    assert len(streams[4]) > 70000 and len(streams[0]) < 100000


def test_length_word_above_the_capacity_is_clamped(sim, tmp_path):
    spans = [span(70000, 1, word=1 << 40, cap=66000), span(5000, 2, word=5001, cap=5000)]
    streams, over = run_spans(sim, tmp_path, "clamp", spans, 3)
    assert not over
    check(streams, spans)
    assert sum(len(x) for x in inflate_chain(streams[0])) == 66000


def test_members_beyond_the_scratch_are_reported(sim, tmp_path):
    """Five members, four slots: the overflow is reported, every total is 0 and (the sanitizer's
    verdict) nothing is written past a slot or a buffer."""
    spans = [span(IN, 1), span(IN + 1, 2), span(2 * IN, 3)]
    streams, over = run_spans(sim, tmp_path, "over", spans, 4)
    assert over and streams == [b""] * 6
