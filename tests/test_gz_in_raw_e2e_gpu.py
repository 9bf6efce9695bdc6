"""The tool with FQ_GZ_IN_DEVICE=2: BGZF inputs go through the raw stream, each window's members
inflated on the device into the window's place (fq_engine_raw_enqueue_bgzf).  The golden cases give
the reference's outputs and reports byte for byte over five windows with carries across them, the
closing log line names the route, inputs the route does not take keep today's, and corrupt inputs
end exactly as on the host path: same outputs, exit status, messages and JSON."""
import gzip
import os
import re
import subprocess

import pytest

import e2e_util as E
from fqtool_amd import abi
from test_gz_in_device_e2e_gpu import device_members, recompressed
from test_host_e2e import bgzf

pytestmark = pytest.mark.gpu

CASES = ["td_pe_qag", "td_se_q", "td_pe_gz", "td_pe_merge", "td_pe_merge_discard", "td_pe_correct", "td_pe_umi_idx1",
         "td_pe_index", "td_pe_split_num", "td_pe_dup"]
ROUTE = re.compile(r"BGZF inputs inflated on the device: (\d+) members")


def run(argv, cwd, **env):
    base = {k: v for k, v in os.environ.items() if k not in ("FQ_GZ_IN_DEVICE", "FQ_GZ_DEVICE")}
    p = subprocess.run(argv, capture_output=True, cwd=cwd, timeout=300, env=dict(base, **env))
    return p.returncode, p.stderr.decode(errors="replace")


def closing_line(err):
    lines = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(lines) == 1, err[-2000:]
    return lines[0]


SMALL = {"FQ_TIMING": "1", "FQ_RAW_WINDOW0": "4096"}  # with --pack_pairs 500: a pack per 1 MiB window at first


def dirs(tmp_path, *names):
    out = [tmp_path / n for n in names]
    for d in out:
        d.mkdir()
    return out


@pytest.mark.parametrize("member", [0xFF00, 30000])
@pytest.mark.parametrize("case", CASES)
def test_golden_cases_through_the_route(case, member, tmp_path):
    inp, out = dirs(tmp_path, "in", "out")
    argv, n_in = recompressed(case, inp, out, member)
    rc, err = run(argv + ["--pack_pairs", "500"], out, FQ_GZ_IN_DEVICE="2", **SMALL)
    assert rc == 0, err[-2000:]
    E.check_outputs(case, str(out))
    line = closing_line(err)
    assert "(raw stream" in line and "ended: end of input" in line, line
    sent = ROUTE.search(line)
    assert sent and int(sent.group(1)) > 0, line
    # 4.5 MB of text per input: five windows of whole 1 MiB reads, the member at each cut sent twice
    # (no multiple of either member size below 5 MB is a multiple of 1 MiB)
    want = 0
    for a in argv:
        if a.startswith(str(inp)):
            size = len(gzip.open(a).read())
            assert 4 << 20 < size < 5 << 20
            want += -(-size // member) + 1 + 4
    assert int(sent.group(1)) == want, line
    counts = device_members(err)
    assert len(counts) == n_in and all(d > 0 and h == 0 for d, h in counts), err[-2000:]


def test_device_in_and_out(tmp_path):
    inp, out = dirs(tmp_path, "in", "out")
    argv, _ = recompressed("td_pe_gz", inp, out, 0xFF00)
    rc, err = run(argv + ["--pack_pairs", "500"], out, FQ_GZ_IN_DEVICE="2", FQ_GZ_DEVICE="1", **SMALL)
    assert rc == 0, err[-2000:]
    E.check_outputs("td_pe_gz", str(out))
    line = closing_line(err)
    assert ROUTE.search(line) and "; device BGZF" in line, line
    assert (out / "o1.fq.gz").read_bytes()[8] == 4, "XFL 4 marks a member the device wrote"


@pytest.mark.parametrize("value", [None, "1"])
def test_other_values_keep_their_routes(value, tmp_path):
    inp, out = dirs(tmp_path, "in", "out")
    argv, _ = recompressed("td_pe_qag", inp, out, 0xFF00)
    rc, err = run(argv, out, FQ_TIMING="1", **({"FQ_GZ_IN_DEVICE": value} if value else {}))
    assert rc == 0, err[-2000:]
    E.check_outputs("td_pe_qag", str(out))
    line = closing_line(err)
    assert not ROUTE.search(line) and "(raw stream" not in line, line


@pytest.mark.parametrize("kind", ["one_mate_plain_gzip", "members_of_100_bytes"])
def test_inputs_the_route_does_not_take(kind, tmp_path):
    inp, out = dirs(tmp_path, "in", "out")
    argv = E.argv_for(abi.FQTOOL_BIN, "td_pe_qag", str(out))
    for k, a in enumerate(argv):
        if a.startswith(E.INPUTS) and a.endswith(".gz"):
            if kind == "one_mate_plain_gzip" and a.endswith("r2.fq.gz"):
                continue  # (the golden input: one gzip member)
            dst = inp / os.path.basename(a)
            dst.write_bytes(bgzf(gzip.open(a).read(), level=1, member=0xFF00 if kind == "one_mate_plain_gzip" else 100))
            argv[k] = str(dst)
    rc, err = run(argv, out, FQ_GZ_IN_DEVICE="2", FQ_TIMING="1")
    assert rc == 0, err[-2000:]
    E.check_outputs("td_pe_qag", str(out))
    assert not ROUTE.search(closing_line(err))
    assert all(d == 0 for d, _ in device_members(err)), err[-2000:]


@pytest.fixture(scope="module")
def golden_bgzf():
    """Both inputs of td_pe_qag as BGZF members of 0xFF00 bytes, and each member's end in the file."""
    out = {}
    for name in ("r1.fq.gz", "r2.fq.gz"):
        comp = bgzf(gzip.open(os.path.join(E.INPUTS, name)).read(), member=0xFF00)
        ends, at = [], 0
        while at < len(comp):
            at += int.from_bytes(comp[at + 16:at + 18], "little") + 1
            ends.append(at)
        out[name] = (comp, ends)
    return out


# read 1: the first member, the one that straddles the first 1 MiB read (16 * 65280 < 2^20 < 17 * 65280),
# the one after it, one in the middle, the last with data; read 2: one in the middle
WHERE = [("r1.fq.gz", 0), ("r1.fq.gz", 16), ("r1.fq.gz", 17), ("r1.fq.gz", 40), ("r1.fq.gz", "last"), ("r2.fq.gz", 40)]


@pytest.mark.parametrize("what", ["crc", "payload", "isize"])
@pytest.mark.parametrize("where", WHERE, ids=["%s-%s" % (w[0][:2], w[1]) for w in WHERE])
def test_corrupt_member_ends_the_run_as_on_the_host(what, where, golden_bgzf, tmp_path):
    (gz,) = dirs(tmp_path, "gz")
    for name, (comp, ends) in golden_bgzf.items():
        comp = bytearray(comp)
        if name == where[0]:
            k = len(ends) - 2 if where[1] == "last" else where[1]  # (the last member is the empty EOF one)
            start, end = (ends[k - 1] if k else 0), ends[k]
            if what == "crc":
                comp[end - 8] ^= 0x5A
            elif what == "isize":
                comp[end - 4] ^= 0x01
            else:
                comp[start + 18 + (end - start - 26) // 2] ^= 0x5A
        (gz / name).write_bytes(bytes(comp))
    results = {}
    for mode in ("host", "device"):
        (out,) = dirs(tmp_path, mode)
        argv = [a.replace(E.INPUTS, str(gz)) for a in E.argv_for(abi.FQTOOL_BIN, "td_pe_qag", str(out))]
        env = dict(SMALL, FQ_GZ_IN_DEVICE="2") if mode == "device" else {"FQ_TIMING": "1"}
        rc, err = run(argv + ["--pack_pairs", "500"], out, **env)
        digests = {n: E.digest(str(out / n)) for n in sorted(os.listdir(out)) if not n.startswith("report.")}
        message = [l for l in err.splitlines() if "rror" in l]
        results[mode] = (rc, message, digests, (out / "report.json").read_text() if (out / "report.json").exists() else None)
        if mode == "device" and rc == 0:
            assert ROUTE.search(closing_line(err)), err[-2000:]
    assert results["host"][1], "the corruption must be reported"
    assert results["host"][:3] == results["device"][:3]
    assert E.mask_software(results["host"][3] or "") == E.mask_software(results["device"][3] or "")
