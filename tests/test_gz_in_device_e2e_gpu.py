"""The tool with FQ_GZ_IN_DEVICE=1: BGZF inputs inflated on the GPU give the reference's outputs and
JSON, the FQ_TIMING log shows which side inflated how many members, corrupt inputs end exactly where
they end on the host path (same outputs, exit status and message), and the .gz outputs the device
compressor writes (FQ_GZ_DEVICE=1) read back like their inflated copies."""
import gzip
import os
import re
import subprocess

import pytest

import e2e_util as E
from fqtool_amd import abi
from test_host_e2e import bgzf

pytestmark = pytest.mark.gpu


def device_members(stderr):
    """[(device, host)] member counts of the tool's FQ_TIMING log, one entry per BGZF input."""
    return [(int(a), int(b)) for a, b in re.findall(r"bgzf input [^\n]*?: (\d+) members inflated on the device, (\d+) on the host",
                                                     stderr)]


def recompressed(case, inp, out, member):
    """The case's argv with its .gz inputs recompressed as BGZF into inp."""
    argv = E.argv_for(abi.FQTOOL_BIN, case, str(out))
    n = 0
    for k, a in enumerate(argv):
        if a.startswith(E.INPUTS) and a.endswith(".gz"):
            dst = inp / os.path.basename(a)
            dst.write_bytes(bgzf(gzip.open(a).read(), member=member))
            argv[k] = str(dst)
            n += 1
    return argv, n


def run(argv, cwd, **env):
    p = subprocess.run(argv, capture_output=True, cwd=cwd, timeout=300, env=dict(os.environ, **env))
    return p.returncode, p.stderr.decode(errors="replace")


@pytest.mark.parametrize("batches", ["one_batch", "small_batches"])
@pytest.mark.parametrize("case", ["td_pe_qag", "td_se_q", "td_pe_gz"])
def test_bgzf_inputs_inflated_on_the_device(case, batches, tmp_path):
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    argv, n_in = recompressed(case, inp, out, 0xFF00 if batches == "one_batch" else 30_000)
    env = {"FQ_GZ_IN_DEVICE": "1", "FQ_TIMING": "1"}
    if batches == "small_batches":
        env["FQ_BGZF_BATCH"] = "262144"
    rc, err = run(argv, out, **env)
    assert rc == 0, err[-2000:]
    E.check_outputs(case, str(out))
    counts = device_members(err)
    assert len(counts) == n_in and all(d > 0 and h == 0 for d, h in counts), err[-2000:]


def test_default_keeps_the_host_path(tmp_path):
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    argv, n_in = recompressed("td_pe_qag", inp, out, 0xFF00)
    rc, err = run(argv, out, FQ_TIMING="1")
    assert rc == 0, err[-2000:]
    E.check_outputs("td_pe_qag", str(out))
    counts = device_members(err)
    assert len(counts) == n_in and all(d == 0 and h > 0 for d, h in counts), err[-2000:]


@pytest.mark.parametrize("kind", ["bgzf", "bgzf_small_batches", "multi"])
def test_corrupt_member_ends_the_stream_as_on_the_host(kind, tmp_path):
    """The three corruptions of test_host_e2e.test_corrupt_member_keeps_the_good_prefix (a CRC32
    flipped in member 40 of read 1): with the variable set the tool gives the same outputs, exit status
    and message as without it."""
    member, bad = 0xFF00, 40
    env = {}
    if kind == "bgzf_small_batches":
        env["FQ_BGZF_BATCH"] = str(1 << 18)
    gz = tmp_path / "gz"
    gz.mkdir()
    for name in ("r1.fq.gz", "r2.fq.gz"):
        data = gzip.open(os.path.join(E.INPUTS, name)).read()
        if kind == "multi":
            parts = [gzip.compress(data[o:o + member], 6) for o in range(0, len(data), member)]
            comp = bytearray(b"".join(parts))
            end = sum(len(p) for p in parts[:bad + 1])
        else:
            comp = bytearray(bgzf(data, member=member))
            end = 0
            for _ in range(bad + 1):
                end += int.from_bytes(comp[end + 16:end + 18], "little") + 1
        if name == "r1.fq.gz":
            comp[end - 8] ^= 0x5A  # the member's CRC32
        (gz / name).write_bytes(bytes(comp))
    results = {}
    for mode in ("host", "device"):
        out = tmp_path / mode
        out.mkdir()
        argv = [a.replace(E.INPUTS, str(gz)) for a in E.argv_for(abi.FQTOOL_BIN, "td_pe_qag", str(out))]
        rc, err = run(argv, out, FQ_TIMING="1", **(dict(env, FQ_GZ_IN_DEVICE="1") if mode == "device" else env))
        digests = {n: E.digest(str(out / n)) for n in sorted(os.listdir(out)) if not n.startswith("report.")}
        message = [l for l in err.splitlines() if "rror" in l]
        results[mode] = (rc, message, digests, (out / "report.json").read_text() if (out / "report.json").exists() else None)
        counts = device_members(err)
        if mode == "device" and kind != "multi":
            # read 2 is good: all on the device; read 1's bad batch went to the host
            assert any(h > 0 for d, h in counts) and any(d > 0 and h == 0 for d, h in counts), err[-2000:]
    assert results["host"][1], "the corruption must be reported"
    assert results["host"][:3] == results["device"][:3]
    assert E.mask_software(results["host"][3] or "") == E.mask_software(results["device"][3] or "")


def test_device_written_outputs_read_back(tmp_path):
    first, plain, back_gz, back_plain = (tmp_path / d for d in ("first", "plain", "back_gz", "back_plain"))
    for d in (first, plain, back_gz, back_plain):
        d.mkdir()
    rc, err = run(E.argv_for(abi.FQTOOL_BIN, "td_pe_gz", str(first)), first, FQ_GZ_DEVICE="1")
    assert rc == 0, err[-2000:]
    E.check_outputs("td_pe_gz", str(first))
    for name in ("o1.fq.gz", "o2.fq.gz"):
        data = (first / name).read_bytes()
        assert data[8] == 4, "XFL 4 marks a member the device wrote"
        (plain / name[:-3]).write_bytes(gzip.decompress(data))

    def argv_for(src, suffix, out):
        return [abi.FQTOOL_BIN, "-w", "1", "-J", str(out / "report.json"), "-H", str(out / "report.html"),
                "-i", str(src / ("o1.fq" + suffix)), "-I", str(src / ("o2.fq" + suffix)),
                "-o", str(out / "b1.fq"), "-O", str(out / "b2.fq"), "-q", "-a"]

    rc, err = run(argv_for(first, ".gz", back_gz), back_gz, FQ_GZ_IN_DEVICE="1", FQ_TIMING="1")
    assert rc == 0, err[-2000:]
    counts = device_members(err)
    assert len(counts) == 2 and all(d > 0 and h == 0 for d, h in counts), err[-2000:]
    rc, err = run(argv_for(plain, "", back_plain), back_plain)
    assert rc == 0, err[-2000:]
    for name in ("b1.fq", "b2.fq"):
        assert E.digest(str(back_gz / name)) == E.digest(str(back_plain / name)), name
        assert E.digest(str(back_gz / name))["lines"] > 0
    for k in ("summary", "filtering_result", "adapter_cutting"):
        import json
        assert json.loads((back_gz / "report.json").read_text()).get(k) == json.loads((back_plain / "report.json").read_text()).get(k), k
