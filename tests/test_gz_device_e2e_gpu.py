"""The tool with FQ_GZ_DEVICE=1: .gz outputs whose members the GPU compressed.

Golden cases run with their outputs named .gz (those that are not already), at several -z levels
and on two engines; the inflated outputs and the reports must equal the reference's for the plain
names, every file must be a valid BGZF chain, and the members of the pair outputs must carry XFL 4
(the device's mark).  Without the variable the same runs have XFL 0 throughout: the default is the
host's compression.  One round trip feeds device-written files back as inputs."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import e2e_util as E
from fqtool_amd import abi

pytestmark = pytest.mark.gpu

PE_CASES = ("td_pe_qag", "synth_pe_c3", "td_pe_gz")
CASES = PE_CASES + ("td_se_all",)
VARIANTS = {"z1": ["-z", "1"], "z3": ["-z", "3"], "z9": ["-z", "9"], "two_engines": ["--devices", "0,0"]}


def members(path):
    """XFL of every member along the BGZF chain of a file (each member inflates on its own)."""
    data = open(path, "rb").read()
    pos, xfl = 0, []
    while pos < len(data):
        h = data[pos:pos + 18]
        assert h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00", (path, pos, h)
        size = struct.unpack("<H", h[16:18])[0] + 1
        d = zlib.decompressobj(31)
        plain = d.decompress(data[pos:pos + size])
        assert d.eof and d.unused_data == b"", (path, pos)
        assert len(plain) <= 65280 and len(plain) == struct.unpack("<I", data[pos + size - 4:pos + size])[0], (path, pos)
        xfl.append(h[8])
        pos += size
    assert pos == len(data)
    return xfl


def run_tool(case, outdir, extra, device_gz):
    """Runs the case with every plain output renamed .gz; returns {golden name: file written}."""
    os.makedirs(outdir)
    argv = E.argv_for(abi.FQTOOL_BIN, case, outdir)
    names = {}
    for name in E.manifest()[case]["outputs"]:
        path = os.path.join(outdir, name)
        names[name] = path if name.endswith(".gz") else path + ".gz"
        argv = [names[name] if a == path else a for a in argv]
    if "-z" in extra and "-z" in argv:  # (one -z: the variant's)
        k = argv.index("-z")
        del argv[k:k + 2]
    env = dict(os.environ)
    env.pop("FQ_GZ_DEVICE", None)
    if device_gz:
        env["FQ_GZ_DEVICE"] = "1"
    p = subprocess.run(argv + extra, capture_output=True, cwd=outdir, timeout=300, env=env)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return names


def check_against_golden(case, outdir, names, view):
    """check_outputs on a copy of the run in which the renamed outputs are inflated to their plain names."""
    os.makedirs(view)
    for name, path in names.items():
        if name.endswith(".gz"):
            shutil.copy(path, os.path.join(view, name))
        else:
            with open(os.path.join(view, name), "wb") as f:
                f.write(gzip.decompress(open(path, "rb").read()))
    for rep in ("report.json", "report.html"):
        shutil.copy(os.path.join(outdir, rep), os.path.join(view, rep))
    assert sorted(n for n in os.listdir(outdir) if not n.startswith("report.")) == sorted(
        os.path.basename(p) for p in names.values())
    E.check_outputs(case, view)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("case", CASES)
def test_device_gz_outputs_match_reference(case, variant, tmp_path):
    on = run_tool(case, str(tmp_path / "on"), VARIANTS[variant], True)
    check_against_golden(case, str(tmp_path / "on"), on, str(tmp_path / "on_view"))
    for name, path in on.items():
        xfl = members(path)
        assert set(xfl) <= {0, 4}
        if case in PE_CASES:
            assert 4 in xfl, "%s: no member written by the device" % name
    # the default is unchanged: host compression, XFL 0 in every member
    off = run_tool(case, str(tmp_path / "off"), VARIANTS[variant], False)
    check_against_golden(case, str(tmp_path / "off"), off, str(tmp_path / "off_view"))
    for path in off.values():
        assert set(members(path)) == {0}


def test_device_written_files_read_back(tmp_path):
    """Device-written o1 / o2 as inputs give what their inflated copies give."""
    first = run_tool("td_pe_qag", str(tmp_path / "first"), [], True)
    gz = [first["o1.fq"], first["o2.fq"]]
    assert all(4 in members(p) for p in gz)
    plain = []
    for p in gz:
        q = p[:-3]
        with open(q, "wb") as f:
            f.write(gzip.decompress(open(p, "rb").read()))
        plain.append(q)
    got = {}
    for tag, ins in (("gz", gz), ("plain", plain)):
        outd = tmp_path / tag
        outd.mkdir()
        argv = [abi.FQTOOL_BIN, "-w", "1", "-i", ins[0], "-I", ins[1], "-o", str(outd / "o1.fq"), "-O", str(outd / "o2.fq"),
                "-J", str(outd / "report.json"), "-H", str(outd / "report.html"), "-q", "-a", "-g"]
        p = subprocess.run(argv, capture_output=True, cwd=outd, timeout=300, env=dict(os.environ, FQ_GZ_DEVICE="1"))
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        got[tag] = (E.digest(str(outd / "o1.fq")), E.digest(str(outd / "o2.fq")),
                    E.mask_software(open(outd / "report.json").read()))
    assert got["gz"][0]["lines"] > 0
    assert got["gz"] == got["plain"]
