"""The tool with FQ_GZ_DEVICE=1 on routed runs (-c, --failed_out, --unpaired_read1/2, -m
--discard_unmerged, -u): every output stream's .gz members compressed on the GPU.

Golden cases run with every plain output renamed .gz, through the raw stream (plain inputs, one
engine, many small windows) and as text packs on two engines.  The inflated outputs and the reports
must equal the reference's, every file must be a valid BGZF chain, every non-empty output must hold a
member the device wrote (XFL 4), and the closing log line must name the route.  Without the variable,
or with one open stream left plain, every member is the host's (XFL 0)."""
import gzip
import os
import shutil
import subprocess

import pytest

import e2e_util as E
from fqtool_amd import abi
from test_gz_device_e2e_gpu import members

pytestmark = pytest.mark.gpu

# -c + failed; failed + unpaired1/2; -m --discard_unmerged; UMI (read 1) + failed; single end + failed
CASES = ("td_pe_correct", "td_pe_all", "td_pe_merge_discard", "td_pe_umi_r1", "td_se_all")
VARIANTS = ("raw_stream", "two_engines")


def run_tool(case, tmp_path, tag, variant, device_gz, keep_plain=()):
    """Runs the case with every plain output (but those in keep_plain) renamed .gz; returns
    ({golden name: file written}, the closing log line, the output directory)."""
    outd = tmp_path / tag
    outd.mkdir()
    argv = E.argv_for(abi.FQTOOL_BIN, case, str(outd))
    names = {}
    for name in E.manifest()[case]["outputs"]:
        path = os.path.join(str(outd), name)
        names[name] = path if name.endswith(".gz") or name in keep_plain else path + ".gz"
        argv = [names[name] if a == path else a for a in argv]
    env = dict(os.environ)
    env.pop("FQ_GZ_DEVICE", None)
    if device_gz:
        env["FQ_GZ_DEVICE"] = "1"
    if variant == "raw_stream":  # plain input files on one engine, 4 KiB first window, 500-pair packs
        ind = tmp_path / (tag + "_in")
        ind.mkdir()
        for k, a in enumerate(argv):
            if a.startswith(E.INPUTS) and a.endswith(".fq.gz"):
                plain = ind / os.path.basename(a)[:-3]
                with gzip.open(a, "rb") as f, open(plain, "wb") as g:
                    shutil.copyfileobj(f, g)
                argv[k] = str(plain)
        argv += ["--pack_pairs", "500"]
        env["FQ_RAW_WINDOW0"] = "4096"
    else:
        argv += ["--devices", "0,0"]
    p = subprocess.run(argv, capture_output=True, cwd=outd, timeout=300, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err[-2000:]
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1, err[-2000:]
    want = "(raw stream" if variant == "raw_stream" else "(text packs"
    assert want in closing[0] and "routed egress of" in closing[0], closing[0]
    return names, closing[0], str(outd)


def check_against_golden(case, outdir, names, view):
    """check_outputs on a copy of the run in which the renamed outputs are inflated to their plain names."""
    os.makedirs(view)
    for name, path in names.items():
        if path.endswith(".gz") and not name.endswith(".gz"):
            with open(os.path.join(view, name), "wb") as f:
                f.write(gzip.decompress(open(path, "rb").read()))
        else:
            shutil.copy(path, os.path.join(view, name))
    for rep in ("report.json", "report.html"):
        shutil.copy(os.path.join(outdir, rep), os.path.join(view, rep))
    assert sorted(n for n in os.listdir(outdir) if not n.startswith("report.")) == sorted(
        os.path.basename(p) for p in names.values())
    E.check_outputs(case, view)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES)
def test_routed_device_gz_outputs_match_reference(case, variant, tmp_path):
    names, closing, outd = run_tool(case, tmp_path, "on", variant, True)
    assert closing.endswith("; device BGZF"), closing
    check_against_golden(case, outd, names, str(tmp_path / "on_view"))
    golden = E.manifest()[case]["outputs"]
    assert len(names) >= 2
    for name, path in names.items():
        xfl = members(path)  # (asserts a valid chain, every member's ISIZE <= 65280)
        assert set(xfl) <= {0, 4}, name
        if golden[name]["lines"] > 0:
            assert 4 in xfl, "%s: no member written by the device" % name
    assert any(golden[name]["lines"] > 0 for name in names)


@pytest.mark.parametrize("case", CASES)
def test_default_and_mixed_outputs_keep_host_compression(case, tmp_path):
    """Without the variable, and with it but one open stream named without .gz (the engine's switch
    covers all streams or none): outputs equal the reference's, every member is the host's."""
    off, closing, outd = run_tool(case, tmp_path, "off", "raw_stream", False)
    assert "device BGZF" not in closing
    check_against_golden(case, outd, off, str(tmp_path / "off_view"))
    for path in off.values():
        assert set(members(path)) <= {0}
    last = sorted(off)[-1]  # (one stream stays plain; a case has at least two outputs)
    mixed, closing, outd = run_tool(case, tmp_path, "mixed", "raw_stream", True, keep_plain=(last,))
    assert "device BGZF" not in closing
    check_against_golden(case, outd, mixed, str(tmp_path / "mixed_view"))
    assert not mixed[last].endswith(".gz")
    for name, path in mixed.items():
        if name != last:
            assert set(members(path)) <= {0}, name
