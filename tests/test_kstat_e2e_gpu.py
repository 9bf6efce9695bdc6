"""--kmer end to end on the GPU: the real `fqtool` binary on every fixture case of
tests/golden/kmer (reference runs, tests/golden/make_kmer.py), -c, -m, UMI and the index filter
included.  Output files, JSON and HTML must be byte-identical to the reference's, or match the
recorded sha256 of the report texts where the fixture keeps only that (k > 5)."""
import subprocess

import pytest

import e2e_util as E
import kmer_util as K
from fqtool_amd import abi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.ok_cases())
def test_fqtool_kmer_matches_reference(case, tmp_path):
    p = subprocess.run(K.argv_for(abi.FQTOOL_BIN, case, str(tmp_path)), capture_output=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    K.check_outputs(case, str(tmp_path))


def test_fqtool_kmer_without_length_is_the_plain_run(tmp_path):
    texts = {}
    for case in ("td_pe_nolen", "td_pe_plain_q"):
        out = tmp_path / case
        out.mkdir()
        p = subprocess.run(K.argv_for(abi.FQTOOL_BIN, case, str(out)), capture_output=True, cwd=out, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        texts[case] = (E.mask_software(open(out / "report.json").read()), E.mask_html(open(out / "report.html").read()))
    assert texts["td_pe_nolen"] == texts["td_pe_plain_q"]


@pytest.mark.parametrize("case", ["td_pe_k5", "synth_pe_correct_umi_merge_k5"])
def test_fqtool_kmer_multi_engine(case, tmp_path):
    """Packs dealt over two engines on one GPU, each with its own tables, which the tool adds up."""
    argv = K.argv_for(abi.FQTOOL_BIN, case, str(tmp_path))
    argv[2] = "4"
    argv += ["--devices", "0,0", "--pack_pairs", "777"]
    p = subprocess.run(argv, capture_output=True, cwd=tmp_path, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert "on 2 engine(s)" in p.stderr.decode()
    K.check_outputs(case, str(tmp_path))
