"""--kmer on the CPU: the numpy model of the counting (tests/kmer_util.py) pinned to the reference's
reports (tests/golden/kmer, made by tests/golden/make_kmer.py), the host side (options, session
API, JSON and HTML reports) with the CPU oracle as the engine and the model's tables handed in,
the CLI's behaviour, and the kernels' per-read routine (fqtool_amd/csrc/kstat_core.h) run on the
host by tools/micro/kstat_sim.cpp against the model."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import e2e_util as E
import kmer_util as K
from batch_util import config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi

# the fixture cases whose post-filter reads are the output files' reads one for one: no -m (a merged
# read is not in o1 / o2) and no -c; not the interleaved case either (the reference, given -o alone
# for pairs, leaves it empty)
FILE_CASES = ["td_pe_k5", "td_pe_k6", "td_se_k8", "td_pe_index_k4"]
KMER_CASES = [c for c in K.ok_cases() if K.manifest()[c]["k"]]


@pytest.fixture(scope="module")
def host(oracle):
    if not (os.path.exists(abi.HOST_LIB) and os.path.exists(abi.FQTOOL_BIN)):
        subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "host"], check=True)
    lib = abi.load_host()
    backend = E.oracle_kmer_backend(oracle)
    lib.fqh_set_kmer_backend(ctypes.addressof(backend))
    yield lib
    lib.fqh_set_kmer_backend(None)


def case_inputs(case):
    """(read-1 sequences, read-2 sequences or None) of a fixture case's input."""
    args = K.manifest()[case]["args"].format(**{"in": E.INPUTS, "out": "/nowhere"}).split()
    in1 = args[args.index("-i") + 1]
    if "--in_fq_interleaved" in args:
        s = K.fastq_seqs(in1)
        return s[0::2], s[1::2]
    return K.fastq_seqs(in1), (K.fastq_seqs(args[args.index("-I") + 1]) if "-I" in args else None)


@pytest.fixture(scope="module")
def sessions(host, oracle, tmp_path_factory):
    """case -> (output directory, the model's tables) of one session run: the oracle as the engine,
    the model counting each pack from its batch and the oracle's records, its tables handed in."""
    cache = {}

    def get(case):
        if case not in cache:
            out = str(tmp_path_factory.mktemp(case))
            _, k, tables = K.run_session_kmer(host, K.argv_for("fqtool", case, out), E.oracle_process(oracle))
            assert k == K.manifest()[case]["k"]
            cache[case] = (out, tables)
        return cache[case]
    return get


@pytest.mark.parametrize("case", [c for c in KMER_CASES if K.manifest()[c]["json"]])
def test_model_pre_tables_match_reference(case):
    """Every fixture with a stored report, -m and -c included: the model on the input files gives
    the reference's Read{1,2}BeforeFiltering.KmerCount."""
    m = K.manifest()[case]
    rep = json.loads(K.golden_text(case, "json"))
    k = m["k"]
    for name, seqs in zip(("Read1BeforeFiltering", "Read2BeforeFiltering"), case_inputs(case)):
        if seqs is None:
            assert name not in rep
            continue
        t = K.Tables(k)
        for s in seqs:
            t.add(0, s)
        want = K.table_from_json(rep[name]["KmerCount"], k)
        assert np.array_equal(t.array()[:4 ** k], want), name
        assert list(rep[name]["KmerCount"]) == sorted(rep[name]["KmerCount"])  # text order, not key order
        assert list(rep[name]).index("KmerCount") == list(rep[name]).index("ContentCurves") + 1


@pytest.mark.parametrize("case", FILE_CASES)
def test_model_post_tables_match_reference(case, sessions):
    """The session's output files equal the reference's; the model run on them gives the fixture's
    Read{1,2}AfterFiltering.KmerCount (where the fixture stores the report) and the tables the model
    built from the packs and the oracle's records."""
    m = K.manifest()[case]
    k = m["k"]
    out, tables = sessions(case)
    K.check_files(case, out)
    tabs = tables.reshape(4, -1)
    rep = json.loads(K.golden_text(case, "json")) if m["json"] else {}
    for table, name, fq in ((2, "Read1AfterFiltering", "o1.fq"), (3, "Read2AfterFiltering", "o2.fq")):
        if fq not in m["outputs"]:
            continue
        t = K.Tables(k)
        for s in K.fastq_seqs(os.path.join(out, fq)):
            t.add(0, s)
        got = t.array()[:4 ** k]
        assert got.sum() > 0
        assert np.array_equal(got, tabs[table]), name
        if rep:
            assert np.array_equal(got, K.table_from_json(rep[name]["KmerCount"], k)), name


@pytest.mark.parametrize("case", KMER_CASES)
def test_host_pipeline_reports_kmer(case, sessions):
    """Options, session API, KmerCount in the JSON and the KMER sections of the HTML: outputs and
    reports byte-identical to the reference's (or to its sha256 for the large k), -m, -c, UMI and the
    index filter included, with the model's tables handed in."""
    out, tables = sessions(case)
    assert tables is not None
    K.check_outputs(case, out)


def test_kmer_without_length_counts_nothing(host, oracle, tmp_path):
    """kmer.kmerLen defaults to 0: the reports are the plain run's."""
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    _, k, tables = K.run_session_kmer(host, K.argv_for("fqtool", "td_pe_nolen", str(a)), E.oracle_process(oracle))
    assert k == 0 and tables is None
    K.check_outputs("td_pe_nolen", str(a))
    K.run_session_kmer(host, K.argv_for("fqtool", "td_pe_plain_q", str(b)), E.oracle_process(oracle))
    K.check_outputs("td_pe_plain_q", str(b))
    assert E.mask_software(K.golden_text("td_pe_nolen", "json")) == E.mask_software(K.golden_text("td_pe_plain_q", "json"))
    assert E.mask_html(K.golden_text("td_pe_nolen", "html")) == E.mask_html(K.golden_text("td_pe_plain_q", "html"))


def run_cli(args, cwd):
    if not os.path.exists(abi.FQTOOL_BIN):
        subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "host"], check=True)
    return subprocess.run([abi.FQTOOL_BIN] + args, capture_output=True, cwd=cwd, timeout=120)


@pytest.mark.parametrize("case", ["err_kmer_needs", "err_kmer_range"])
def test_cli_kmer_errors_match_reference(case, tmp_path):
    m = K.manifest()[case]
    p = subprocess.run(K.argv_for(abi.FQTOOL_BIN, case, str(tmp_path)), capture_output=True, cwd=tmp_path, timeout=120)
    assert p.returncode == m["exit"] and m["exit"] in (105, 107), p.stderr
    assert p.stderr.decode().replace(E.INPUTS, "{in}").replace(str(tmp_path), "{out}") == m["stderr"]


@pytest.mark.parametrize("k", [K.MAX_K + 1, 16])
def test_cli_refuses_lengths_above_the_limit(k, tmp_path):
    """After the reference's own CLI checks and before any input is read or output created."""
    p = run_cli(["-i", os.path.join(E.INPUTS, "r1.fq.gz"), "-o", str(tmp_path / "o.fq"), "--kmer", "--kmer_length", str(k)],
                tmp_path)
    err = p.stderr.decode()
    assert p.returncode not in (0, 105, 107), err
    lines = err.strip().splitlines()  # the message, then the trailer every CLI error carries
    assert len(lines) == 2 and lines[1] == "Run with --help for more information.", err
    assert "limit of %d" % K.MAX_K in lines[0] and "4^k" in lines[0] and "16" in lines[0], err
    assert not os.listdir(tmp_path)


def test_cli_still_refuses_ora(tmp_path):
    p = run_cli(["-i", os.path.join(E.INPUTS, "r1.fq.gz"), "-o", str(tmp_path / "o.fq"), "--ora"], tmp_path)
    assert p.returncode == 2 and b"--ora" in p.stderr
    h = run_cli(["--help"], tmp_path).stdout.decode() + run_cli(["--help"], tmp_path).stderr.decode()
    tagged = [l.split()[0] for l in h.splitlines() if "[not supported by fqtool-amd]" in l]
    assert tagged == ["--ora"], tagged


# ---- the kernels' per-read routine on the host --------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("sim") / "kstat_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", os.path.join(abi.REPO_DIR, "tools", "micro", "kstat_sim.cpp"),
                    "-o", binary], check=True)
    return binary


def sim_tables(sim, tmp_path, pk, p, res, k):
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    K.write_sim_input(inp, pk, p, res, k)
    subprocess.run([sim, inp, out], check=True, timeout=120)
    return np.fromfile(out, np.uint64)


def test_sim_self_check(sim):
    subprocess.run([sim, "--self"], check=True, timeout=120)


@pytest.mark.parametrize("k", [4, 5, K.LDS_MAX_K, K.LDS_MAX_K + 1, K.MAX_K])
@pytest.mark.parametrize("paired", [True, False])
def test_sim_lengths_and_bad_bytes(sim, oracle, tmp_path, k, paired):
    p = config("C3" if paired else "C2", max_cycles=256)
    pk = K.length_pack(k, paired)
    res, _ = run_oracle(oracle, p, pk)
    want = K.model_pack(pk, p, res, k).array()
    assert want.reshape(4, -1)[0].sum() > 0
    assert np.array_equal(sim_tables(sim, tmp_path, pk, p, res, k), want)


@pytest.mark.parametrize("name,stride", [("C3", 160), ("C4", 160), ("PE_merge_discard", 160), ("PE_umi", 160),
                                         ("PE_umi_merge", 160), ("SE_all", 160), ("C4", 320), ("C2", 320)])
def test_sim_pack_variants(sim, oracle, tmp_path, name, stride):
    """SE, PE, -m (merged, unmerged, discarded), UMI front trims, index-filtered pairs, both strides:
    the post tables from the oracle's records."""
    p = config(name, max_cycles=1024)
    paired = bool(p.paired)
    pk = edge_pack(700, paired, stride=stride, seed=3)
    pk.flags = (np.random.default_rng(2).random(pk.n) < 0.15).astype(np.uint8) * abi.FQ_BF_INDEX_FILTERED
    res, _ = run_oracle(oracle, p, pk)
    want = K.model_pack(pk, p, res, 5).array()
    assert np.array_equal(sim_tables(sim, tmp_path, pk, p, res, 5), want)


def test_sim_merged_junction(sim, oracle, tmp_path):
    """Merged reads whose windows over the junction hold an N the complement produced."""
    p = config("C4", max_cycles=512)
    pk = K.junction_pack()
    res, _ = run_oracle(oracle, p, pk)
    merged = (res["flags"][0::2] & abi.FQ_RF_MERGED) != 0
    assert merged.sum() > pk.n // 2 and (res["m_len2"][0::2][merged] > 0).all()
    want = K.model_pack(pk, p, res, 6).array()
    assert np.array_equal(sim_tables(sim, tmp_path, pk, p, res, 6), want)


def test_engine_without_kmer_calls_is_an_error(tmp_path):
    """The tool binds fq_kstat_* weakly.  Against an engine library without them (the CPU stand-in
    of `make cpuhost`) a run with an effective k-mer length stops with a one-line error instead of
    writing reports without the KmerCount sections; --kmer alone (no length) runs as before."""
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    cpu_bin = os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool")
    out = tmp_path / "k5"
    out.mkdir()
    p = subprocess.run(K.argv_for(cpu_bin, "td_pe_k5", str(out)), capture_output=True, cwd=out, timeout=300)
    err = [l for l in p.stderr.decode().splitlines() if l.startswith("ERROR:")]
    assert p.returncode != 0 and len(err) == 1 and "fq_kstat" in err[0], p.stderr.decode()[-2000:]
    assert not os.path.exists(out / "report.json")
    out = tmp_path / "nolen"
    out.mkdir()
    p = subprocess.run(K.argv_for(cpu_bin, "td_pe_nolen", str(out)), capture_output=True, cwd=out, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    K.check_outputs("td_pe_nolen", str(out))
