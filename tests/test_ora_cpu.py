"""--ora on the CPU: the Python model of the reference's overrepresented-sequence analysis
(tests/ora_util.py: hot-set selection and per-read counting) pinned to the reference's reports
(tests/golden/ora, made by tests/golden/make_ora.py), the host side (options, evaluator, session
API, JSON and HTML reports) with the CPU oracle as the engine and the model's blocks handed in, the
CLI's opt-in behaviour, and the kernels' per-read routine (fqtool_amd/csrc/ora_core.h) run on the
host by tools/micro/ora_sim.cpp against the model."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import e2e_util as E
import kmer_util as K
import ora_util as O
from batch_util import config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi

# the fixture cases whose post-filter reads are the output files' reads one for one: no -m (a merged
# read is not in o1 / o2), no -c, no UMI; not the interleaved case either (the reference, given -o
# alone for pairs, leaves it empty)
FILE_CASES = ["td_pe", "td_pe_s1", "ora_pe", "ora_pe_s1", "ora_pe_s7", "ora_pe_s100", "ora_se_s1", "ora_pe_kmer", "ora100_pe"]


@pytest.fixture(scope="module")
def host(oracle):
    if not (os.path.exists(abi.HOST_LIB) and os.path.exists(abi.FQTOOL_BIN)):
        subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "host"], check=True)
    lib = abi.load_host()
    backend = E.oracle_kmer_backend(oracle)
    lib.fqh_set_kmer_backend(ctypes.addressof(backend))
    os.environ["FQ_ORA"] = "1"  # the session parses its command line in this process
    yield lib
    del os.environ["FQ_ORA"]
    lib.fqh_set_kmer_backend(None)


def case_model(case, rep):
    """The model over a fixture's input files: hot sets and evaluated lengths as the pre-pass takes them."""
    in1, in2, inter = O.case_inputs(case)
    r1 = O.file_reads(in1)
    ev1 = max(len(s) for s in r1[:1000])
    ev2 = max(len(s) for s in O.file_reads(in2)[:1000]) if in2 else 151
    return O.Model(O.case_sampling(case), ev1, ev2, O.file_hot_set(in1), O.file_hot_set(in2) if in2 else ())


def listed(section):
    o = section["OverrepresentedSequences"]
    assert o is None or len(o) > 0  # null, never {}
    return {k.encode("latin-1").decode("latin-1"): v for k, v in o.items()} if o else None


@pytest.mark.parametrize("case", O.ok_cases())
def test_model_pre_sections_match_reference(case):
    """Every fixture, -m and -c included: hot sets chosen by the model from the input files and its
    counting of every sampling-th read give the reference's Read{1,2}BeforeFiltering lists."""
    rep = json.loads(O.golden_text(case, "json"))
    in1, in2, inter = O.case_inputs(case)
    model = case_model(case, rep)
    if inter:
        s = O.file_reads(in1)
        streams = (s[0::2], s[1::2])
    else:
        streams = (O.file_reads(in1), O.file_reads(in2) if in2 else None)
    for t, name in ((0, "Read1BeforeFiltering"), (1, "Read2BeforeFiltering")):
        if streams[t] is None:
            assert name not in rep
            continue
        for s in streams[t]:
            model.add(t, s)
        assert model.passing(t) == listed(rep[name]), name
        keys = list(rep[name])
        assert keys.index("OverrepresentedSequences") == keys.index("KmerCount" if "KmerCount" in keys else "ContentCurves") + 1
        if rep[name]["OverrepresentedSequences"]:
            assert list(rep[name]["OverrepresentedSequences"]) == sorted(rep[name]["OverrepresentedSequences"])


def test_fixtures_are_worth_having():
    """The condition tests/golden/make_ora.py checks before it writes: one case lists >= 3 sequences of
    >= 3 lengths in all four Stats, the -m case lists merged reads' hits, one case is null everywhere,
    and at 100 cycles the fifth step (98) lists nothing that the 151-cycle run does not."""
    rep = json.loads(O.golden_text("ora_pe_s1", "json"))
    for name in O.SECTIONS:
        o = rep[name]["OverrepresentedSequences"]
        assert len(o) >= 3 and len({len(k) for k in o}) >= 3, name
    assert json.loads(O.golden_text("ora_pe_merge_s1", "json"))["MergedAndFiltered"]["OverrepresentedSequences"]
    null = json.loads(O.golden_text("synth_pe_null", "json"))
    assert all(null[name]["OverrepresentedSequences"] is None for name in O.SECTIONS)
    short = json.loads(O.golden_text("ora100_pe", "json"))
    assert all(len(k) in (10, 20, 40) for name in O.SECTIONS for k in (short[name]["OverrepresentedSequences"] or {}))


def test_real_data_fixtures():
    """What the reference reports on r1.fq.gz / r2.fq.gz (-q -a -g), whose hot sets have 18,726 and
    16,876 members: at the default sampling a 20-mer and a 100-mer in both pre Stats, 100-mers only
    in post-R2 (two of them) and null in post-R1; at --ora_sample 1 the 100-mer drops out of pre-R1;
    with -m --ora_sample 7 MergedAndFiltered is null."""
    def lens(case, name):
        o = json.loads(O.golden_text(case, "json"))[name]["OverrepresentedSequences"]
        return None if o is None else sorted(len(k) for k in o)
    assert lens("td_pe", "Read1BeforeFiltering") == [20, 100] and lens("td_pe", "Read2BeforeFiltering") == [20, 100]
    assert lens("td_pe", "Read2AfterFiltering") == [100, 100] and lens("td_pe", "Read1AfterFiltering") is None
    assert lens("td_pe_s1", "Read1BeforeFiltering") == [20] and lens("td_pe_s1", "Read2BeforeFiltering") == [20, 100]
    assert lens("td_pe_merge_s7", "MergedAndFiltered") is None
    assert len(O.file_hot_set(os.path.join(E.INPUTS, "r1.fq.gz"))) == 18726
    assert len(O.file_hot_set(os.path.join(E.INPUTS, "r2.fq.gz"))) == 16876


@pytest.fixture(scope="module")
def sessions(host, oracle, tmp_path_factory):
    """case -> (output directory, the session's hot sets, the model) of one session run: the oracle as
    the engine, the model counting each pack from its batch and the oracle's records."""
    cache = {}

    def get(case):
        if case not in cache:
            out = str(tmp_path_factory.mktemp(case))
            _, sets, model = O.run_session_ora(host, O.argv_for("fqtool", case, out), E.oracle_process(oracle))
            cache[case] = (out, sets, model)
        return cache[case]
    return get


@pytest.mark.parametrize("case", O.ok_cases())
def test_evaluator_hot_sets_match_model(case, sessions):
    """Evaluator::computeOverRepSeq of the host against the model's: same sequences, same (map) order;
    an interleaved input's mates all go to the first set."""
    in1, in2, inter = O.case_inputs(case)
    _, sets, _ = sessions(case)
    assert sets[0] == list(O.file_hot_set(in1))
    assert sets[1] == (list(O.file_hot_set(in2)) if in2 else [])


@pytest.mark.parametrize("case", FILE_CASES)
def test_model_post_sections_match_reference(case, sessions):
    """The session's output files equal the reference's; the model run on them (every read that
    reached the post-filter Stats, in order) gives the fixture's Read{1,2}AfterFiltering lists and
    the blocks the model built from the packs and the oracle's records."""
    m = O.manifest()[case]
    out, sets, model = sessions(case)
    O.check_files(case, out)
    rep = json.loads(O.golden_text(case, "json"))
    again = O.Model(model.sampling, model.eval[0], model.eval[1], sets[0], sets[1])
    for table, name, fq in ((2, "Read1AfterFiltering", "o1.fq"), (3, "Read2AfterFiltering", "o2.fq")):
        if fq not in m["outputs"]:
            continue
        for s in K.fastq_seqs(os.path.join(out, fq)):
            again.add(table, s)
        assert np.array_equal(again.rows[table], model.rows[table]), name
        assert again.passing(table) == listed(rep[name]), name


@pytest.mark.parametrize("case", O.ok_cases())
def test_host_pipeline_reports_ora(case, sessions):
    """Options, evaluator, session API, OverrepresentedSequences in the JSON and the ORA sections of
    the HTML: outputs and reports byte-identical to the reference's, -m, -c, UMI, --kmer and the
    interleaved input included, with the model's blocks handed in."""
    out, _, _ = sessions(case)
    O.check_files(case, out)
    O.check_reports(case, out)


def test_session_refuses_blocks_of_the_wrong_size(host, oracle, tmp_path):
    enc = [a.encode() for a in O.argv_for("fqtool", "ora_pe", str(tmp_path))]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    s = ctypes.c_void_p()
    assert host.fqh_session_open(len(enc), arr, ctypes.byref(s)) == 0
    try:
        on, smp, e1, e2, sets = O.session_sets(host, s)
        assert on and smp == O.DEFAULT_SAMPLING and (e1, e2) == (151, 151)
        words = 2 * (len(sets[0]) * (1 + e1) + len(sets[1]) * (1 + e2))
        buf = np.zeros(words + 1, np.uint64)
        assert host.fqh_session_set_ora(s, buf.ctypes.data, words + 1) == -1
        assert host.fqh_session_set_ora(s, buf.ctypes.data, words) == 0
    finally:
        host.fqh_session_close(s)


# ---- the CLI ------------------------------------------------------------------------------------
def run_cli(args, cwd, ora=True, binary=None):
    if not os.path.exists(abi.FQTOOL_BIN):
        subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "host"], check=True)
    env = {k: v for k, v in os.environ.items() if k != "FQ_ORA"}
    if ora:
        env["FQ_ORA"] = "1"
    return subprocess.run([binary or abi.FQTOOL_BIN] + args, capture_output=True, cwd=cwd, timeout=120, env=env)


def test_cli_refuses_without_the_variable(tmp_path):
    """Without FQ_ORA=1 the behaviour is today's: exit 2 naming the flag, the help tag on --ora;
    FQ_ORA=0 is the same."""
    args = ["-i", os.path.join(E.INPUTS, "r1.fq.gz"), "-o", str(tmp_path / "o.fq"), "--ora"]
    p = run_cli(args, tmp_path, ora=False)
    assert p.returncode == 2 and b"--ora" in p.stderr
    h = run_cli(["--help"], tmp_path, ora=False).stdout.decode()
    assert [l.split()[0] for l in h.splitlines() if "[not supported by fqtool-amd]" in l] == ["--ora"]
    env = dict(os.environ, FQ_ORA="0")
    assert subprocess.run([abi.FQTOOL_BIN] + args, capture_output=True, cwd=tmp_path, env=env, timeout=120).returncode == 2
    assert not os.listdir(tmp_path)


def test_cli_help_with_the_variable(tmp_path):
    h0 = run_cli(["--help"], tmp_path, ora=False).stdout.decode()
    h1 = run_cli(["--help"], tmp_path, ora=True).stdout.decode()
    assert "[not supported by fqtool-amd]" not in h1
    assert h1 == h0.replace(" [not supported by fqtool-amd]", "")


@pytest.mark.parametrize("case", O.err_cases())
def test_cli_ora_errors_match_reference(case, tmp_path):
    """--ora_sample keeps the reference's range and `needs` errors, with and without the variable."""
    m = O.manifest()[case]
    for ora in (True, False):
        p = run_cli(O.argv_for("x", case, str(tmp_path))[1:], tmp_path, ora=ora)
        assert p.returncode == m["exit"] and m["exit"] in (105, 107), p.stderr
        assert p.stderr.decode().replace(E.INPUTS, "{in}").replace(str(tmp_path), "{out}") == m["stderr"]


@pytest.fixture(scope="module")
def cpuhost_tool():
    """The host pipeline linked against the CPU stand-in engine, which has no fq_ora_*."""
    binary = os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool")
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    return binary


def test_cli_accepts_and_needs_an_engine_with_ora(cpuhost_tool, tmp_path):
    """With the variable the flag is accepted: the run gets as far as attaching the counts to its
    engine, and against an engine library without fq_ora_* stops with one ERROR line."""
    p = run_cli(O.argv_for("x", "ora_pe", str(tmp_path))[1:], tmp_path, ora=True, binary=cpuhost_tool)
    lines = [l for l in p.stderr.decode().splitlines() if l.startswith("ERROR:")]
    assert p.returncode == 255 and len(lines) == 1 and "fq_ora_" in lines[0], p.stderr
    # the same command line without --ora runs there
    args = [a for a in O.argv_for("x", "ora_pe", str(tmp_path))[1:] if a != "--ora"]
    assert run_cli(args, tmp_path, ora=True, binary=cpuhost_tool).returncode == 0


# ---- the kernels' per-read routine on the host --------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("sim") / "ora_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", os.path.join(abi.REPO_DIR, "tools", "micro", "ora_sim.cpp"),
                    "-o", binary], check=True)
    return binary


def test_sim_self_check(sim):
    subprocess.run([sim, "--self"], check=True, timeout=120)


def test_sim_sanitized(tmp_path):
    """The same self check under AddressSanitizer and UBSan: every access of the routine lands inside
    the exactly sized heap blocks."""
    binary = str(tmp_path / "ora_sim_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(abi.REPO_DIR, "tools", "micro", "ora_sim.cpp"), "-o", binary], check=True)
    subprocess.run([binary, "--self"], check=True, timeout=300)


def sim_blocks(sim, tmp_path, pk, p, res, model_args, counts):
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    O.write_sim_input(inp, pk, p, res, *model_args, counts=counts)
    subprocess.run([sim, inp, out], check=True, timeout=120)
    return np.fromfile(out, np.uint64)


@pytest.mark.parametrize("name,sampling", [("C3", 1), ("C3", 3), ("C2", 1), ("C4", 1), ("PE_merge_discard", 3),
                                           ("PE_umi_merge", 100)])
def test_sim_matches_model(sim, oracle, tmp_path, name, sampling):
    """The GPU tests' packs through the routine on the host: two packs in a row, the running counts
    carried from the first into the second."""
    p = config(name, max_cycles=512)
    paired = bool(p.paired)
    packs = [O.hot_pack(700, paired, 11), O.hot_pack(333, paired, 12)]
    sets = O.pools()
    args = (sampling, 151, 140, sets[0], sets[1])
    model = O.Model(*args)
    counts = [0, 0, 0, 0]
    total = np.zeros(model.array().size, np.uint64)
    for pk in packs:
        res, _ = run_oracle(oracle, p, pk)
        K.model_pack(pk, p, res, 0, model)
        got = sim_blocks(sim, tmp_path, pk, p, res, args, counts)
        total += got[:-4]
        counts = [int(c) for c in got[-4:]]
        assert counts == model.reads
    assert model.rows[0].sum() > 0 and model.rows[2].sum() > 0 and np.array_equal(total, model.array())
