"""The device ingest on the CPU: the Python model of the index filter, --phred64 and the pack cuts
(tests/ingest_util.py) pinned to the reference's output files on the index-filter, phred64 and split
cases of tests/golden/e2e, through the host's option handling and the oracle's records; the kernels'
per-record routines (fqtool_amd/csrc/ingest_core.h) run on the host by tools/micro/ingest_sim.cpp,
built with the address and undefined-behaviour sanitizers, against the model on the synthetic pack of
hostile names; fq_cuts_bound / fq_cuts_count against the model's tables; and the tool against the CPU
stand-in engine, which lacks the new calls and so keeps the host packs."""
import os
import re
import subprocess

import numpy as np
import pytest

import e2e_util as E
import egress_util as G
import ingest_util as I
import umi_util as U
from batch_util import config, run_oracle
from fqtool_amd import abi

CPU_BIN = os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool")


@pytest.fixture(scope="module")
def host(oracle):
    import ctypes
    if not (os.path.exists(abi.HOST_LIB) and os.path.exists(abi.FQTOOL_BIN)):
        subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "host"], check=True)
    lib = abi.load_host()
    backend = E.oracle_kmer_backend(oracle)
    lib.fqh_set_kmer_backend(ctypes.addressof(backend))
    yield lib
    lib.fqh_set_kmer_backend(None)


@pytest.fixture(scope="module")
def cases(host, oracle, tmp_path_factory):
    """case -> (reads per mate as the input files hold them, the oracle's records of the whole input,
    the run's fq_params): one session run per case, the oracle as the engine."""
    cache = {}

    def get(case):
        if case not in cache:
            out = str(tmp_path_factory.mktemp(case))
            parts, params = [], []
            inner = E.oracle_process(oracle)

            def process(p, b, nres, mc):
                res, acc = inner(p, b, nres, mc)
                parts.append(res.copy())
                params.append(p)
                return res, acc
            E.run_session(host, E.argv_for("fqtool", case, out), process, dup_engine=lambda k: E.OracleDup(oracle, k))
            reads = G.case_reads(case)
            res = np.concatenate(parts)
            assert len(res) == len(reads[0].names) * len(reads)
            cache[case] = (reads, res, params[0])
        return cache[case]
    return get


@pytest.fixture(scope="module")
def cpu_tool(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    runs = {}

    def run(case):
        """The stand-in's run of a case, once per case: (its stderr, its output directory)."""
        if case not in runs:
            outdir = str(tmp_path_factory.mktemp("cpu_" + case))
            p = subprocess.run(E.argv_for(CPU_BIN, case, outdir), capture_output=True, cwd=outdir, timeout=300)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            runs[case] = (p.stderr.decode(), outdir)
        return runs[case]
    return run


def out_names(case):
    return [os.path.basename(I.case_option(case, o)) for o in ("-o", "-O") if I.case_option(case, o)]


# ---- the model against the reference --------------------------------------------------------------
@pytest.mark.parametrize("case", I.INDEX_CASES)
def test_index_model_matches_reference(case, cases):
    """The model's flags are the records' FQ_RF_INDEX_FILTERED bits, and the streams of the records
    under the model's flags are the reference's files (sha256)."""
    reads, res, p = cases(case)
    l1, l2, t = I.case_lists(case)
    flags = I.index_flags(reads, l1, l2, t)
    mates = len(reads)
    assert np.array_equal(flags != 0, (res["flags"][::mates] & abi.FQ_RF_INDEX_FILTERED) != 0)
    if l1 or l2:
        assert 0 < np.count_nonzero(flags) < len(flags)
    u = U.case_umi(("e2e", case))  # (td_pe_index_diff1 tags its names too: the filter sees the input names)
    streams = U.model(reads, I.with_flags(res, flags, mates), mates == 2, False, False, G.case_mask(case), u if u.location else None)
    m = E.manifest()[case]
    files = G.case_streams(case)
    assert sorted(files.values()) == sorted(m["outputs"])
    for s, name in files.items():
        assert G.sha(streams[s]) == m["outputs"][name], "%s: %s" % (case, name)


@pytest.mark.parametrize("case", I.PHRED64_CASES)
def test_phred64_model_matches_reference(case, cases):
    reads, res, p = cases(case)
    assert any(q != I.phred64(q) for q in reads[0].quals)
    streams = G.model(I.phred64_reads(reads), res, len(reads) == 2, False, False, G.case_mask(case))
    m = E.manifest()[case]
    for s, name in G.case_streams(case).items():
        assert G.sha(streams[s]) == m["outputs"][name], "%s: %s" % (case, name)


def test_phred64_rule():
    q = bytes(range(256))
    want = bytes(max(33, (b - 256 if b >= 128 else b) - 31) for b in range(256))
    assert I.phred64(q) == want
    assert want[63] == 33 and want[64] == 33 and want[65] == 34 and want[127] == 96 and want[128] == 33 and want[255] == 33


@pytest.mark.parametrize("case", I.SPLIT_CASES)
def test_split_model_matches_reference(case, cases, cpu_tool):
    """(stream, cuts) -> the numbered files, from device packs of 777 records (so most packs start
    inside a reference pack), equal the reference's files."""
    reads, res, p = cases(case)
    mates, n = len(reads), len(reads[0].names)
    every = int(I.case_option(case, "--max_item_in_pack"))
    by_lines = "-S" in G.case_args(case)
    if by_lines:
        split_size, split_number = int(I.case_option(case, "--splie_file_line")), 0
    else:  # the split size comes from the evaluator's read-count estimate, which the tool logs
        split_number = int(I.case_option(case, "--split_file_number"))
        split_size = int(re.search(r"split size: (\d+)", cpu_tool(case)[0]).group(1))
    packs = []
    for first in range(0, n, 777):
        hi = min(n, first + 777)
        sub = [G.Reads(r.names[first:hi], r.strands[first:hi], r.seqs[first:hi], r.quals[first:hi]) for r in reads]
        sres = res[mates * first:mates * hi]
        mask = G.mask(G.OUT1, G.OUT2) if mates == 2 else G.mask(G.OUT1)
        streams = G.model(sub, sres, mates == 2, False, False, mask)
        sizes = I.out_sizes(sub, sres)
        assert [int(z.sum()) for z in sizes] == [len(streams[m]) for m in range(mates)]
        cuts = I.cut_table(sizes, every, first)
        assert len(cuts) == I.cuts_count(every, first, hi - first)
        packs.append((first, streams, cuts))
    files = I.split_files(packs, out_names(case), every, by_lines, split_size, split_number)
    m = E.manifest()[case]
    assert sorted(files) == sorted(m["outputs"])
    for name, data in files.items():
        assert G.sha(data) == m["outputs"][name], "%s: %s" % (case, name)


# ---- ingest_core.h on the host --------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("sim") / "ingest_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(abi.REPO_DIR, "tools", "micro", "ingest_sim.cpp"), "-o", binary], check=True)
    return binary


@pytest.fixture(scope="module")
def synth(oracle):
    """paired -> (pack, texts, reads, the oracle's records under ingest_util.SYNTH_CFG)."""
    cache = {}

    def get(paired):
        if paired not in cache:
            pk, texts = U.synth_pack_and_texts(paired)
            reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
            res, _ = run_oracle(oracle, config(I.SYNTH_CFG[paired], max_cycles=512), pk)
            cache[paired] = (pk, texts, reads, res)
        return cache[paired]
    return get


def expected_filtered(name, paired, count, n):
    """The condition of the GPU tests: a non-degenerate list drops some records and keeps some."""
    if name in I.DEGENERATE:
        assert count == (n if I.DEGENERATE[name] == "all" else 0)
    elif name == "list2only1" and not paired:
        assert count == 0  # single end uses list 1 only
    else:
        assert 0 < count < n, (name, paired, count)


@pytest.mark.parametrize("paired", [True, False], ids=["PE", "SE"])
def test_sim_matches_model(paired, synth, sim, tmp_path):
    pk, texts, reads, res = synth(paired)
    sizes = I.out_sizes(reads, res)
    assert 0 < np.count_nonzero(sizes[0]) < pk.n
    lists = dict(I.SYNTH_LISTS, big=(I.big_list(), [], 0))
    cuts_args = [(1, 0), (7, 0), (7, 5), (pk.n, 0), (pk.n + 1, 5), (pk.n, 5)]
    for k, (name, lst) in enumerate(lists.items()):
        every, first = cuts_args[k % len(cuts_args)]
        convert = k % 2
        inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        I.write_sim_input(inp, [t[:2] for t in texts], paired, pk.stride, lst, sizes, every, first, convert)
        subprocess.run([sim, inp, out], check=True, timeout=120)
        flags, out_texts, cuts = I.read_sim_output(out, [t[:2] for t in texts])
        want = I.index_flags(reads, *lst)
        if name != "big":
            expected_filtered(name, paired, int(np.count_nonzero(want)), pk.n)
        assert np.array_equal(flags, want), name
        for m in range(len(texts)):
            assert out_texts[m] == (I.converted_text(*texts[m][:2]) if convert else texts[m][0].tobytes()), (name, m)
        assert cuts == I.cut_table(sizes, every, first), (name, every, first)


def test_hostile_qualities_cover_the_phred64_branches(synth):
    """edge_pack's qualities hold bytes below 64, above 64 and >= 128."""
    pk = synth(True)[0]
    q = np.concatenate([pk.qual1[i, :int(pk.len1[i])] for i in range(pk.n)])
    assert (q < 64).any() and (q > 64).any() and (q >= 128).any()


# ---- the bound ------------------------------------------------------------------------------------
def test_cuts_bound_covers_every_table():
    lib = abi.load_engine()
    assert lib.fq_cuts_bound(0, 100) == 0 and lib.fq_cuts_count(0, 0, 100) == 0
    for every in (1, 2, 7, 100, 699, 700, 701, 5000):
        for first in (0, 1, 5, 6, 7, 699, 700, 12345):
            for n in (0, 1, 6, 7, 8, 700):
                sizes = [np.ones(n, np.uint32)]
                table = I.cut_table(sizes, every, first)
                assert lib.fq_cuts_count(every, first, n) == len(table) == I.cuts_count(every, first, n)
                assert len(table) <= lib.fq_cuts_bound(every, n) == n // every + 2
                assert sum(c.items for c in table) == n


# ---- the stand-in engine --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["td_pe_index", "td_pe_split_num", "edge64_pe"])
def test_stand_in_engine_keeps_host_packs(case, cpu_tool):
    """build/cpuhost/fqtool links the CPU stand-in, which has none of the new calls: the weakly bound
    calls are absent, the run goes through host packs and is the reference's byte for byte."""
    err, outdir = cpu_tool(case)
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1 and "(raw stream" not in closing[0] and "(text packs" not in closing[0], err[-2000:]
    E.check_outputs(case, outdir)
