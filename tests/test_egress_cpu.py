"""Routed egress on the CPU: the Python model of the six output streams (tests/egress_util.py)
pinned to the reference's output files (tests/golden/e2e, made by tests/golden/make_e2e.py) through
the host's option handling and the oracle's records; the kernels' per-pair routine
(fqtool_amd/csrc/egress_core.h) run on the host by tools/micro/egress_sim.cpp against the model;
fq_egress_bound against the size of every model output."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import e2e_util as E
import egress_util as G
from fqtool_amd import abi


@pytest.fixture(scope="module")
def host(oracle):
    if not (os.path.exists(abi.HOST_LIB) and os.path.exists(abi.FQTOOL_BIN)):
        subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "host"], check=True)
    lib = abi.load_host()
    backend = E.oracle_kmer_backend(oracle)
    lib.fqh_set_kmer_backend(ctypes.addressof(backend))
    yield lib
    lib.fqh_set_kmer_backend(None)


@pytest.fixture(scope="module")
def cases(host, oracle, tmp_path_factory):
    """case -> (reads per mate, the oracle's records of the whole input, the run's fq_params, the
    model's six streams): one session run per case, the oracle as the engine."""
    cache = {}

    def get(case):
        if case in cache:
            return cache[case]
        out = str(tmp_path_factory.mktemp(case))
        parts, params = [], []
        inner = E.oracle_process(oracle)

        def process(p, b, nres, mc):
            res, acc = inner(p, b, nres, mc)
            parts.append(res.copy())
            params.append(p)
            return res, acc
        E.run_session(host, E.argv_for("fqtool", case, out), process, dup_engine=lambda k: E.OracleDup(oracle, k))
        res, p = np.concatenate(parts), params[0]
        reads = G.case_reads(case)
        assert len(res) == len(reads[0].names) * len(reads) and bool(p.paired) == (len(reads) == 2)
        streams = G.model(reads, res, bool(p.paired), bool(p.merge_enabled), bool(p.discard_unmerged),
                          G.case_mask(case))
        cache[case] = (reads, res, p, streams)
        return cache[case]
    return get


@pytest.mark.parametrize("case", G.PINNED_CASES)
def test_model_streams_match_reference(case, cases):
    """Every output file the case names holds the model's stream, byte for byte (sha256)."""
    _, _, _, streams = cases(case)
    m = E.manifest()[case]
    files = G.case_streams(case)
    assert sorted(files.values()) == sorted(m["outputs"])
    for s, name in files.items():
        assert G.sha(streams[s]) == m["outputs"][name], "%s: %s (%s)" % (case, name, G.STREAM_NAMES[s])
    for s in range(G.STREAMS):
        assert s in files or not streams[s]


def test_pinned_cases_reach_every_stream(cases):
    for s in range(G.STREAMS):
        assert any(cases(c)[3][s] for c in G.PINNED_CASES), G.STREAM_NAMES[s]


def test_bound_covers_every_model_output(cases):
    lib = abi.load_engine()
    for case in G.PINNED_CASES:
        reads, _, _, streams = cases(case)
        t1 = G.text_bytes(reads[0])
        t2 = G.text_bytes(reads[1]) if len(reads) == 2 else 0
        for s in range(G.STREAMS):
            assert lib.fq_egress_bound(s, t1, t2, len(reads[0].names)) >= len(streams[s]), (case, G.STREAM_NAMES[s])
    # a FAILED record is its input plus a blank and the longest tag
    assert lib.fq_egress_bound(G.FAILED, 100, 0, 1) >= 100 + G.LONGEST_TAG
    assert lib.fq_egress_bound(G.FAILED, 100, 100, 1) >= 200 + 2 * G.LONGEST_TAG


# ---- the kernels' per-pair routine on the host --------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("sim") / "egress_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", os.path.join(abi.REPO_DIR, "tools", "micro", "egress_sim.cpp"),
                    "-o", binary], check=True)
    return binary


@pytest.mark.parametrize("case", G.PINNED_CASES)
def test_sim_matches_model(case, cases, sim, tmp_path):
    reads, res, p, streams = cases(case)
    texts = [G.fastq_of(r) for r in reads]
    stride = max(16, E.round16(max(max((len(s) for s in r.seqs), default=0) for r in reads)))
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    G.write_sim_input(inp, texts, res, bool(p.paired), bool(p.merge_enabled), bool(p.discard_unmerged),
                      bool(p.correction_enabled), G.case_mask(case), stride)
    subprocess.run([sim, inp, out], check=True, timeout=120)
    got = G.read_sim_output(out)
    for s in range(G.STREAMS):
        assert got[s] == streams[s], "%s: %s" % (case, G.STREAM_NAMES[s])


def test_sim_drops_streams_without_a_writer(cases, sim, tmp_path):
    """Only OUT1 / OUT2 open on a case that feeds every other stream: those two alone, unchanged
    except that read 1 of a pair whose read 2 alone passes no longer counts on the left writer."""
    reads, res, p, _ = cases("td_pe_all")
    texts = [G.fastq_of(r) for r in reads]
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open_mask = G.mask(G.OUT1, G.OUT2)
    G.write_sim_input(inp, texts, res, True, False, False, False, open_mask, 160)
    subprocess.run([sim, inp, out], check=True, timeout=120)
    assert G.read_sim_output(out) == G.model(reads, res, True, False, False, open_mask)
