"""UMI (-u) on the routed egress, on the CPU: the Python model of the tag, the tagged name and the
NULL-read cut (tests/umi_util.py) pinned to the reference's output files on every UMI case of
tests/golden/e2e and tests/golden/umi, through the host's option handling and the oracle's records;
the kernels' per-pair routine (fqtool_amd/csrc/egress_core.h) run on the host by
tools/micro/egress_sim.cpp, built with the address and undefined-behaviour sanitizers, against the
model on those cases and on a synthetic pack of hostile names; fq_egress_bound_umi against every
model stream; and the tool against the CPU stand-in engine, which lacks the UMI calls and so keeps
the host packs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import e2e_util as E
import egress_util as G
import umi_util as U
from batch_util import run_oracle
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
    """case -> (reads per mate, the oracle's records of the whole input, the run's fq_params, the UMI
    description, the model's six streams): one session run per case, the oracle as the engine."""
    cache = {}

    def get(case):
        if case in cache:
            return cache[case]
        out = str(tmp_path_factory.mktemp(case[1]))
        parts, params = [], []
        inner = E.oracle_process(oracle)

        def process(p, b, nres, mc):
            res, acc = inner(p, b, nres, mc)
            parts.append(res.copy())
            params.append(p)
            return res, acc
        E.run_session(host, U.argv_for("fqtool", case, out), process, dup_engine=lambda k: E.OracleDup(oracle, k))
        res, p = np.concatenate(parts), params[0]
        reads, u = U.case_reads(case), U.case_umi(case)
        assert len(res) == len(reads[0].names) * len(reads) and bool(p.paired) == (len(reads) == 2)
        assert (int(p.umi_front1), int(p.umi_front2)) == (U.umi_front(u, 0, bool(p.paired)), U.umi_front(u, 1, bool(p.paired)))
        streams = U.model(reads, res, bool(p.paired), bool(p.merge_enabled), bool(p.discard_unmerged), U.case_mask(case), u)
        cache[case] = (reads, res, p, u, streams)
        return cache[case]
    return get


@pytest.mark.parametrize("case", U.ALL_CASES, ids=U.CASE_IDS)
def test_model_streams_match_reference(case, cases):
    """Every output file the case names holds the model's stream, byte for byte (sha256)."""
    _, _, _, _, streams = cases(case)
    m = U.entry(case)
    files = U.case_streams(case)
    assert sorted(files.values()) == sorted(m["outputs"])
    for s, name in files.items():
        assert G.sha(streams[s]) == m["outputs"][name], "%s: %s (%s)" % (case[1], name, G.STREAM_NAMES[s])


def test_cases_cover_the_locations_and_flags():
    umis = [U.case_umi(c) for c in U.ALL_CASES]
    assert {u.location for u in umis} == {0, 1, 2, 3, 4, 5, 6}  # (0: -u without --umi_location)
    assert {(u.location, u.not_trim) for u in umis} >= {(3, 1), (4, 1), (6, 1)}
    assert any(u.location == 6 and not u.drop_comment for u in umis) and any(u.drop_comment for u in umis)
    assert len(U.OLD_CASES) >= 8 and len(U.NEW_CASES) >= 8


# ---- the kernels' per-pair routine on the host --------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    binary = str(tmp_path_factory.mktemp("sim") / "egress_sim")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(abi.REPO_DIR, "tools", "micro", "egress_sim.cpp"), "-o", binary], check=True)
    return binary


def run_sim(sim, tmp_path, texts, res, p, open_mask, stride, u):
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    if u.location == 0:  # -u without --umi_location: the run has no description, the routine runs without one
        G.write_sim_input(inp, [t[:2] for t in texts], res, bool(p.paired), bool(p.merge_enabled), bool(p.discard_unmerged),
                          bool(p.correction_enabled), open_mask, stride)
    else:
        U.write_sim_input(inp, [t[:2] for t in texts], res, bool(p.paired), bool(p.merge_enabled), bool(p.discard_unmerged),
                          bool(p.correction_enabled), open_mask, stride, u)
    subprocess.run([sim, inp, out], check=True, timeout=120)
    return G.read_sim_output(out)


@pytest.mark.parametrize("case", U.ALL_CASES, ids=U.CASE_IDS)
def test_sim_matches_model_on_the_cases(case, cases, sim, tmp_path):
    reads, res, p, u, streams = cases(case)
    texts = [G.fastq_of(r) for r in reads]
    stride = max(16, E.round16(max(max((len(s) for s in r.seqs), default=0) for r in reads)))
    got = run_sim(sim, tmp_path, texts, res, p, U.case_mask(case), stride, u)
    for s in range(G.STREAMS):
        assert got[s] == streams[s], "%s: %s" % (case[1], G.STREAM_NAMES[s])


@pytest.fixture(scope="module")
def synth(oracle):
    """(config, location, not_trim, filtered) -> (pack, texts, params, records): the synthetic pack's
    records from the oracle, once per key; filtered: 15 % of the pairs carry FQ_BF_INDEX_FILTERED."""
    packs, cache = {}, {}

    def get(cfg, loc, not_trim, filtered):
        key = (cfg, loc, not_trim, filtered)
        if key not in cache:
            p, _ = U.synth_params(cfg, loc, 0, not_trim)
            paired = bool(p.paired)
            if paired not in packs:
                packs[paired] = U.synth_pack_and_texts(paired)
            pk, texts = packs[paired]
            pk.flags = (np.random.RandomState(3).rand(pk.n) < 0.15).astype(np.uint8) * abi.FQ_BF_INDEX_FILTERED if filtered else None
            res, _ = run_oracle(oracle, p, pk)
            pk.flags = None
            cache[key] = (pk, texts, p, res)
        return cache[key]
    return get


@pytest.mark.parametrize("cfg", U.SYNTH_CONFIGS)
def test_sim_matches_model_on_the_synthetic_pack(cfg, synth, sim, tmp_path):
    """Every location x drop_comment x not_trim; the index-filtered variant at every location."""
    lib = abi.load_engine()
    seen = [False] * G.STREAMS
    tagged = untagged = 0
    for loc, drop, not_trim in U.synth_umis():
        for filtered in ((0, 1) if drop == 0 else (0,)):
            pk, texts, p, res = synth(cfg, loc, not_trim, filtered)
            _, u = U.synth_params(cfg, loc, drop, not_trim)
            if filtered:
                assert (res["flags"] & abi.FQ_RF_INDEX_FILTERED).any()
            reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(len(texts))]
            open_mask = U.SYNTH_MASK[cfg]
            exp = U.model(reads, res, bool(p.paired), bool(p.merge_enabled), False, open_mask, u)
            got = run_sim(sim, tmp_path, texts, res, p, open_mask, pk.stride, u)
            t1, t2 = texts[0][0].size, texts[1][0].size if p.paired else 0
            for s in range(G.STREAMS):
                assert got[s] == exp[s], "%s, location %d, drop %d, not_trim %d: %s" % (cfg, loc, drop, not_trim, G.STREAM_NAMES[s])
                assert len(exp[s]) <= lib.fq_egress_bound_umi(s, t1, t2, pk.n, ctypes.byref(U.fq_umi(u)))
                seen[s] = seen[s] or bool(exp[s])
            tags = [U.umi_tag(u, reads, i) for i in range(pk.n)]
            tagged += sum(1 for t in tags if t)
            untagged += sum(1 for t in tags if not t)
    assert tagged and untagged
    for s in range(G.STREAMS):
        assert seen[s] == bool((U.SYNTH_MASK[cfg] >> s) & 1), G.STREAM_NAMES[s]


def test_synthetic_pack_has_null_reads_and_short_reads(synth):
    """What the NULL-read cut and the clamped parts need: NULL records of reads longer than the cut,
    and reads shorter than the UMI."""
    pk, texts, p, res = synth("PE_umi", 6, 0, 0)
    lens = np.stack([pk.len1, pk.len2], 1).reshape(-1)
    null = (res["flags"] & abi.FQ_RF_NULL) != 0
    assert (null & (lens > 1)).any()
    assert (lens == 0).any() and (lens < int(p.umi_front1)).any() and (pk.len1 < pk.len2).any() and (pk.len1 > pk.len2).any()


# ---- the bound -------------------------------------------------------------------------------------
def test_bound_covers_every_model_output(cases):
    lib = abi.load_engine()
    for case in U.ALL_CASES:
        reads, _, _, u, streams = cases(case)
        t1 = G.text_bytes(reads[0])
        t2 = G.text_bytes(reads[1]) if len(reads) == 2 else 0
        n = len(reads[0].names)
        for s in range(G.STREAMS):
            desc = ctypes.byref(U.fq_umi(u)) if u.location else None
            assert lib.fq_egress_bound_umi(s, t1, t2, n, desc) >= len(streams[s]), (case, G.STREAM_NAMES[s])


def test_bound_without_a_description_is_the_plain_bound():
    lib = abi.load_engine()
    for t1, t2, n in ((0, 0, 0), (100, 0, 1), (100, 100, 1), (123456, 120000, 777)):
        for s in range(-1, G.STREAMS + 1):
            assert lib.fq_egress_bound_umi(s, t1, t2, n, None) == lib.fq_egress_bound(s, t1, t2, n)
    # a sequence location adds the two prefixes and both parts per record, twice for FAILED's two mates
    u = abi.FqUmi(6, 8, 0, 0, 0)
    assert lib.fq_egress_bound_umi(G.OUT1, 100, 100, 1, ctypes.byref(u)) >= lib.fq_egress_bound(G.OUT1, 100, 100, 1) + 14 + 32
    assert lib.fq_egress_bound_umi(G.FAILED, 100, 100, 1, ctypes.byref(u)) >= lib.fq_egress_bound(G.FAILED, 100, 100, 1) + 2 * (14 + 32)


# ---- the stand-in engine ---------------------------------------------------------------------------
def test_stand_in_engine_keeps_host_packs(tmp_path):
    """build/cpuhost/fqtool links the CPU stand-in, which has no fq_engine_set_umi: the weakly bound
    calls are absent, the UMI run goes through host packs and is the reference's byte for byte."""
    subprocess.run(["make", "-s", "-C", abi.REPO_DIR, "cpuhost"], check=True)
    case = ("e2e", "td_pe_umi_r1")
    p = subprocess.run(U.argv_for(os.path.join(abi.REPO_DIR, "build", "cpuhost", "fqtool"), case, str(tmp_path)),
                       capture_output=True, cwd=tmp_path, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1 and "(raw stream" not in closing[0] and "(text packs" not in closing[0], err[-2000:]
    U.check_outputs(case, str(tmp_path))
