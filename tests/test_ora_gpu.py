"""Overrepresented-sequence counting on the GPU (fq_ora_*, fqtool_amd/csrc/ora.hip) against the Python
model of the reference's counting (tests/ora_util.py, pinned to the reference's reports by
tests/test_ora_cpu.py), and the tool with FQ_ORA=1 against the reference's fixtures.

Bit-exact: the four blocks [pre-R1 | pre-R2 | post-R1 | post-R2] must equal the model's.  The post
blocks' expectation comes from the ORACLE's records of the same pack, never from the engine's own."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kmer_util as K
import ora_util as O
from batch_util import Pack, config, run_oracle
from fqtool_amd import abi
from test_kstat_gpu import make_engine, run_pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


def engine_blocks(lib, p, packs, args, entry="process"):
    """The packs, in order, through one engine with one handle; the four blocks."""
    h, ora = make_engine(lib, p, packs), O.make_ora(lib, *args)
    try:
        assert lib.fq_engine_set_ora(h, ora) == 0, lib.fq_engine_last_error(h)
        for i, pk in enumerate(packs):
            run_pack(lib, h, pk, entry, i, merge=bool(p.merge_enabled))
        return O.read_blocks(lib, ora)
    finally:
        lib.fq_engine_destroy(h)
        lib.fq_ora_destroy(ora)


def model_blocks(oracle, p, packs, args):
    model = O.Model(*args)
    for pk in packs:
        res, _ = run_oracle(oracle, p, pk)
        K.model_pack(pk, p, res, 0, model)
    return model


def check(model, got):
    want = model.array()
    assert want.size == got.size
    if not np.array_equal(want, got):
        bad = np.nonzero(want != got)[0]
        edges = np.cumsum([0] + [r.size for r in model.rows])
        t = int(np.searchsorted(edges, bad[0], side="right") - 1)
        row, col = divmod(int(bad[0] - edges[t]), 1 + model.eval[t])
        raise AssertionError("%d counters differ; first: block %d sequence %d (%d bytes) word %d: model %d engine %d" % (
            len(bad), t, row, len(model.seqs[t][row]), col, want[bad[0]], got[bad[0]]))


def args_for(sampling, eval1=151, eval2=140, sets=None):
    sets = sets or O.pools()
    return (sampling, eval1, eval2, sets[0], sets[1])


def test_create_limits(lib):
    s = O.pools()
    for bad in ((0, 151, 151), (-1, 151, 151), (1, 2, 151), (1, 151, 2), (1, 0, 151)):
        O.make_ora(lib, bad[0], bad[1], bad[2], s[0], s[1], expect=abi.FQ_E_INVALID)
    O.make_ora(lib, 1, 151, 151, [b"ACGTACGTAC", b"ACGTACGTAC"], [], expect=abi.FQ_E_INVALID)  # a repeated member
    ora = O.make_ora(lib, 1, 3, 151, s[0], [])  # evalLen 3: the fifth step is 1; an empty R2 set
    try:
        assert lib.fq_ora_words(ora) == 2 * len(s[0]) * 4
        assert not O.read_blocks(lib, ora).any()
        small = np.zeros(4, np.uint64)
        assert lib.fq_ora_read(ora, small.ctypes.data, small.size) == abi.FQ_E_INVALID
    finally:
        lib.fq_ora_destroy(ora)
    empty = O.make_ora(lib, 5, 151, 151, [], [])
    try:
        assert lib.fq_ora_words(empty) == 0 and O.read_blocks(lib, empty).size == 0
    finally:
        lib.fq_ora_destroy(empty)


def edge_reads_pack(sets, paired, stride=160):
    """Reads of length 0 .. 12; every hot sequence alone at len == step, step + 1, step + 2 (0, 1 and 2
    windows examined), twice back to back (the second is skipped) and with one byte between (both
    count), at the start, the end and across the 16-byte chunk edges; reads longer than evalLen."""
    import random
    rng = random.Random(3)
    reads = [O.rand_seq(rng, L) for L in range(13)]
    for h in sets[0] + (sets[1] or ()):
        n = len(h)
        for extra in (0, 1, 2):
            if n + extra <= stride:
                reads.append(h + O.rand_seq(rng, extra))
        for lead in (0, 1, 15, 16, 17, stride - 2 * n - 3):
            if lead >= 0 and lead + 2 * n + 3 <= stride:
                reads.append(O.rand_seq(rng, lead) + h + h + b"AC")
                reads.append(O.rand_seq(rng, lead) + h + b"T" + h + b"AC")
        if n + 2 <= stride:
            reads.append(O.rand_seq(rng, stride - n - 2) + h + b"GA")
    pk = Pack(len(reads), stride, paired)
    for i, s in enumerate(reads):
        pk.set(i, 1, s, b"I" * len(s))
        if paired:
            s2 = reads[(i * 7 + 3) % len(reads)]
            pk.set(i, 2, s2, b"I" * len(s2))
    return pk


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("evals", [(151, 140), (150, 151), (42, 22), (12, 3)])
def test_lengths_steps_and_neighbours(lib, oracle, paired, evals):
    """The smallest reads that can go wrong, at evaluated lengths whose fifth step is 149, 148, 40 (equal
    to another step), 20, 10 and 1, with members of exactly those lengths in the sets."""
    import random
    rng = random.Random(evals[0])
    sets = []
    for st in range(2):
        fifth = min(150, evals[st] - 2)
        hot = set(O.pools()[st]) | {O.rand_seq(rng, fifth), O.rand_seq(rng, fifth)}
        sets.append(tuple(sorted(hot)))
    p = config("C3" if paired else "C2", max_cycles=256)
    pk = edge_reads_pack(sets, paired)
    args = (1, evals[0], evals[1], sets[0], sets[1])
    model = model_blocks(oracle, p, [pk], args)
    assert model.rows[0][:, 0].sum() > 0 and model.rows[2][:, 0].sum() > 0
    check(model, engine_blocks(lib, p, [pk], args))


def test_empty_r2_set(lib, oracle):
    p = config("C3", max_cycles=256)
    pk = O.hot_pack(300, True, 5)
    args = (1, 151, 151, O.pools()[0], ())
    model = model_blocks(oracle, p, [pk], args)
    assert model.rows[1].size == 0 and model.rows[0].sum() > 0
    check(model, engine_blocks(lib, p, [pk], args))


@pytest.mark.parametrize("sampling", [1, 3, 100])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 3001])
def test_sampling_across_packs(lib, oracle, n, sampling):
    """n pairs fed as several packs, about half of them failing -q: the four running counts carry over
    the pack borders (the post counts are prefix counts over the filter results)."""
    p = config("C3", max_cycles=256)
    cuts = sorted({0, n // 3, n // 3 + 1, (2 * n) // 3, n})
    whole = O.hot_pack(n, True, 100 + n)
    packs = []
    for a, b in zip(cuts, cuts[1:]):
        pk = Pack(b - a, whole.stride, True)
        for k in ("seq1", "qual1", "len1", "seq2", "qual2", "len2"):
            getattr(pk, k)[:] = getattr(whole, k)[a:b]
        packs.append(pk)
    args = args_for(sampling)
    model = model_blocks(oracle, p, packs, args)
    assert model.reads[0] == n and (n < 30 or 0.2 * n < model.reads[2] < 0.8 * n)
    check(model, engine_blocks(lib, p, packs, args))
    if n > 1:  # one pack of all n gives the same
        check(model, engine_blocks(lib, p, [whole], args))


VARIANTS = [("C2", 160), ("SE_all", 320), ("SE_umi", 160), ("C3", 160), ("C5", 320), ("C4", 160), ("C4", 320),
            ("PE_merge_discard", 160), ("PE_umi", 160), ("PE_umi_merge", 160), ("PE_correct", 160),
            ("PE_correct_umi_merge", 160), ("PE_correct_all", 320)]


@pytest.mark.parametrize("name,stride", VARIANTS)
def test_pack_variants(lib, oracle, name, stride):
    """SE, PE, -m (merged with hits across the junction, unmerged, discarded), UMI front trims, -c (the
    post pass reads the corrected planes, the pre pass the original ones), index-filtered pairs, both
    row strides; merged reads are longer than evalLen (the distribution's cut-off)."""
    p = config(name, max_cycles=1024)
    paired = bool(p.paired)
    packs = [O.hot_pack(900, paired, 3, stride=stride), O.hot_pack(500, paired, 4, stride=stride, read_len=stride - 9)]
    for pk in packs:
        pk.flags = (np.random.default_rng(2).random(pk.n) < 0.1).astype(np.uint8) * abi.FQ_BF_INDEX_FILTERED
    args = args_for(2)
    model = model_blocks(oracle, p, packs, args)
    assert model.rows[0][:, 0].sum() > 0 and model.rows[2][:, 0].sum() > 0
    if p.merge_enabled:
        res, _ = run_oracle(oracle, p, packs[0])
        assert ((res["flags"][0::2] & abi.FQ_RF_MERGED) != 0).sum() > 50
    check(model, engine_blocks(lib, p, packs, args))


@pytest.mark.parametrize("entry", ["submit", "device", "device_norecords", "text"])
@pytest.mark.parametrize("name", ["C3", "C2", "C4"])
def test_entry_points(lib, oracle, entry, name):
    """Every way into the engine passes through the same launch."""
    p = config(name, max_cycles=512)
    packs = [O.hot_pack(700, bool(p.paired), 21), O.hot_pack(400, bool(p.paired), 22)]
    args = args_for(3)
    check(model_blocks(oracle, p, packs, args), engine_blocks(lib, p, packs, args, entry=entry))


def test_contention_on_one_sequence(lib, oracle):
    """2048 identical reads at sampling 1: every increment lands on one sequence's cells."""
    p = config("C2", max_cycles=256)
    hot = O.pools()[0]
    h100 = next(s for s in hot if len(s) == 100)
    read = b"ACGTA" + h100 + b"GATTACAGATTACAGATTACA"
    pk = Pack(2048, 160, False)
    for i in range(pk.n):
        pk.set(i, 1, read, b"I" * len(read))
    args = args_for(1)
    model = model_blocks(oracle, p, [pk], args)
    assert model.rows[0][hot.index(h100), 0] == 2048 and model.rows[2][hot.index(h100), 0] == 2048
    check(model, engine_blocks(lib, p, [pk], args))


def test_object_behaviour(lib, oracle):
    """Several packs accumulate; reset clears the blocks and the running counts; a detached handle
    stops counting; the handle survives its engine."""
    p = config("C3", max_cycles=256)
    packs = [O.hot_pack(500 + 37 * i, True, 40 + i) for i in range(3)]
    args = args_for(7)
    h, ora = make_engine(lib, p, packs), O.make_ora(lib, *args)
    try:
        assert lib.fq_engine_set_ora(h, ora) == 0
        run_pack(lib, h, packs[0])
        first = O.read_blocks(lib, ora)
        check(model_blocks(oracle, p, packs[:1], args), first)
        assert lib.fq_ora_last_kernel_ms(ora) > 0
        run_pack(lib, h, packs[1])
        check(model_blocks(oracle, p, packs[:2], args), O.read_blocks(lib, ora))
        assert lib.fq_ora_reset(ora) == 0
        assert not O.read_blocks(lib, ora).any()
        run_pack(lib, h, packs[0])  # (the counts restarted too: the same reads are sampled again)
        assert np.array_equal(first, O.read_blocks(lib, ora))
        assert lib.fq_engine_set_ora(h, None) == 0
        run_pack(lib, h, packs[1])
        assert np.array_equal(first, O.read_blocks(lib, ora))
        lib.fq_engine_destroy(h)
        h = make_engine(lib, p, packs)
        assert lib.fq_engine_set_ora(h, ora) == 0
        run_pack(lib, h, packs[1])
        check(model_blocks(oracle, p, packs[:2], args), O.read_blocks(lib, ora))
    finally:
        lib.fq_engine_destroy(h)
        lib.fq_ora_destroy(ora)


@pytest.mark.parametrize("name", ["C3", "PE_correct_umi_merge", "SE_all"])
def test_no_side_effect(lib, oracle, name):
    """The same pack with and without a handle attached: identical records and accumulator (the
    oracle's)."""
    p = config(name, max_cycles=512)
    pk = O.hot_pack(1500, bool(p.paired), 9)
    res_o, acc_o = run_oracle(oracle, p, pk)
    for attach in (False, True):
        h, ora = make_engine(lib, p, [pk]), O.make_ora(lib, *args_for(1))
        try:
            if attach:
                assert lib.fq_engine_set_ora(h, ora) == 0
            res = run_pack(lib, h, pk)
            acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
            assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
            assert np.array_equal(res, res_o) and np.array_equal(acc, acc_o), attach
            assert O.read_blocks(lib, ora).any() == attach
        finally:
            lib.fq_engine_destroy(h)
            lib.fq_ora_destroy(ora)


# ---- the tool -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", O.ok_cases())
def test_tool_matches_reference(case, tmp_path):
    """fqtool with FQ_ORA=1 on every ORA fixture: FASTQ, JSON and HTML byte-identical to the reference's."""
    out = str(tmp_path)
    env = dict(os.environ, FQ_ORA="1")
    p = subprocess.run(O.argv_for(abi.FQTOOL_BIN, case, out), capture_output=True, cwd=out, timeout=120, env=env)
    assert p.returncode == 0, p.stderr.decode()
    O.check_files(case, out)
    O.check_reports(case, out)


def test_tool_uses_one_engine(tmp_path):
    """Several --devices: the run uses the first and says so; the reports are the same."""
    out = str(tmp_path)
    env = dict(os.environ, FQ_ORA="1")
    argv = O.argv_for(abi.FQTOOL_BIN, "ora_pe_s7", out, extra=("--devices", "0,0", "--pack_pairs", "500"))
    p = subprocess.run(argv, capture_output=True, cwd=out, timeout=120, env=env)
    assert p.returncode == 0, p.stderr.decode()
    assert "--ora: one engine on device 0 of the 2 given" in p.stderr.decode()
    O.check_files("ora_pe_s7", out)
    O.check_reports("ora_pe_s7", out)
