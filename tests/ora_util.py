"""--ora helpers: a Python model of the reference's overrepresented-sequence analysis -- the hot-set
selection of the evaluator pre-pass (Evaluator::computeOverRepSeq, reference
src/evaluator.cpp:120-189) and the per-read counting (Stats::statRead, src/stats.cpp:277-293) --
the fixtures written by tests/golden/make_ora.py, and engine test inputs."""
import collections
import ctypes
import functools
import gzip
import json
import os
import random

import numpy as np

import kmer_util as K
from fqtool_amd import abi
from e2e_util import GOLDEN, INPUTS, digest, mask_html, mask_software

ORA = os.path.join(GOLDEN, "ora")
HOT_STEPS = (10, 20, 40, 100, 149)  # computeOverRepSeq: min(150, 151 - 2)
BASE_LIMIT = 151 * 10000
DEFAULT_SAMPLING = 20  # reference src/options.h:158


# ---- the hot sets ---------------------------------------------------------------------------------
def keep_from(length):
    """The smallest count at which computeOverRepSeq keeps a substring of this length."""
    return 3 if length >= 150 else 5 if length >= 100 else 20 if length >= 40 else 100 if length >= 20 else 500


def hot_set(reads):
    """Evaluator::computeOverRepSeq over `reads` (bytes, in file order): the hot sequences in
    std::map order (bytes compare as unsigned chars, which is Python's order of bytes)."""
    counts = {}
    bases = 0
    taken = []
    for s in reads:
        if bases >= BASE_LIMIT:
            break
        bases += len(s)
        taken.append(s)
    for step in HOT_STEPS:
        c = collections.Counter(s[i:i + step] for s in taken for i in range(len(s) - step))  # i < rlen - step
        need = keep_from(step)
        counts.update({k: v for k, v in c.items() if v >= need})
    hot = dict(sorted(counts.items()))
    # the erase loop: in map order, against the map as it stands, integer division.  A container is a
    # longer member, so its windows at the shorter hot lengths are looked up once (the plain
    # "seq in s2" over all pairs is quadratic: 18.7 k hot 100-mers on the real-data input)
    lens = sorted({len(s) for s in hot})
    containers = {s: [] for s in hot}
    for big in hot:
        for n in lens:
            if n >= len(big):
                break
            for i in range(len(big) - n + 1):
                c = containers.get(big[i:i + n])
                if c is not None:
                    c.append(big)
    gone = set()
    for seq, count in hot.items():
        if any(s2 not in gone and count // hot[s2] < 10 for s2 in containers[seq]):
            gone.add(seq)
    return [s for s in hot if s not in gone]


@functools.lru_cache(maxsize=None)
def file_reads(path):
    return tuple(K.fastq_seqs(path))


@functools.lru_cache(maxsize=None)
def file_hot_set(path):
    return tuple(hot_set(file_reads(path)))


def steps_for(eval_len):
    return sorted({10, 20, 40, 100, min(150, eval_len - 2)})


# ---- the counting ---------------------------------------------------------------------------------
class Model:
    """The four Stats objects' ORA state: [pre-R1 | pre-R2 | post-R1 | post-R2].  add(table, seq) is
    one statRead call, in stream order per table (kmer_util.model_pack feeds it a pack)."""

    def __init__(self, sampling, eval1, eval2, set1, set2):
        self.sampling = sampling
        self.eval = [eval1, eval2, eval1, eval2]
        sets = [list(set1), list(set2)]
        self.seqs = [sets[0], sets[1], sets[0], sets[1]]
        self.reads = [0, 0, 0, 0]
        self.index, self.steps, self.rows = [], [], []
        for t in range(4):
            idx = {bytes(s): i for i, s in enumerate(self.seqs[t])}
            assert len(idx) == len(self.seqs[t])
            self.index.append(idx)
            lens = {len(s) for s in idx}
            # (a step that matches no hot length can never hit)
            self.steps.append([st for st in steps_for(self.eval[t]) if st in lens and st >= 1])
            self.rows.append(np.zeros((len(idx), 1 + self.eval[t]), np.uint64))

    def add(self, table, seq):
        n = self.reads[table]
        self.reads[table] = n + 1
        if n % self.sampling:
            return
        seq = bytes(seq)
        idx, rows, ev = self.index[table], self.rows[table], self.eval[table]
        for step in self.steps[table]:
            j = 0
            while j < len(seq) - step:
                i = idx.get(seq[j:j + step])
                if i is not None:
                    rows[i, 0] += 1
                    if j < ev:
                        rows[i, 1 + j:1 + min(j + step, ev)] += 1
                    j += step
                j += 1

    def array(self):
        return np.concatenate([r.reshape(-1) for r in self.rows]) if sum(r.size for r in self.rows) else np.zeros(0, np.uint64)

    def passing(self, table):
        """The report's OverrepresentedSequences of one Stats: {sequence: count}, None when empty."""
        out = {}
        for i, s in enumerate(self.seqs[table]):
            c = int(self.rows[table][i, 0])
            limit = {10: 500, 20: 200, 40: 100, 100: 50}.get(len(s), 20)
            if self.sampling * c > limit:
                out[bytes(s).decode("latin-1")] = c
        return out or None


def pack_set(seqs):
    """A set as fq_ora_create takes it: (bytes array, uint32 offsets, n); keeps the arrays alive."""
    data = np.frombuffer(b"".join(bytes(s) for s in seqs) or b"\0", np.uint8).copy()
    off = np.zeros(len(seqs) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return data, off, len(seqs)


def make_ora(lib, sampling, eval1, eval2, set1, set2, expect=0):
    a, b = pack_set(set1), pack_set(set2)
    h = ctypes.c_void_p()
    rc = lib.fq_ora_create(0, sampling, eval1, eval2, a[0].ctypes.data, a[1].ctypes.data, a[2],
                           b[0].ctypes.data, b[1].ctypes.data, b[2], ctypes.byref(h))
    assert rc == expect, rc
    return h


def read_blocks(lib, h):
    t = np.zeros(lib.fq_ora_words(h), np.uint64)
    assert lib.fq_ora_read(h, t.ctypes.data if t.size else None, t.size) == 0
    return t


# ---- fixtures (tests/golden/ora, written by tests/golden/make_ora.py) -----------------------------
def manifest():
    with open(os.path.join(ORA, "manifest.json")) as f:
        return json.load(f)


def ok_cases():
    return sorted(c for c, v in manifest().items() if v["exit"] == 0)


def err_cases():
    return sorted(c for c, v in manifest().items() if v["exit"] != 0)


def argv_for(binary, case, outdir, extra=()):
    args = manifest()[case]["args"]
    argv = [binary, "-w", "1", "-J", os.path.join(outdir, "report.json"), "-H", os.path.join(outdir, "report.html")]
    return argv + list(extra) + args.format(**{"in": INPUTS, "out": outdir}).split()


def golden_text(case, kind):
    with gzip.open(os.path.join(ORA, manifest()[case][kind]), "rt") as f:
        return f.read()


def check_files(case, outdir):
    """Every output file but the reports equals the reference's."""
    m = manifest()[case]
    present = {name: digest(os.path.join(outdir, name)) for name in sorted(os.listdir(outdir))
               if not name.startswith("report.")}
    assert sorted(present) == sorted(m["outputs"]), (sorted(present), sorted(m["outputs"]))
    for name, d in m["outputs"].items():
        assert present[name] == d, "%s: %s differs from the reference" % (case, name)


def check_reports(case, outdir):
    """JSON and HTML byte-identical to the reference's (run-dependent parts masked)."""
    for kind, mask in (("json", mask_software), ("html", mask_html)):
        with open(os.path.join(outdir, "report." + kind)) as f:
            got = mask(f.read())
        ref = mask(golden_text(case, kind))
        if got != ref:
            at = next(i for i in range(min(len(got), len(ref)) + 1) if got[i:i + 1] != ref[i:i + 1])
            raise AssertionError("%s: %s report differs at %d: ours ...%r... reference ...%r..." % (
                case, kind, at, got[max(0, at - 80):at + 80], ref[max(0, at - 80):at + 80]))


def case_inputs(case):
    """(in1, in2 or None, interleaved) of a fixture's command line."""
    a = manifest()[case]["args"].format(**{"in": INPUTS, "out": "OUT"}).split()
    in1 = a[a.index("-i") + 1]
    in2 = a[a.index("-I") + 1] if "-I" in a else None
    return in1, in2, "--in_fq_interleaved" in a


def case_sampling(case):
    a = manifest()[case]["args"].split()
    return int(a[a.index("--ora_sample") + 1]) if "--ora_sample" in a else DEFAULT_SAMPLING


SECTIONS = ("Read1BeforeFiltering", "Read2BeforeFiltering", "Read1AfterFiltering", "Read2AfterFiltering")


def report_sections(report):
    """The four Stats objects' JSON of a report (None where the run has none)."""
    out = []
    for name in SECTIONS:
        out.append(report.get(name))
    if report.get("MergedAndFiltered") is not None:
        out[2] = report["MergedAndFiltered"]
    return out


# ---- the host pipeline with the model as the counter ----------------------------------------------
def session_sets(host, s):
    on, smp, e1, e2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert host.fqh_session_ora_params(s, ctypes.byref(on), ctypes.byref(smp), ctypes.byref(e1), ctypes.byref(e2)) == 0
    sets = []
    for which in range(2):
        seq, off, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
        assert host.fqh_session_ora_hot_set(s, which, ctypes.byref(seq), ctypes.byref(off), ctypes.byref(n)) == 0
        o = np.ctypeslib.as_array(ctypes.cast(off, ctypes.POINTER(ctypes.c_uint32)), (n.value + 1,)).copy()
        data = ctypes.string_at(seq, int(o[-1])) if n.value else b""
        sets.append([data[o[i]:o[i + 1]] for i in range(n.value)])
    return bool(on.value), smp.value, e1.value, e2.value, sets


def run_session_ora(host, argv, process, max_n=1500):
    """e2e_util.run_session for an --ora command line: the model counts every pack from its batch
    and the records `process` returns, over the session's own hot sets, and its four blocks go in
    through fqh_session_set_ora before the reports are written.  Returns (JSON text, the session's
    sets, the model)."""
    from e2e_util import round16
    enc = [a.encode() for a in argv]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    s = ctypes.c_void_p()
    rc = host.fqh_session_open(len(enc), arr, ctypes.byref(s))
    try:
        assert rc == 0, host.fqh_session_error(s)
        p0 = abi.FqParams()
        host.fqh_session_params(s, 16, ctypes.byref(p0))
        on, smp, e1, e2, sets = session_sets(host, s)
        assert on
        model = Model(smp, e1, e2, sets[0], sets[1])
        kon, k = ctypes.c_int(), ctypes.c_int()
        host.fqh_session_kmer_params(s, ctypes.byref(kon), ctypes.byref(k))
        tables = K.Tables(k.value) if k.value else None  # (--kmer next to --ora)
        while True:
            b = abi.FqBatch()
            r = host.fqh_session_next(s, max_n, ctypes.byref(b))
            assert r >= 0, host.fqh_session_error(s)
            if r == 0:
                break
            n, paired = b.n, bool(b.seq2)
            l1 = np.ctypeslib.as_array(ctypes.cast(b.len1, ctypes.POINTER(ctypes.c_uint16)), (n,))
            need = int(l1.max()) if n else 0
            if paired:
                l2 = np.ctypeslib.as_array(ctypes.cast(b.len2, ctypes.POINTER(ctypes.c_uint16)), (n,))
                m2 = int(l2.max()) if n else 0
                need = need + m2 if p0.merge_enabled else max(need, m2)
            mc = max(16, round16(need))
            p = abi.FqParams()
            host.fqh_session_params(s, mc, ctypes.byref(p))
            res, acc = process(p, b, n * (2 if paired else 1), mc)
            if n:
                K.model_pack(K.BatchPack(b), p, res, 0, model)
                if tables is not None:
                    K.model_pack(K.BatchPack(b), p, res, k.value, tables)
            assert host.fqh_session_consume(s, res.ctypes.data, mc) == 0, host.fqh_session_error(s)
            host.fqh_session_add_acc(s, acc.ctypes.data, mc)
        if tables is not None:
            karr = tables.array()
            assert host.fqh_session_set_kmer(s, karr.ctypes.data) == 0
        blocks = model.array()
        assert host.fqh_session_set_ora(s, blocks.ctypes.data if blocks.size else None, blocks.size) == 0
        return abi.take_string(host, host.fqh_session_finish(s)), sets, model
    finally:
        host.fqh_session_close(s)


# ---- engine test inputs ---------------------------------------------------------------------------
def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def write_sim_input(path, pk, p, res, sampling, eval1, eval2, set1, set2, counts=(0, 0, 0, 0)):
    """A pack (and its records) in the input format of tools/micro/ora_sim.cpp."""
    head = np.array([0x4f524131, sampling, eval1, eval2, int(pk.paired), int(p.merge_enabled), int(p.discard_unmerged),
                     pk.n, pk.stride, 0 if res is None else 1, len(set1), len(set2)], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.array(counts, np.uint64).tobytes())
        for st in (set1, set2):
            data, off, _ = pack_set(st)
            f.write(off.tobytes())
            f.write(data[:int(off[-1])].tobytes())
        f.write(pk.len1.astype("<u2").tobytes())
        if pk.paired:
            f.write(pk.len2.astype("<u2").tobytes())
        f.write(np.ascontiguousarray(pk.seq1).tobytes())
        if pk.paired:
            f.write(np.ascontiguousarray(pk.seq2).tobytes())
        if res is not None:
            f.write(res.tobytes())


COMP = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")


@functools.lru_cache(maxsize=None)
def pools(seed=1):
    """The hot sets of the engine tests, (R1's, R2's), each in sorted order: every step's length, twice;
    members with N, lower-case and IUPAC bytes; 20-mers that share their 12 leading bytes (one hash
    chain); a length no step has."""
    rng = random.Random(seed)
    out = []
    for _ in range(2):
        hot = {rand_seq(rng, n) for n in (10, 10, 20, 20, 40, 40, 100, 100, 149, 149, 33)}
        hot |= {b"ACGTNACGgT", b"TTGNCAtGGACCTAaGTCAG", b"RYKMACGTACGTNNNNacgtACGTACGTACGTWSACGTAC"}
        lead = rand_seq(rng, 12)
        hot |= {lead + rand_seq(rng, 8) for _ in range(6)}
        out.append(tuple(sorted(hot)))
    return tuple(out)


def hot_pack(n, paired, seed, stride=160, read_len=151, sets=None):
    """n reads (pairs) with the pools' sequences planted: alone, twice back to back, twice with one
    byte between, several of different lengths overlapping; a third of the pairs overlap (the R1 set's
    sequences planted in the fragment, some across the end of read 1, so a merged read's hit spans the
    junction); about half the pairs have a low-quality mate and fail -q; some reads are short or empty."""
    from batch_util import Pack
    sets = sets or pools()
    rng = random.Random(seed)
    pk = Pack(n, stride, paired)

    def planted(s, pool):
        for _ in range(rng.choice((0, 1, 1, 2, 3))):
            h = rng.choice(pool)
            h = rng.choice((h, h, h + h, h + b"T" + h))
            if len(h) <= len(s):
                at = rng.randint(0, len(s) - len(h))
                s = s[:at] + h + s[at + len(h):]
        return s

    for i in range(n):
        L = rng.choice((read_len,) * 6 + (100, rng.randint(0, stride), stride))
        if paired and rng.random() < 0.35 and L >= 100:
            ins = rng.randint(L + 10, 2 * L - 35)
            frag = planted(rand_seq(rng, ins), sets[0])
            r = [frag[:L], frag[-L:].translate(COMP)[::-1]]
        else:
            r = [planted(rand_seq(rng, L), sets[0]), planted(rand_seq(rng, L), sets[1] or sets[0])]
        bad = rng.randrange(4)  # 0, 1: a low-quality mate
        for m in range(2 if paired else 1):
            q = b"#" * L if bad == m else b"I" * L
            pk.set(i, m + 1, r[m], q)
    return pk
