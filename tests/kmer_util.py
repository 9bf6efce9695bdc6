"""--kmer helpers: a numpy model of the reference's k-mer counting (Stats::statRead, reference
src/stats.cpp:245,266-274, Evaluator::seq2int), the model of which reads feed which of the four
tables given a pack and its records, and the fixtures written by tests/golden/make_kmer.py."""
import gzip
import hashlib
import json
import os
import random

import numpy as np

from fqtool_amd import abi
from e2e_util import GOLDEN, INPUTS, digest, mask_html, mask_software

KMER = os.path.join(GOLDEN, "kmer")
MIN_K, MAX_K = 4, 12  # FQ_KSTAT_MIN_K, FQ_KSTAT_MAX_K (include/fqengine.h)
LDS_MAX_K = 7         # largest k whose tables the kernels keep in LDS (fqtool_amd/csrc/kstat.hip)

_CODE = np.full(256, -1, np.int64)
for _c, _v in zip(b"ATCG", range(4)):
    _CODE[_c] = _v
_COMP = np.full(256, ord("N"), np.uint8)  # util::complement, reference src/util.h:438-451
for _a, _b in zip(b"ATCGatcg", b"TAGCTAGC"):
    _COMP[_a] = _b


def read_keys(seq, k):
    """Keys of every window of k consecutive upper-case A/T/C/G bytes of `seq` (bytes or uint8
    array): base 4, A0 T1 C2 G3, first base most significant."""
    s = np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else seq
    n = len(s) - k + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    code = _CODE[s]
    bad = np.concatenate(([0], np.cumsum(code < 0)))
    ok = (bad[k:] - bad[:-k]) == 0
    key = np.zeros(n, np.int64)
    for j in range(k):
        key = key * 4 + np.maximum(code[j:j + n], 0)
    return key[ok]


class Tables:
    """The four KmerCount tables [pre-R1 | pre-R2 | post-R1 | post-R2] of 4^k counters.  The reads
    of a table are kept end to end with a '.' between them (no window spans it) and counted once."""

    def __init__(self, k):
        self.k = k
        self.text = [bytearray(), bytearray(), bytearray(), bytearray()]

    def add(self, table, seq):
        if len(seq) >= self.k:
            self.text[table] += bytes(seq) + b"."

    def array(self):
        size = 4 ** self.k
        out = np.zeros((4, size), np.uint64)
        for t in range(4):
            keys = read_keys(self.text[t], self.k)
            if len(keys):
                out[t] = np.bincount(keys, minlength=size).astype(np.uint64)
        return out.reshape(-1)


def key_text(key, k):
    """Evaluator::int2seq."""
    return "".join("ATCG"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))


def table_from_json(obj, k):
    """A report's KmerCount object -> counts by key."""
    assert len(obj) == 4 ** k
    out = np.zeros(4 ** k, np.uint64)
    for key in range(4 ** k):
        out[key] = int(obj[key_text(key, k)])
    return out


def fastq_seqs(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        lines = f.read().split(b"\n")
    return lines[1::4][:len(lines) // 4]


def correct_pair(s1, q1, s2, q2, offset, ol, len2):
    """fq_correct_pair_text (include/fqengine.h) on bytearrays that start at the records' starts."""
    start1 = max(offset, 0)
    start2 = len2 - (-offset if offset < 0 else 0) - 1
    good, bad = 33 + 30, 33 + 14
    sq = lambda v: v - 256 if v > 127 else v
    for i in range(ol):
        p1, p2 = start1 + i, start2 - i
        if s1[p1] == _COMP[s2[p2]]:
            continue
        if sq(q1[p1]) >= good and sq(q2[p2]) <= bad:
            s2[p2] = _COMP[s1[p1]]
            q2[p2] = q1[p1]
        elif sq(q2[p2]) >= good and sq(q1[p1]) <= bad:
            s1[p1] = _COMP[s2[p2]]
            q1[p1] = q2[p2]


def model_pack(pk, p, res, k, tables=None):
    """Adds one pack to the model tables: the original reads to the pre tables, and to the post
    tables what the records `res` (the oracle's) say reached the post-filter statRead (reference
    src/peprocessor.cpp:351-403, src/seprocessor.cpp:339-345)."""
    t = tables if tables is not None else Tables(k)
    PASS = 0
    for i in range(pk.n):
        l1 = int(pk.len1[i])
        s1 = bytearray(pk.seq1[i, :l1].tobytes())
        t.add(0, s1)
        if not pk.paired:
            r = res[i]
            if r["flags"] & (abi.FQ_RF_NULL | abi.FQ_RF_INDEX_FILTERED) or r["code"] != PASS:
                continue
            t.add(2, s1[int(r["start"]):int(r["start"]) + int(r["len"])])
            continue
        l2 = int(pk.len2[i])
        s2 = bytearray(pk.seq2[i, :l2].tobytes())
        t.add(1, s2)
        r1, r2 = res[2 * i], res[2 * i + 1]
        if (r1["flags"] | r2["flags"]) & (abi.FQ_RF_NULL | abi.FQ_RF_INDEX_FILTERED):
            continue
        st1, n1, st2, n2 = int(r1["start"]), int(r1["len"]), int(r2["start"]), int(r2["len"])
        if (r1["flags"] | r2["flags"]) & abi.FQ_RF_CORRECTED:
            q1 = bytearray(pk.qual1[i, :l1].tobytes())
            q2 = bytearray(pk.qual2[i, :l2].tobytes())
            a, qa, b, qb = s1[st1:], q1[st1:], s2[st2:], q2[st2:]
            correct_pair(a, qa, b, qb, int(np.int16(r2["m_len1"])), int(r2["m_len2"]), int(r2["reserved"]))
            s1[st1:], s2[st2:] = a, b
        w1, w2 = s1[st1:st1 + n1], s2[st2:st2 + n2]
        if p.merge_enabled:
            if r1["flags"] & abi.FQ_RF_MERGED:
                if r1["code"] == PASS:
                    m1, m2 = int(r1["m_len1"]), int(r1["m_len2"])
                    rc2 = _COMP[np.frombuffer(bytes(w2), np.uint8)][::-1].tobytes()
                    ol = n2 - m2
                    t.add(2, bytes(w1[:m1]) + rc2[ol:ol + m2])
            elif not p.discard_unmerged:
                if r1["code"] == PASS:
                    t.add(2, w1)
                if r2["code"] == PASS:
                    t.add(3, w2)
        elif r1["code"] == PASS and r2["code"] == PASS:
            t.add(2, w1)
            t.add(3, w2)
    return t


# ---- fixtures (tests/golden/kmer, written by tests/golden/make_kmer.py) -------------------------
def manifest():
    with open(os.path.join(KMER, "manifest.json")) as f:
        return json.load(f)


def ok_cases():
    return sorted(c for c, v in manifest().items() if v["exit"] == 0)


def argv_for(binary, case, outdir, extra=()):
    args = manifest()[case]["args"]
    argv = [binary, "-w", "1", "-J", os.path.join(outdir, "report.json"), "-H", os.path.join(outdir, "report.html")]
    return argv + list(extra) + args.format(**{"in": INPUTS, "out": outdir}).split()


def golden_text(case, kind):
    with gzip.open(os.path.join(KMER, manifest()[case][kind]), "rt") as f:
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
    """JSON and HTML byte-identical to the reference's (run-dependent parts masked), or equal to
    the recorded sha256 of the masked text where the fixture keeps only that."""
    m = manifest()[case]
    for kind, mask in (("json", mask_software), ("html", mask_html)):
        with open(os.path.join(outdir, "report." + kind)) as f:
            got = mask(f.read())
        if m.get(kind):
            ref = mask(golden_text(case, kind))
            if got != ref:
                at = next(i for i in range(min(len(got), len(ref)) + 1) if got[i:i + 1] != ref[i:i + 1])
                raise AssertionError("%s: %s report differs at %d: ours ...%r... reference ...%r..." % (
                    case, kind, at, got[max(0, at - 80):at + 80], ref[max(0, at - 80):at + 80]))
        else:
            assert hashlib.sha256(got.encode()).hexdigest() == m[kind + "_sha256"], \
                "%s: %s report differs from the reference's sha256" % (case, kind)


def check_outputs(case, outdir):
    check_files(case, outdir)
    check_reports(case, outdir)


# ---- engine test inputs ---------------------------------------------------------------------------
def length_pack(k, paired, stride=160):
    """Reads of length 0 .. k + 1 and across the 16-byte chunk boundaries, all A/C/G/T, then a
    2k-long read with an N, a lower-case and an IUPAC byte at each position in turn."""
    from batch_util import Pack
    rng = random.Random(1000 + k)
    lens = list(range(0, k + 2)) + [15, 16, 17, 31, 32, 33, 47, 48, 49]
    reads = [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in lens]
    base = bytes(rng.choice(b"ACGT") for _ in range(2 * k))
    for pos in range(2 * k):
        for bad in b"NaR":
            reads.append(base[:pos] + bytes([bad]) + base[pos + 1:])
    pk = Pack(len(reads), stride, paired)
    for i, s in enumerate(reads):
        pk.set(i, 1, s, b"I" * len(s))
        if paired:
            s2 = reads[(i * 7 + 3) % len(reads)]
            pk.set(i, 2, s2, b"I" * len(s2))
    return pk


def junction_pack(n=64, stride=160, seed=5):
    """Overlapping pairs whose read 2 holds N / lower-case / IUPAC bytes in the part that the merge
    appends (complemented to N, or to an upper-case base), next to the junction."""
    from batch_util import Pack
    rng = random.Random(seed)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    pk = Pack(n, stride, True)
    for i in range(n):
        L = 100
        ins = rng.randint(110, 170)  # insert longer than the reads: offset > 0, read 2 adds ins - L bases
        frag = bytes(rng.choice(b"ACGT") for _ in range(ins))
        r1 = frag[:L]
        r2 = bytearray(frag[ins - L:].translate(comp)[::-1])
        # read 2's first ins - L bases become the merged read's tail, the last of them at the junction
        extra = ins - L
        pos = extra - 1 - (i % min(extra, 8))
        r2[pos] = b"NnaRc"[i % 5]
        q = b"I" * L
        pk.set(i, 1, r1, q)
        pk.set(i, 2, bytes(r2), q)
    return pk


def write_sim_input(path, pk, p, res, k):
    """A pack (and its records) in the input format of tools/micro/kstat_sim.cpp."""
    head = np.array([0x4b535431, k, int(pk.paired), int(p.merge_enabled), int(p.discard_unmerged), pk.n, pk.stride,
                     0 if res is None else 1], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(pk.len1.astype("<u2").tobytes())
        if pk.paired:
            f.write(pk.len2.astype("<u2").tobytes())
        f.write(np.ascontiguousarray(pk.seq1).tobytes())
        if pk.paired:
            f.write(np.ascontiguousarray(pk.seq2).tobytes())
        if res is not None:
            f.write(res.tobytes())


class BatchPack:
    """The rows of an fq_batch in host memory, as batch_util.Pack holds them (for model_pack)."""

    def __init__(self, b):
        import ctypes
        self.n, self.stride, self.paired = b.n, b.stride, bool(b.seq2)
        nbytes = abi.batch_bytes(b.n, b.stride)

        def rows(ptr):
            plane = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8)), (nbytes,))
            return abi.untile_rows(plane, b.n, b.stride)

        def lens(ptr):
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint16)), (b.n,)).copy()
        self.seq1, self.qual1, self.len1 = rows(b.seq1), rows(b.qual1), lens(b.len1)
        if self.paired:
            self.seq2, self.qual2, self.len2 = rows(b.seq2), rows(b.qual2), lens(b.len2)


def run_session_kmer(host, argv, process, model=True, max_n=1500):
    """e2e_util.run_session for a --kmer command line: the numpy model counts every pack from its
    batch and the records `process` returns, and its four tables go in through fqh_session_set_kmer
    before the reports are written.  Returns (JSON text, effective k, the tables or None)."""
    import ctypes
    from e2e_util import round16
    enc = [a.encode() for a in argv]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    s = ctypes.c_void_p()
    rc = host.fqh_session_open(len(enc), arr, ctypes.byref(s))
    try:
        assert rc == 0, host.fqh_session_error(s)
        p0 = abi.FqParams()
        host.fqh_session_params(s, 16, ctypes.byref(p0))
        on, k = ctypes.c_int(), ctypes.c_int()
        host.fqh_session_kmer_params(s, ctypes.byref(on), ctypes.byref(k))
        tables = Tables(k.value) if model and k.value else None
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
            if tables is not None and n:
                model_pack(BatchPack(b), p, res, k.value, tables)
            assert host.fqh_session_consume(s, res.ctypes.data, mc) == 0, host.fqh_session_error(s)
            host.fqh_session_add_acc(s, acc.ctypes.data, mc)
        arr = None
        if tables is not None:
            arr = tables.array()
            assert host.fqh_session_set_kmer(s, arr.ctypes.data) == 0
        return abi.take_string(host, host.fqh_session_finish(s)), k.value, arr
    finally:
        host.fqh_session_close(s)
