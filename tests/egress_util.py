"""Routed egress helpers: a Python restatement of the host's format_range
(fqtool_amd/host/processor.cpp; reference src/peprocessor.cpp:351-429, src/seprocessor.cpp:337-350)
over the six output streams of fq_engine_set_egress, from a pack's reads and the oracle's records;
the golden e2e cases that pin it to the reference; the input format of tools/micro/egress_sim.cpp."""
import gzip
import hashlib
import os

import numpy as np

import e2e_util as E
from fqtool_amd import abi
from kmer_util import _COMP, correct_pair

OUT1, OUT2, MERGED, UNPAIRED1, UNPAIRED2, FAILED = range(6)
STREAMS = 6
STREAM_NAMES = ["out1", "out2", "merged", "unpaired1", "unpaired2", "failed"]

# FilterResult's failed_type text (fqtool_amd/host/processor.cpp failed_type): "" for other codes
FAILED_TYPE = {0: b"passed", 4: b"failed_polyx_filter", 8: b"failed_bad_overlap", 12: b"failed_too_many_n_bases",
               16: b"failed_too_short", 17: b"failed_too_long", 20: b"failed_quality_filter",
               24: b"failed_low_complexity"}
MATE_FAILING = b"paired_read_is_failing"
LONGEST_TAG = 1 + len(MATE_FAILING)  # the blank and the tag: 23 bytes


def mask(*streams):
    m = 0
    for s in streams:
        m |= 1 << s
    return m


def merged_name(name, m1, m2):
    """OverlapAnalysis::merge's name (src/overlapanalysis.cpp:74-104; host merged_name)."""
    tag = b"_merged_%d_%d" % (m1, m2)
    pos = name.find(b" ")
    if pos < 0:
        return tag
    return name[:pos - 1] + tag + name[pos:]


class Reads:
    """One mate's reads: names, strand lines, sequence and quality bytes."""

    def __init__(self, names, strands, seqs, quals):
        self.names, self.strands, self.seqs, self.quals = names, strands, seqs, quals


def reads_of_pack(pk, mate, names, strands):
    lens = getattr(pk, "len%d" % mate)
    s, q = getattr(pk, "seq%d" % mate), getattr(pk, "qual%d" % mate)
    return Reads(names, strands, [s[i, :int(lens[i])].tobytes() for i in range(pk.n)],
                 [q[i, :int(lens[i])].tobytes() for i in range(pk.n)])


def model(reads, res, paired, merge, discard, open_mask):
    """The six streams (bytes each) of a pack: reads = [Reads] per mate, res = the oracle's records."""
    out = [bytearray() for _ in range(STREAMS)]
    NULL, IDX, MERGED_F, CORR = abi.FQ_RF_NULL, abi.FQ_RF_INDEX_FILTERED, abi.FQ_RF_MERGED, abi.FQ_RF_CORRECTED
    is_open = lambda s: (open_mask >> s) & 1

    def view(m, i, r, seq, qual):
        if int(r["flags"]) & NULL:
            return seq, qual
        a, n = int(r["start"]), int(r["len"])
        return seq[a:a + n], qual[a:a + n]

    def put(stream, m, i, seq, qual, tag=None, name=None):
        if not is_open(stream):
            return
        nm = reads[m].names[i] if name is None else name
        if tag is not None:
            nm = nm + b" " + tag
        out[stream] += nm + b"\n" + bytes(seq) + b"\n" + reads[m].strands[i] + b"\n" + bytes(qual) + b"\n"

    n = len(reads[0].names)
    if not paired:
        for i in range(n):
            r = res[i]
            if int(r["flags"]) & IDX:
                continue
            s, q = view(0, i, r, reads[0].seqs[i], reads[0].quals[i])
            if not (int(r["flags"]) & NULL) and int(r["code"]) == 0:
                put(OUT1, 0, i, s, q)
            else:
                put(FAILED, 0, i, s, q, FAILED_TYPE.get(int(r["code"]), b""))
        return [bytes(o) for o in out]
    left = is_open(UNPAIRED1)
    for i in range(n):
        a, b = res[2 * i], res[2 * i + 1]
        fa, fb = int(a["flags"]), int(b["flags"])
        if fa & IDX:
            continue
        s1, q1 = bytearray(reads[0].seqs[i]), bytearray(reads[0].quals[i])
        s2, q2 = bytearray(reads[1].seqs[i]), bytearray(reads[1].quals[i])
        if (fa | fb) & CORR:  # apply_corrections: the pair's text with the corrector's edits
            st1, st2 = int(a["start"]), int(b["start"])
            x1, y1, x2, y2 = s1[st1:], q1[st1:], s2[st2:], q2[st2:]
            correct_pair(x1, y1, x2, y2, int(np.int16(b["m_len1"])), int(b["m_len2"]), int(b["reserved"]))
            s1[st1:], q1[st1:], s2[st2:], q2[st2:] = x1, y1, x2, y2
        nn1, nn2 = not (fa & NULL), not (fb & NULL)
        v1, w1 = view(0, i, a, s1, q1)
        v2, w2 = view(1, i, b, s2, q2)
        ca, cb = int(a["code"]), int(b["code"])
        if merge and nn1 and nn2:
            if fa & MERGED_F:
                if ca == 0:
                    m1, m2 = int(a["m_len1"]), int(a["m_len2"])
                    ol = len(v2) - m2
                    rc = _COMP[np.frombuffer(bytes(v2), np.uint8)][::-1].tobytes()
                    put(MERGED, 0, i, bytes(v1[:m1]) + rc[ol:ol + m2], bytes(w1[:m1]) + bytes(w2)[::-1][ol:ol + m2],
                        name=merged_name(reads[0].names[i], m1, m2))
                continue
            if not discard:
                if ca == 0:
                    put(MERGED, 0, i, v1, w1)
                if cb == 0:
                    put(MERGED, 1, i, v2, w2)
                continue
        p1, p2 = nn1 and ca == 0, nn2 and cb == 0
        if p1 and p2:
            put(OUT1, 0, i, v1, w1)
            put(OUT2, 1, i, v2, w2)
        elif p1:
            if left:
                put(UNPAIRED1, 0, i, v1, w1)
                put(FAILED, 1, i, v2, w2, FAILED_TYPE.get(cb, b""))
            else:
                put(FAILED, 0, i, v1, w1, MATE_FAILING)
                put(FAILED, 1, i, v2, w2, FAILED_TYPE.get(cb, b""))
        elif p2:
            if left:  # the reference tests the left writer, and tags read 1 with read 2's code
                put(UNPAIRED2, 1, i, v2, w2)
                put(FAILED, 0, i, v1, w1, FAILED_TYPE.get(cb, b""))
            else:
                put(FAILED, 0, i, v1, w1, FAILED_TYPE.get(ca, b""))
                put(FAILED, 1, i, v2, w2, MATE_FAILING)
    return [bytes(o) for o in out]


# ---- the golden e2e cases that use these options (tests/golden/make_e2e.py) -------------------------
# --failed_out / --unpaired_read* / --discard_unmerged / -c, PE, SE and interleaved; no UMI, index
# filter or split.  (td_pe_unpaired_same names one file for both unpaired outputs: two streams into
# one file, which the model's separate streams do not describe.)
PINNED_CASES = ["edge_pe_all", "edge_pe_correct", "edge_pe_correct_front", "edge_se_all", "inter_pe", "synth_pe_correct_merge",
                "td_pe_all", "td_pe_correct", "td_pe_correct_only", "td_pe_failed_only", "td_pe_merge_discard", "td_se_all"]
OPTION_STREAM = {"-o": OUT1, "-O": OUT2, "--merge_output": MERGED, "--unpaired_read1": UNPAIRED1,
                 "--unpaired_read2": UNPAIRED2, "--failed_out": FAILED}


def read_fastq(path):
    """(names, sequences, strand lines, qualities) of a FASTQ file (.gz or plain), lines as the
    reference's reader leaves them (a trailing '\\r' dropped)."""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        lines = [l[:-1] if l.endswith(b"\r") else l for l in f.read().split(b"\n")]
    n = len(lines) // 4
    return lines[0:4 * n:4], lines[1:4 * n:4], lines[2:4 * n:4], lines[3:4 * n:4]


def case_args(case):
    return E.manifest()[case]["args"].format(**{"in": E.INPUTS, "out": "{out}"}).split()


def case_streams(case):
    """{stream: output file name} of a case's command line."""
    args = case_args(case)
    return {OPTION_STREAM[a]: os.path.basename(args[k + 1]) for k, a in enumerate(args) if a in OPTION_STREAM}


def case_mask(case):
    """The streams that have a writer: the files the case names, except that a paired run writes the
    pair outputs only with both writers (src/peprocessor.cpp:469; OutputSet::write)."""
    args, streams = case_args(case), set(case_streams(case))
    paired = "-I" in args or "--in_fq_interleaved" in args
    if paired and not {OUT1, OUT2} <= streams:
        streams -= {OUT1, OUT2}
    return mask(*streams)


def case_reads(case):
    """The case's input reads per mate: [Reads] (one entry for single end)."""
    args = case_args(case)
    n1, s1, t1, q1 = read_fastq(args[args.index("-i") + 1])
    if "--in_fq_interleaved" in args:
        return [Reads(n1[0::2], t1[0::2], s1[0::2], q1[0::2]), Reads(n1[1::2], t1[1::2], s1[1::2], q1[1::2])]
    if "-I" not in args:
        return [Reads(n1, t1, s1, q1)]
    n2, s2, t2, q2 = read_fastq(args[args.index("-I") + 1])
    return [Reads(n1, t1, s1, q1), Reads(n2, t2, s2, q2)]


def sha(data):
    return {"sha256": hashlib.sha256(data).hexdigest(), "lines": data.count(b"\n")}


def text_bytes(reads):
    """Bytes of the mate's input text with '\\n' terminators (what a pack of these records spans)."""
    return sum(len(a) + len(b) + len(c) + len(d) + 4 for a, b, c, d in zip(reads.names, reads.seqs, reads.strands, reads.quals))


# ---- tools/micro/egress_sim.cpp ---------------------------------------------------------------------
def fastq_of(reads):
    """FASTQ bytes of one mate's reads plus their fq_text_rec index."""
    parts, recs, off = [], [], 0
    for name, seq, strand, qual in zip(reads.names, reads.seqs, reads.strands, reads.quals):
        seq_off = off + len(name) + 1
        strand_off = seq_off + len(seq) + 1
        qual_off = strand_off + len(strand) + 1
        parts.append(name + b"\n" + seq + b"\n" + strand + b"\n" + qual + b"\n")
        recs.append((off, seq_off, strand_off, qual_off, len(name), len(strand), len(seq), 0))
        off += len(parts[-1])
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(recs, dtype=np.dtype(abi.TEXT_REC_DTYPE))


def write_sim_input(path, texts, res, paired, merge, discard, correction, open_mask, stride):
    """texts = [(text bytes array, fq_text_rec array)] per mate."""
    n = len(texts[0][1])
    head = np.array([0x45475231, int(paired), int(merge), int(discard), int(correction), open_mask, n, stride], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for text, recs in texts:
            f.write(np.array([text.size], np.uint64).tobytes())
            f.write(text.tobytes())
            f.write(recs.tobytes())
        f.write(res.tobytes())


def read_sim_output(path):
    data = open(path, "rb").read()
    sizes = np.frombuffer(data[:8 * STREAMS], np.uint64)
    out, at = [], 8 * STREAMS
    for s in range(STREAMS):
        out.append(data[at:at + int(sizes[s])])
        at += int(sizes[s])
    assert at == len(data)
    return out
