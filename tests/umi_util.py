"""UMI (-u) on the routed egress: a Python restatement of the tag, the tagged name and the NULL-read
cut (reference src/umiprocessor.cpp:10-89, src/read.h:106-123, :203-208; the host's umi_tag /
tagged_name / view in fqtool_amd/host/processor.cpp) around egress_util.model; the golden cases that
pin it to the reference (the UMI cases of tests/golden/e2e and tests/golden/umi, made by
tests/golden/make_umi.py); the synthetic pack of hostile names; the UMI input format of
tools/micro/egress_sim.cpp."""
import gzip
import json
import os
import random
from collections import namedtuple

import numpy as np

import e2e_util as E
import egress_util as G
from batch_util import config, edge_pack
from fqtool_amd import abi

UMI_DIR = os.path.join(E.GOLDEN, "umi")

# the UMI description (fq_umi)
Umi = namedtuple("Umi", "location length skip drop_comment not_trim")


# ---- the model ---------------------------------------------------------------------------------------
def umi_cut(k, length):
    """Read::trimFront of the UMI step: min(k, len - 1) bases, none of an empty read."""
    return min(k, length - 1) if k > 0 and length > 0 else 0


def umi_front(u, mate, paired):
    """Options::umi_front: the leading bases the UMI step cuts off mate 0 / 1, before clamping."""
    if u.not_trim:
        return 0
    r1, r2 = u.location in (3, 6), u.location in (4, 6) and paired
    return u.length + u.skip if (r1 if mate == 0 else r2) else 0


def first_index(name):
    """Read::firstIndex: backwards from len - 3, a '+' ends the index at the byte before it (kept by
    substr's count, sic), the first ':' starts it."""
    n = len(name)
    end = n
    if n < 5:
        return b""
    for i in range(n - 3, -1, -1):
        c = name[i:i + 1]
        if c == b"+":
            end = i - 1
        if c == b":":
            return name[i + 1:i + 1 + (end - i)]
    return b""


def umi_tag(u, reads, i):
    """UmiProcessor::process: the tag both names get, or b"" (no umi part: nothing is added)."""
    paired = len(reads) == 2
    umi, qua, L = b"", b"", u.length
    s1, q1 = reads[0].seqs[i], reads[0].quals[i]
    s2, q2 = (reads[1].seqs[i], reads[1].quals[i]) if paired else (b"", b"")
    if u.location == 1:
        umi = first_index(reads[0].names[i])
    elif u.location == 2:
        if paired:
            umi = first_index(reads[1].names[i])
    elif u.location == 3:
        umi, qua = s1[:min(len(s1), L)], q1[:min(len(s1), L)]
    elif u.location == 4:
        if paired:
            umi, qua = s2[:min(len(s2), L)], q2[:min(len(s1), L, len(s2))]  # sic: read 1's length
    elif u.location == 5:
        umi = first_index(reads[0].names[i])
        if paired:
            umi += b"-" + first_index(reads[1].names[i])
    elif u.location == 6:
        umi, qua = s1[:min(len(s1), L)], q1[:min(len(s1), L)]
        if paired:  # read 2's quality part after its cut, bounded by read 1's cut length
            front = 0 if u.not_trim else L + u.skip
            c1, c2 = umi_cut(front, len(s1)), umi_cut(front, len(s2))
            umi += b"-" + s2[:min(len(s2), L)]
            qua += b"-" + q2[c2:c2 + min(len(s1) - c1, L, len(s2) - c2)]
    if not umi:
        return b""
    return b" OX:Z:" + umi + (b" BZ:Z:" + qua if qua else b"")


def tagged_name(name, tag, drop_comment):
    """UmiProcessor::addTagToName."""
    pos = name.find(b" ")
    if pos < 0:
        return name + tag
    return name[:pos] + tag + (b"" if drop_comment else name[pos:])


def tagged_reads(reads, res, u):
    """The reads as the loop body sees them after the UMI step: tagged names, and a FQ_RF_NULL read
    (which the model writes whole) without its UMI cut.  Other reads keep their bytes: their
    records' windows count from the untrimmed read."""
    paired = len(reads) == 2
    mates = len(reads)
    out = [G.Reads(list(r.names), r.strands, list(r.seqs), list(r.quals)) for r in reads]
    for i in range(len(reads[0].names)):
        tag = umi_tag(u, reads, i)
        for m in range(mates):
            if tag:
                out[m].names[i] = tagged_name(reads[m].names[i], tag, u.drop_comment)
            if int(res[mates * i + m]["flags"]) & abi.FQ_RF_NULL:
                c = umi_cut(umi_front(u, m, paired), len(reads[m].seqs[i]))
                out[m].seqs[i], out[m].quals[i] = reads[m].seqs[i][c:], reads[m].quals[i][c:]
    return out


def model(reads, res, paired, merge, discard, open_mask, u):
    """The six streams of a pack with the UMI description u (None: egress_util.model as it is)."""
    if u is None:
        return G.model(reads, res, paired, merge, discard, open_mask)
    return G.model(tagged_reads(reads, res, u), res, paired, merge, discard, open_mask)


# ---- the golden cases ------------------------------------------------------------------------------
def umi_manifest():
    with open(os.path.join(UMI_DIR, "manifest.json")) as f:
        return json.load(f)


def _has_umi(args):
    return " -u " in " " + args + " "


# every reference run with -u that exits 0: (manifest, name)
OLD_CASES = sorted(k for k, v in E.manifest().items() if v["exit"] == 0 and _has_umi(v["args"]))
NEW_CASES = sorted(umi_manifest())
ALL_CASES = [("e2e", c) for c in OLD_CASES] + [("umi", c) for c in NEW_CASES]
CASE_IDS = ["%s-%s" % c for c in ALL_CASES]


def entry(case):
    return (E.manifest() if case[0] == "e2e" else umi_manifest())[case[1]]


def case_args(case):
    return entry(case)["args"].format(**{"in": E.INPUTS, "out": "{out}"}).split()


def argv_for(binary, case, outdir):
    argv = [binary, "-w", "1", "-J", os.path.join(outdir, "report.json"), "-H", os.path.join(outdir, "report.html")]
    return argv + entry(case)["args"].format(**{"in": E.INPUTS, "out": outdir}).split()


def case_umi(case):
    args = case_args(case)
    val = lambda opt: int(args[args.index(opt) + 1]) if opt in args else 0
    return Umi(val("--umi_location"), val("--umi_length"), val("--umi_skip_length"), int("--umi_drop_comment" in args),
               int("--umi_not_trim" in args))


def case_streams(case):
    args = case_args(case)
    return {G.OPTION_STREAM[a]: os.path.basename(args[k + 1]) for k, a in enumerate(args) if a in G.OPTION_STREAM}


def case_mask(case):
    """As egress_util.case_mask: a paired run writes the pair outputs only with both writers."""
    args, streams = case_args(case), set(case_streams(case))
    if "-I" in args and not {G.OUT1, G.OUT2} <= streams:
        streams -= {G.OUT1, G.OUT2}
    return G.mask(*streams)


def case_reads(case):
    args = case_args(case)
    n1, s1, t1, q1 = G.read_fastq(args[args.index("-i") + 1])
    if "-I" not in args:
        return [G.Reads(n1, t1, s1, q1)]
    n2, s2, t2, q2 = G.read_fastq(args[args.index("-I") + 1])
    return [G.Reads(n1, t1, s1, q1), G.Reads(n2, t2, s2, q2)]


def check_outputs(case, outdir):
    """E.check_outputs for either manifest: every output file and both reports equal the reference's."""
    if case[0] == "e2e":
        return E.check_outputs(case[1], outdir)
    m = entry(case)
    present = {n: E.digest(os.path.join(outdir, n)) for n in sorted(os.listdir(outdir)) if not n.startswith("report.")}
    assert sorted(present) == sorted(m["outputs"]), (sorted(present), sorted(m["outputs"]))
    for name, d in m["outputs"].items():
        assert present[name] == d, "%s: %s differs from the reference (%s vs %s lines)" % (
            case[1], name, present[name]["lines"], d["lines"])
    for kind, mask in (("html", E.mask_html), ("json", E.mask_software)):
        with gzip.open(os.path.join(UMI_DIR, m[kind]), "rt") as f:
            ref = mask(f.read())
        with open(os.path.join(outdir, "report." + kind)) as f:
            got = mask(f.read())
        assert got == ref, "%s: the %s report differs from the reference" % (case[1], kind)


# ---- the synthetic pack -----------------------------------------------------------------------------
SYNTH_PAIRS = 700
SYNTH_CONFIGS = ["PE_umi", "PE_umi_merge", "PE_correct_umi_merge", "SE_umi"]
PAIR, UNP, FAIL, MRG = G.mask(G.OUT1, G.OUT2), G.mask(G.UNPAIRED1, G.UNPAIRED2), G.mask(G.FAILED), G.mask(G.MERGED)
# the streams with a writer per config
SYNTH_MASK = {"PE_umi": PAIR | UNP | FAIL, "PE_umi_merge": MRG, "PE_correct_umi_merge": MRG, "SE_umi": G.mask(G.OUT1) | FAIL}


def hostile_name(rng, i, mate):
    """Names that reach every branch of Read::firstIndex and addTagToName."""
    kind = rng.randrange(12)
    tail = b"/%d" % mate
    return [
        lambda: b"@" + bytes(rng.choice(b"ab:+ ") for _ in range(rng.randint(0, 3))),  # shorter than 5 bytes
        lambda: b"@read%d%s" % (i, tail),                                   # no ':' and no blank
        lambda: b"@read%d%s with a comment" % (i, tail),                    # no ':', blank plus comment
        lambda: b"@M0:7:%d %d:N:0:ACGTAC" % (i, mate),                      # one index
        lambda: b"@M0:7:%d %d:N:0:ACGTAC+TTGCAA" % (i, mate),               # two indexes
        lambda: b"@M0:7:%d %d:N:0:ACG+TT" % (i, mate),                      # '+' at len - 3, where the scan starts
        lambda: b"@M0:7:%d %d:N:0:ACGT+T" % (i, mate),                      # '+' at len - 2: never seen
        lambda: b"@M0:7:%d %d:N:0:AC+GTT" % (i, mate),                      # '+' at len - 4
        lambda: b"@M0:7:%d:ACGT+TTAG%d" % (i, mate),                        # indexes, no blank
        lambda: b"@M0:7:%d %d:N:0:+ACGT" % (i, mate),                       # '+' right after the ':'
        lambda: b"@M0:7:%d %d:N:0:A:C" % (i, mate),                         # ':' in the last two bytes
        lambda: b"@M0 7 %d+x:%d  two  blanks" % (i, mate),                  # '+' before the only ':', several blanks
    ][kind]()


def synth_texts(pk, seed=23, crlf=True):
    """Per mate (text, fq_text_rec index, names, strands) of the pack's reads under hostile names: the
    mates' names differ (their kinds too, for a third of the pairs); with crlf a tenth of the records
    end their lines in CRLF (text packs take them; the raw stream stops at one)."""
    rng = random.Random(seed)
    mates = (1, 2) if pk.paired else (1,)
    names = {m: [] for m in mates}
    for i in range(pk.n):
        state = rng.getstate()
        for m in mates:
            if m == 2 and rng.random() < 0.67:
                rng.setstate(state)  # the same kind as read 1's name
            names[m].append(hostile_name(rng, i, m))
    out = []
    for m in mates:
        seqs, quals, lens = getattr(pk, "seq%d" % m), getattr(pk, "qual%d" % m), getattr(pk, "len%d" % m)
        parts, recs, strands, off = [], [], [], 0
        for i in range(pk.n):
            L = int(lens[i])
            name = names[m][i]
            strand = b"+" if rng.random() < 0.8 else b"+r%d" % i
            eol = b"\r\n" if crlf and rng.random() < 0.1 else b"\n"
            seq_off = off + len(name) + len(eol)
            strand_off = seq_off + L + len(eol)
            qual_off = strand_off + len(strand) + len(eol)
            rec = name + eol + seqs[i, :L].tobytes() + eol + strand + eol + quals[i, :L].tobytes() + eol
            parts.append(rec)
            recs.append((off, seq_off, strand_off, qual_off, len(name), len(strand), L, 0))
            strands.append(strand)
            off += len(rec)
        out.append((np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(recs, dtype=np.dtype(abi.TEXT_REC_DTYPE)),
                    names[m], strands))
    return out


def synth_pack_and_texts(paired, crlf=True, min_len=0):
    """batch_util.edge_pack reads (lengths from 0 up, read 2 both shorter and longer than read 1).
    min_len = 1 gives the empty reads one base: the raw stream takes records whose four lines are
    non-empty (include/fqengine.h) and stops at any other."""
    pk = edge_pack(SYNTH_PAIRS, paired, seed=31)
    for m in ((1, 2) if paired else (1,)):
        for i in np.flatnonzero(getattr(pk, "len%d" % m) < min_len):
            pk.set(int(i), m, b"A" * min_len, b"I" * min_len)
    return pk, synth_texts(pk, crlf=crlf)


def synth_umis():
    """Every location x drop_comment x not_trim."""
    return [(loc, drop, keep) for loc in range(1, 7) for drop in (0, 1) for keep in (0, 1)]


def synth_params(cfg, loc, drop, not_trim):
    """The config with its UMI length + skip kept (read 1's umi_front) and umi_front1/2 as the
    description implies them; returns (params, description)."""
    p = config(cfg, max_cycles=512)
    front = int(p.umi_front1)
    u = Umi(loc, front - 2, 2, drop, not_trim)
    p.umi_front1, p.umi_front2 = umi_front(u, 0, bool(p.paired)), umi_front(u, 1, bool(p.paired))
    return p, u


def fq_umi(u):
    """(location 0, -u without --umi_location, is no description: the engine refuses it)"""
    return abi.FqUmi(u.location, u.length, u.skip, u.drop_comment, u.not_trim)


# ---- tools/micro/egress_sim.cpp, the UMI input format -------------------------------------------------
def write_sim_input(path, texts, res, paired, merge, discard, correction, open_mask, stride, u):
    n = len(texts[0][1])
    head = np.array([0x45475532, int(paired), int(merge), int(discard), int(correction), open_mask, n, stride,
                     u.location, u.length, u.skip, u.drop_comment, u.not_trim], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for text, recs in texts:
            f.write(np.array([text.size], np.uint64).tobytes())
            f.write(text.tobytes())
            f.write(recs.tobytes())
        f.write(res.tobytes())
