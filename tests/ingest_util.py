"""Device ingest helpers: a Python restatement of the index filter (Filter::match / filterByIndex,
reference src/filter.cpp:191-232, over Read::firstIndex), of --phred64 (Read::convertPhred64To33,
src/read.h:71-75) and of the pack cuts of split outputs (the pieces fq_engine_next_cuts describes,
and what ThreadConfig::markProcessed / writeEmptyFilesForSplitting, src/threadconfig.cpp:88-137, make
of them at -w 1); the golden e2e cases that pin it to the reference; the synthetic lists and packs of
the GPU tests; the input format of tools/micro/ingest_sim.cpp."""
from collections import namedtuple

import numpy as np

import egress_util as G
import umi_util as U
from batch_util import Pack
from fqtool_amd import abi

INDEX_CASES = ["td_pe_index", "td_pe_index_diff1", "td_pe_index_nofile", "td_pe_dup_hist2", "td_se_index"]
PHRED64_CASES = ["edge64_pe"]
SPLIT_CASES = ["td_pe_split_num", "td_pe_split_num_gz", "td_se_split_lines", "td_se_split_num_many"]

Cut = namedtuple("Cut", "bytes0 bytes1 items passed")
# the configs of the synthetic-pack tests (paired -> name): adapter and quality trimming, some pairs pass
SYNTH_CFG = {True: "C3", False: "SE_adapter"}


# ---- the model ---------------------------------------------------------------------------------------
def match(entries, index, threshold):
    """Filter::match: some entry differs from the index in at most `threshold` of their first
    min(len(entry), len(index)) bytes."""
    for s in entries:
        diff = 0
        for k in range(min(len(s), len(index))):
            if s[k] != index[k]:
                diff += 1
                if diff > threshold:
                    break
        if diff <= threshold:
            return True
    return False


def index_flags(reads, list1, list2, threshold):
    """FQ_BF_* flags per record: list 1 against read 1's first index, then (paired) list 2 against
    read 2's."""
    n = len(reads[0].names)
    out = np.zeros(n, np.uint8)
    for i in range(n):
        hit = match(list1, U.first_index(reads[0].names[i]), threshold)
        if not hit and len(reads) == 2:
            hit = match(list2, U.first_index(reads[1].names[i]), threshold)
        out[i] = abi.FQ_BF_INDEX_FILTERED if hit else 0
    return out


def phred64(qual):
    """max(33, (signed char)q - 31) per byte."""
    q = np.frombuffer(bytes(qual), np.int8).astype(np.int16) - 31
    return np.maximum(q, 33).astype(np.uint8).tobytes()


def phred64_reads(reads):
    return [G.Reads(r.names, r.strands, r.seqs, [phred64(q) for q in r.quals]) for r in reads]


def out_sizes(reads, res):
    """text_size_kernel: per mate the bytes each record adds to OUT1 / OUT2 (a pair is written when both
    reads pass, a single read when it passes)."""
    mates, n = len(reads), len(reads[0].names)
    bad = abi.FQ_RF_NULL | abi.FQ_RF_INDEX_FILTERED
    ok = ((res["flags"] & bad) == 0) & (res["code"] == 0)
    ok = ok.reshape(n, mates).all(axis=1)
    sizes = []
    for m in range(mates):
        z = np.zeros(n, np.uint32)
        for i in np.flatnonzero(ok):
            z[i] = len(reads[m].names[i]) + len(reads[m].strands[i]) + 2 * int(res[mates * i + m]["len"]) + 4
        sizes.append(z)
    return sizes


def cuts_count(every, first, n):
    return (first + n - 1) // every - first // every + 1 if n else 0


def cut_table(sizes, every, first):
    """The pieces of a pack whose first record has global index `first`, cut in front of every record
    whose global index is a multiple of `every`."""
    n = len(sizes[0])
    out, lo = [], 0
    while lo < n:
        hi = min(n, (first + lo) // every * every + every - first)
        b = [int(z[lo:hi].sum()) for z in sizes] + [0]
        out.append(Cut(b[0], b[1], hi - lo, int(np.count_nonzero(sizes[0][lo:hi]))))
        lo = hi
    return out


def split_files(packs, out_names, pack_items, by_lines, split_size, split_number):
    """The numbered files of a split run at -w 1.  packs: per device pack (first_item, [stream per
    mate], its cut table); out_names: the -o (and -O) base names.  Pieces of one reference pack
    (global index // pack_items) are one markProcessed step."""
    files, working, cur = {}, 0, 0

    def open_files():
        for nm in out_names:
            files["%04d.%s" % (working + 1, nm)] = bytearray()
    open_files()
    ref, count, passed = None, 0, 0

    def finish():
        nonlocal working, cur
        if ref is None:
            return
        cur += passed if by_lines else count
        if cur >= split_size and (by_lines or working + 1 < split_number):
            working += 1
            open_files()
            cur = 0
    for first, streams, cuts in packs:
        at, o = first, [0] * len(out_names)
        for c in cuts:
            if ref != at // pack_items:
                finish()
                ref, count, passed = at // pack_items, 0, 0
            for m, nm in enumerate(out_names):
                b = (c.bytes0, c.bytes1)[m]
                files["%04d.%s" % (working + 1, nm)] += streams[m][o[m]:o[m] + b]
                o[m] += b
            count += c.items
            passed += c.passed
            at += c.items
        assert o == [len(s) for s in streams[:len(out_names)]]
    finish()
    if not by_lines:  # writeEmptyFilesForSplitting
        while working + 1 < split_number:
            working += 1
            open_files()
    return {k: bytes(v) for k, v in files.items()}


# ---- the golden cases --------------------------------------------------------------------------------
def case_option(case, opt, default=None):
    args = G.case_args(case)
    return args[args.index(opt) + 1] if opt in args else default


def read_list(path):
    """Options::index_list: the file's lines as std::getline gives them."""
    if path is None:
        return []
    data = open(path, "rb").read()
    lines = data.split(b"\n")
    return lines[:-1] if lines[-1] == b"" else lines


def case_lists(case):
    return (read_list(case_option(case, "--index1_file")), read_list(case_option(case, "--index2_file")),
            int(case_option(case, "--max_diff_for_match", 0)))


# ---- synthetic lists (over umi_util.synth_pack_and_texts's hostile names) -------------------------------
# name -> (list 1, list 2, threshold).  The hostile names' first indexes are "ACGTAC", "ACG", "ACGT", "ACGT+T",
# "AC", "A:C", "<mate>  two  blanks" and, for over a third of the names, the empty index; an empty index matches
# any non-empty list and an entry matches on the shorter of the two lengths, so every non-degenerate list drops
# most records and must keep some (tests/test_ingest_cpu.py and the GPU tests assert 0 < dropped < n).
LONG = b"ACGTACGGTTAACCGGTT"  # longer than any index
HIGH = b"AC\xc7T"             # a byte >= 128
SYNTH_LISTS = {
    "exact0": ([b"ACGTAC", LONG[::-1]], [b"TTTT"], 0),
    "long0": ([LONG], [LONG + b"A"], 0),                # an entry longer than any index: its prefix decides
    "prefix0": ([b"AC"], [b"2 "], 0),                   # 2-byte prefix entries
    "high1": ([HIGH, b"GGGGGGGG"], [HIGH], 1),          # a byte >= 128, one mismatch allowed
    "far10": ([b"TTTTTTTTTTTTTTTTTT"], [], 10),         # threshold 10: every index of <= 10 bytes matches
    "list2only1": ([], [b"ACGTAC+"], 1),                # list 1 empty: paired runs drop by read 2 alone
    "empty_entry0": ([b"GGGG", b""], [b"GGGG"], 0),     # an empty entry matches every record (degenerate)
    "none": ([], [], 0),                                # the empty lists: nothing dropped (degenerate)
}
DEGENERATE = {"empty_entry0": "all", "none": "none"}


def big_list(n=3000):
    """Above 32 KiB of offsets and bytes: n 12-byte entries no index resembles, then the one that matches."""
    rng = np.random.RandomState(5)
    body = [bytes(rng.choice(list(b"GT"), 12).tolist()) for _ in range(n)]
    return body + [b"ACGTAC"]


def fq_index_filter(list1, list2, threshold):
    """(FqIndexFilter, the arrays it points to)."""
    f, keep = abi.FqIndexFilter(), []
    for m, lst in enumerate((list1, list2)):
        data = np.frombuffer(b"".join(lst), np.uint8).copy() if lst else np.zeros(0, np.uint8)
        off = np.zeros(len(lst) + 1, np.uint32)
        off[1:] = np.cumsum([len(s) for s in lst])
        keep += [data, off]
        f.list[m], f.off[m], f.n[m] = (data.ctypes.data if data.size else None), off.ctypes.data, len(lst)
    f.threshold = threshold
    return f, keep


def with_flags(res, flags, mates):
    """The oracle's records for a pack whose per-record flags are `flags`: helper for expectations that
    only need the FQ_RF_INDEX_FILTERED bit replaced."""
    out = res.copy()
    idx = np.repeat(flags != 0, mates)
    out["flags"] = np.where(idx, out["flags"] | abi.FQ_RF_INDEX_FILTERED, out["flags"] & ~np.uint8(abi.FQ_RF_INDEX_FILTERED))
    return out


# ---- tools/micro/ingest_sim.cpp ------------------------------------------------------------------------
def write_sim_input(path, texts, paired, stride, lists, sizes, every, first, convert):
    """texts = [(text bytes array, fq_text_rec array)] per mate; lists = (list 1, list 2, threshold)."""
    n = len(texts[0][1])
    l1, l2, t = lists
    with open(path, "wb") as f:
        f.write(np.array([0x494E4731, int(paired), n, stride, t, len(l1), len(l2), int(convert)], np.int32).tobytes())
        f.write(np.array([every, first], np.uint64).tobytes())
        for lst in (l1, l2):
            f.write(np.concatenate([[0], np.cumsum([len(s) for s in lst])]).astype(np.uint32).tobytes())
        for lst in (l1, l2):
            f.write(b"".join(lst))
        for text, recs in texts:
            f.write(np.array([text.size], np.uint64).tobytes())
            f.write(text.tobytes())
            f.write(recs.tobytes())
        for z in sizes:
            f.write(np.asarray(z, np.uint32).tobytes())


def read_sim_output(path, texts):
    data = open(path, "rb").read()
    n = len(texts[0][1])
    flags, at = np.frombuffer(data[:n], np.uint8), n
    out_texts = []
    for text, _ in texts:
        out_texts.append(data[at:at + text.size])
        at += text.size
    pieces = int(np.frombuffer(data[at:at + 4], np.uint32)[0])
    at += 4
    cuts = np.frombuffer(data[at:at + 24 * pieces], np.dtype(abi.CUT_DTYPE))
    assert at + 24 * pieces == len(data)
    return flags, out_texts, [Cut(int(c["bytes"][0]), int(c["bytes"][1]), int(c["items"]), int(c["passed"])) for c in cuts]


def converted_text(text, recs):
    """A mate's text with every record's quality line converted."""
    out = bytearray(text.tobytes())
    for r in recs:
        a, n = int(r["qual_off"]), int(r["len"])
        out[a:a + n] = phred64(out[a:a + n])
    return bytes(out)


# ---- the phred64 pack -----------------------------------------------------------------------------------
def phred64_pack(paired, raw=False):
    """umi_util's synthetic pack with its qualities redrawn over 33..126, a few bytes >= 128 and the
    63 / 64 / 65 boundary; returns (the pack as the input holds it, its texts, the pack as the host's
    reader converts it)."""
    pk, _ = U.synth_pack_and_texts(paired, crlf=not raw, min_len=1 if raw else 0)
    rng = np.random.RandomState(64)
    src, conv = Pack(pk.n, pk.stride, paired), Pack(pk.n, pk.stride, paired)
    for m in ((1, 2) if paired else (1,)):
        lens = getattr(pk, "len%d" % m)
        getattr(src, "len%d" % m)[:] = lens
        getattr(conv, "len%d" % m)[:] = lens
        for i in range(pk.n):
            L = int(lens[i])
            q = rng.randint(33, 127, L).astype(np.uint8)
            for j in np.flatnonzero(rng.rand(L) < 0.05):
                q[j] = rng.choice([63, 64, 65, 128, 200, 255])
            for dst, qq in ((src, q), (conv, np.frombuffer(phred64(q.tobytes()), np.uint8))):
                getattr(dst, "seq%d" % m)[i, :L] = getattr(pk, "seq%d" % m)[i, :L]
                getattr(dst, "qual%d" % m)[i, :L] = qq
    return src, U.synth_texts(src, crlf=not raw), conv
