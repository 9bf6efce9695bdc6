"""The removed-mode Stats pass's labels for read 2 (fqtool_amd/csrc/pe_fast.hip), restated in NumPy.

Read 2's code column holds the reverse complement of the whole row: forward chunk F is column word
kChunks - 1 - F, field u of it forward position 16 F + 15 - u, the stored code the complement
(code ^ 2, code order A C T G), an N stored as code 3 with its flag in the N word.  The pass takes the
word through one bit reversal, which restores the position order and leaves each two-bit field
bit-swapped, counts the base under that value (+ 4 inside the kept window, + 5 for an N), and the
flush reads read 2's rows through `rem_slot`.  This test walks that chain for every base at every
position of a chunk, kept and removed, and asks that the base ends in the Stats class of the reference
(its byte & 7, src/stats.cpp:249) and that read 1, whose words are walked as stored, is untouched.

The two tables themselves are taken from the source: the lines that define them are compiled into a
small host program with g++ and its output is what the model uses.
"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "fqtool_amd", "csrc", "pe_fast.hip")

CODE = {"A": 0, "C": 1, "T": 2, "G": 3}  # the columns' code order
K_RN_SLOT = 8                              # removed N; kept N = K_RN_SLOT + 4
DUMMY = 10


def _definition(text, name):
    m = re.search(r"^[^\n/]*\b%s\(int[^\n]*\{[^\n]*\}[ \t]*$" % name, text, re.M)
    assert m, "no one-line definition of %s in pe_fast.hip" % name
    return m.group(0)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """rem_slot(mate, s) for s < 4 and slot_class(s) for s < 5, printed by a host build of the
    source's own definitions."""
    text = open(SRC).read()
    d = tmp_path_factory.mktemp("relabel")
    prog = d / "tables.cpp"
    prog.write_text(
        "#include <cstdio>\n#define __host__\n#define __device__\n#define __forceinline__ inline\n"
        + _definition(text, "slot_class") + "\n" + _definition(text, "rem_slot") + "\n"
        "int main() {\n"
        "    for (int m = 0; m < 2; ++m) { for (int s = 0; s < 4; ++s) std::printf(\"%d \", rem_slot(m, s)); std::printf(\"\\n\"); }\n"
        "    for (int s = 0; s < 5; ++s) std::printf(\"%d \", slot_class(s));\n"
        "    std::printf(\"\\n\");\n    return 0;\n}\n")
    exe = d / "tables"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), str(prog)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    rem = [[int(x) for x in out[m].split()] for m in range(2)]
    cls = [int(x) for x in out[2].split()]
    assert len(rem[0]) == len(rem[1]) == 4 and len(cls) == 5
    return rem, cls


def bfrev(x):
    x = np.uint32(x)
    x = ((x >> np.uint32(1)) & np.uint32(0x55555555)) | ((x & np.uint32(0x55555555)) << np.uint32(1))
    x = ((x >> np.uint32(2)) & np.uint32(0x33333333)) | ((x & np.uint32(0x33333333)) << np.uint32(2))
    x = ((x >> np.uint32(4)) & np.uint32(0x0F0F0F0F)) | ((x & np.uint32(0x0F0F0F0F)) << np.uint32(4))
    x = ((x >> np.uint32(8)) & np.uint32(0x00FF00FF)) | ((x & np.uint32(0x00FF00FF)) << np.uint32(8))
    return np.uint32((x >> np.uint32(16)) | (x << np.uint32(16)))


def column_words(bases, mate):
    """Code and N word of one 16-base forward chunk as staging leaves them for the Stats pass: read
    1 as read, read 2 reversed and complemented; a lowercase letter has its uppercase letter's code
    and its flag (the odd bit of the N word) is cleared again before the pass."""
    cw = nw = 0
    for p, b in enumerate(bases):
        u = 15 - p if mate else p
        if b == "N":
            code, n = 3, 1
        else:
            code, n = CODE[b.upper()] ^ (2 if mate else 0), 0
        cw |= code << (2 * u)
        nw |= n << (2 * u)
    return np.uint32(cw), np.uint32(nw)


def spread(x):
    """The 16 two-bit fields of x widened to nibbles: (low word, high word)."""
    out = [0, 0]
    for u in range(16):
        out[u >> 3] |= ((int(x) >> (2 * u)) & 3) << (4 * (u & 7))
    return out


def pass_slots(cw, nw, mate, kept_len, length=16):
    """The slot nibble of each of the chunk's 16 positions, as the pass builds them."""
    if mate:  # one v_bfrev each: position order restored, fields bit-swapped, N flags at the odd bits
        cw, nw = bfrev(cw), bfrev(nw)
    nf = (int(nw) | (int(nw) >> 1)) & 0x55555555  # fold2: the flags wherever the reversal left them
    assert nf == ((int(nw) >> 1) & 0x55555555 if mate else int(nw))
    lo, hi = spread(cw)
    n_lo, n_hi = spread(nf)
    kept = [(1 << (4 * min(max(kept_len - 8 * h, 0), 8))) - 1 for h in range(2)]
    words = []
    for h, (w, n) in enumerate(((lo, n_lo), (hi, n_hi))):
        w |= kept[h] & 0x44444444
        w += n | (n << 2)  # + 5 per N; no nibble carries (7 + 5 < 16)
        words.append(w)
    slots = [(words[p >> 3] >> (4 * (p & 7))) & 0xF for p in range(16)]
    return [s if p < length else DUMMY for p, s in enumerate(slots)]


def flush_class(slot, mate, rem, cls):
    """(Stats class, kept) that the flush gives the cell `slot` of a mate's rows."""
    for s in range(5):
        rs = rem[mate][s] if s < 4 else K_RN_SLOT
        if slot in (rs, rs + 4):
            return cls[s], slot == rs + 4
    raise AssertionError("slot %d of mate %d is read by no class" % (slot, mate))


def test_tables(tables):
    rem, cls = tables
    assert rem[0] == [0, 1, 2, 3]
    # read 2: bitswap(c ^ 2)
    assert rem[1] == [((c ^ 2) >> 1) | (((c ^ 2) & 1) << 1) for c in range(4)] == [1, 3, 0, 2]
    assert sorted(rem[1]) == [0, 1, 2, 3]
    assert cls == [ord(b) & 7 for b in "ACTGN"]


@pytest.mark.parametrize("mate", [0, 1])
@pytest.mark.parametrize("kept_len", [0, 1, 7, 8, 9, 15, 16])
def test_every_base_every_position(tables, mate, kept_len):
    rem, cls = tables
    alphabet = "ACGTNacgt"
    for shift in range(len(alphabet)):
        for pos in range(16):
            # the base under test at `pos`, every other position cycling through the alphabet
            bases = [alphabet[(p + shift) % len(alphabet)] for p in range(16)]
            for b in alphabet:
                bases[pos] = b
                cw, nw = column_words(bases, mate)
                slots = pass_slots(cw, nw, mate, kept_len)
                for p, (bb, s) in enumerate(zip(bases, slots)):
                    c, k = flush_class(s, mate, rem, cls)
                    assert c == ord(bb) & 7, (mate, kept_len, p, bb, s)
                    assert k == (p < kept_len), (mate, kept_len, p, bb, s)
                    if mate == 0 and bb != "N":  # read 1: labelled by the code, as before
                        assert s == CODE[bb.upper()] + (4 if p < kept_len else 0)


def test_several_n_in_one_chunk_and_read_end(tables):
    rem, cls = tables
    for mate in (0, 1):
        for length in (1, 5, 15, 16):
            bases = ["N" if p in (0, 1, 2, length - 1) else "ACGT"[p & 3] for p in range(16)]
            cw, nw = column_words(bases[:length] + ["A"] * (16 - length), mate)
            # (staging keeps N flags only inside the read; codes past it are masked to the dummy slot)
            slots = pass_slots(cw, nw, mate, kept_len=3, length=length)
            for p in range(16):
                if p >= length:
                    assert slots[p] == DUMMY
                    continue
                c, k = flush_class(slots[p], mate, rem, cls)
                assert (c, k) == (ord(bases[p]) & 7, p < 3), (mate, length, p)
                if bases[p] == "N":
                    assert slots[p] == K_RN_SLOT + (4 if p < 3 else 0)
