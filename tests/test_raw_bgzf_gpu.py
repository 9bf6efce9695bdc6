"""BGZF windows of the raw stream (fq_engine_raw_enqueue_bgzf: the window's members inflated on the
device into the window's place) against the oracle.

Each mate's FASTQ text is cut into BGZF members; the windows are byte ranges of the inflated stream
that start and end anywhere, so most start inside a member (skip > 0: the member's leading bytes
land in the carry region and the carried bytes overwrite them) and every member a window cuts is
inflated again by the next one.  Over the whole stream the packs must equal what the plain raw
stream gives (test_raw_gpu.py): pack sizes, output text, adapter entries and every accumulator word
equal to the oracle's.  A member that does not inflate ends the stream with stop = 2 before anything
of its window is taken."""
import ctypes
import random
import struct
import zlib
from collections import Counter

import numpy as np
import pytest

from batch_util import config, edge_pack, run_oracle, synth_pack
from fqtool_amd import abi
from test_raw_gpu import adapter_strings, decode_entries, plain_fastq
from test_text_gpu import expected_out

pytestmark = pytest.mark.gpu

WCAP, CCAP = 200000, 600000
HEADER = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0])


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


class Chain:
    """One mate's text as a BGZF file image (members of `msize` bytes, then the empty EOF member)
    and its member table: payload offset and length, isize, crc and the member's stream offset."""

    def __init__(self, text, msize, level):
        self.text = text
        raw = text.tobytes()
        img, self.members = bytearray(), []
        for o in list(range(0, len(raw), msize)) + [len(raw)]:
            blk = raw[o:o + msize] if o < len(raw) else b""
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            d = c.compress(blk) + c.flush()
            assert len(d) <= abi.FQ_INFLATE_MAX
            img += HEADER + struct.pack("<H", len(d) + 25)
            self.members.append([len(img), len(d), len(blk), zlib.crc32(blk), o])
            img += d + struct.pack("<II", zlib.crc32(blk), len(blk))
        self.img = np.frombuffer(bytes(img), np.uint8).copy()

    def window(self, pos, n):
        """(first member, one past the last) of the members overlapping [pos, pos + n); the last
        window of the stream takes the EOF member too."""
        ms = self.members
        if not n:
            return (len(ms) - 1, len(ms)) if pos == self.text.size else (0, 0)
        a = max(i for i in range(len(ms) - 1) if ms[i][4] <= pos)
        b = a
        while b < len(ms) and ms[b][4] < pos + n:
            b += 1
        if pos + n == self.text.size:
            b = len(ms)
        return a, b


def fill_bgzf(w, keep, m, chain, pos, n, tamper=None):
    """Mate m's part of a fq_raw_bgzf_window for stream bytes [pos, pos + n).  tamper = (member, kind)
    spoils that member of the chain.  Returns the window's byte count (a spoilt size may shorten it)."""
    a, b = chain.window(pos, n)
    if a == b:
        w.comp[m], w.comp_bytes[m], w.members[m], w.skip[m], w.n[m] = None, 0, 0, 0, 0
        return 0
    ms = chain.members
    lo, hi = ms[a][0], ms[b - 1][0] + ms[b - 1][1]
    comp = chain.img[lo:hi].copy()
    tab = (abi.FqInflateMember * (b - a))()
    for i in range(a, b):
        off, ln, isize, crc, _ = ms[i]
        if tamper and tamper[0] == i:
            kind = tamper[1]
            if kind == "data":
                comp[off - lo] = 0x07  # a final block of the reserved type 3
            elif kind == "long":
                isize -= 1
            elif kind == "short":
                isize += 1
            elif kind == "crc":
                crc ^= 1
        t = tab[i - a]
        t.in_off, t.in_len, t.isize, t.crc = off - lo, ln, isize, crc
        t.status, t.produced = 77, 77  # (ignored)
    skip = pos - ms[a][4]
    total = sum(tab[i].isize for i in range(b - a))
    n = min(n, total - skip)
    assert total - skip <= WCAP and skip <= CCAP and comp.size <= WCAP
    keep += [comp, tab]
    w.comp[m], w.comp_bytes[m] = comp.ctypes.data, comp.size
    w.m[m] = ctypes.cast(tab, ctypes.POINTER(abi.FqInflateMember))
    w.members[m], w.skip[m], w.n[m] = b - a, skip, n
    return n


def run_raw_bgzf(lib, p, chains, max_batch, stride, rng, mix=False, tamper=None, tamper_window=2):
    """test_raw_gpu.run_raw with BGZF windows (mix: every other window goes through
    fq_engine_raw_enqueue).  tamper = (mate, kind): the first member of that mate's window
    `tamper_window` is spoilt.  Returns run_raw's tuple and, per window, (carry before it, result)."""
    mates = len(chains)
    texts = [c.text for c in chains]
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, max_batch, stride, ctypes.byref(h)) == 0, \
        lib.fq_engine_last_error(None).decode()
    keep = []
    try:
        assert lib.fq_engine_raw_begin(h, WCAP, CCAP) == 0, lib.fq_engine_last_error(h).decode()
        pos = [0, 0]
        starts = []
        frac = [0.0]
        span = 60000  # windows of at most this many bytes: a member of 65280 bytes is cut by every one

        def enqueue(empty=False):
            win = []
            frac[0] = min(1.0, frac[0] + rng.uniform(0.2, 1.0) * span * 0.8 / max(t.size for t in texts))
            plain = mix and len(starts) % 2 == 1
            w = abi.FqRawWindow() if plain else abi.FqRawBgzfWindow()
            for m in range(mates):
                want = int(frac[0] * texts[m].size) - pos[m] + rng.randint(-3000, 3000)
                n = 0 if empty else max(0, min(want, span, texts[m].size - pos[m]))
                if frac[0] >= 1.0 and not empty:
                    n = min(span, texts[m].size - pos[m])
                if plain:
                    w.bytes[m] = texts[m].ctypes.data + pos[m] if n else None
                    w.n[m] = n
                else:
                    spoil = tamper and tamper[0] == m and len(starts) == tamper_window
                    first = chains[m].window(pos[m], n)[0]
                    n = fill_bgzf(w, keep, m, chains[m], pos[m], n, (first, tamper[1]) if spoil else None)
                win.append((pos[m], n))
                pos[m] += n
            call = lib.fq_engine_raw_enqueue if plain else lib.fq_engine_raw_enqueue_bgzf
            assert call(h, ctypes.byref(w)) == 0, lib.fq_engine_last_error(h).decode()
            starts.append(win)

        def more():
            return any(pos[m] < texts[m].size for m in range(mates))

        packs, outs, ads, stop, log = [], [bytearray(), bytearray()], [Counter(), Counter()], None, []
        adapters = [bytes(p.adapter1), bytes(p.adapter2)]
        pending = []
        carry = [0, 0]

        def take(kk, oo, bb):
            seq = ctypes.c_uint64()
            assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
            assert seq.value == kk
            for m in range(mates):
                nb = oo.text.bytes[m]
                outs[m] += bb[m][:nb].tobytes()
                ads[m] += decode_entries(bb[m][nb:nb + oo.adapter_bytes[m]].tobytes(), adapters[m])

        enqueue()
        k = 0
        while True:
            if more() and len(starts) - k < 2:
                enqueue()
            r = abi.FqRawResult()
            rw = abi.FqRawResult()
            o = abi.FqRawOut()
            bufs = []
            for m in range(mates):
                tb = np.zeros(CCAP + WCAP + 4 * max_batch + 64, np.uint8)
                bufs.append(tb)
                o.text.text[m] = tb.ctypes.data
            assert lib.fq_engine_raw_wait(h, ctypes.byref(rw)) == 0
            assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(o), k) == 0, lib.fq_engine_last_error(h).decode()
            assert (rw.pairs, rw.stop, list(rw.carry)) == (r.pairs, r.stop, list(r.carry))
            pending.append((k, o, bufs))
            keep.append(bufs)
            packs.append(r.pairs)
            log.append((list(carry), r))
            carry = [r.carry[0], r.carry[1]]
            while len(pending) > 2:
                take(*pending.pop(0))
            left = any(r.carry[m] for m in range(mates))
            win = starts[k]
            k += 1
            last = not more() and len(starts) == k
            exhausted = any(pos[m] == texts[m].size for m in range(mates))
            if r.stop or (r.pairs == 0 and exhausted) or (last and not (left and r.pairs > 0)):
                stop = (r.stop, [win[m][0] + win[m][1] - r.carry[m] for m in range(mates)], r.pairs, win)
                break
            if last:
                enqueue(empty=True)
        for item in pending:
            take(*item)
        assert lib.fq_engine_raw_end(h) == 0
        assert lib.fq_engine_sync(h) == 0
        acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
        assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
        return packs, [bytes(x) for x in outs[:mates]], ads[:mates], acc, stop, log
    finally:
        lib.fq_engine_destroy(h)


def make_chains(texts, msize, levels):
    return [Chain(t[0], msize, levels[m % len(levels)]) for m, t in enumerate(texts)]


@pytest.mark.parametrize("cfg", ["C3", "PE_all", "SE_all"])
@pytest.mark.parametrize("source", ["synth", "edge"])
@pytest.mark.parametrize("max_batch", [4096, 97])
@pytest.mark.parametrize("msize", [65280, 30000, 777])
def test_bgzf_windows_match_oracle(lib, oracle, cfg, source, max_batch, msize):
    paired = cfg != "SE_all"
    p = config(cfg, max_cycles=512)
    pk = synth_pack(oracle, 3000, paired, first=17) if source == "synth" else edge_pack(2000, paired)
    if source == "edge":  # an empty sequence line is not plain: give those reads one base
        for i in range(pk.n):
            for m in ((1, 2) if paired else (1,)):
                if int(getattr(pk, "len%d" % m)[i]) == 0:
                    pk.set(i, m, b"N", b"#")
    rng = random.Random(zlib.crc32(("%s/%s/%d/%d" % (cfg, source, max_batch, msize)).encode()))
    texts = [plain_fastq(pk, m, rng) for m in ((1, 2) if paired else (1,))]
    stride = 320 if source == "edge" else 160
    assert int(pk.len1.max()) <= stride and (not paired or int(pk.len2.max()) <= stride)
    # mate 1 at level 1 and mate 2 at level 6; single end: one level per batch size
    chains = make_chains(texts, msize, (1, 6) if paired else ((1,) if max_batch == 4096 else (6,)))
    res_o, acc_o = run_oracle(oracle, p, pk)
    packs, outs, ads, acc, stop, log = run_raw_bgzf(lib, p, chains, max_batch, stride, rng)
    assert sum(packs) == pk.n and max(packs) <= max_batch, packs
    assert stop[0] == 0
    assert np.array_equal(acc, acc_o)
    exp = expected_out(pk, res_o, paired, [(None, None, t[2], t[3]) for t in texts])
    for m in range(len(outs)):
        assert outs[m] == exp[m], f"mate {m + 1}: output text differs"
    want = adapter_strings(res_o, pk, p, paired)
    for m in range(len(ads)):
        assert ads[m] == want[m], f"mate {m + 1}: adapter strings differ"


@pytest.fixture(scope="module")
def c3_stream(oracle):
    """A C3 pair stream shared by the tests below: pack, texts, chains of 30000-byte members."""
    pk = synth_pack(oracle, 3000, True, first=5)
    rng = random.Random(99)
    texts = [plain_fastq(pk, m, rng) for m in (1, 2)]
    return pk, texts, make_chains(texts, 30000, (1, 6))


def check_prefix(oracle, p, texts, n_pairs, outs, acc):
    sub = synth_pack(oracle, n_pairs, True, first=5)
    res_o, acc_o = run_oracle(oracle, p, sub)
    assert np.array_equal(acc, acc_o)
    assert outs == expected_out(sub, res_o, True, [(None, None, t[2][:n_pairs], t[3][:n_pairs]) for t in texts])


def test_bgzf_and_plain_windows_mixed(lib, oracle, c3_stream):
    pk, texts, chains = c3_stream
    p = config("C3", max_cycles=512)
    packs, outs, _, acc, stop, _ = run_raw_bgzf(lib, p, chains, 4096, 160, random.Random(3), mix=True)
    assert sum(packs) == pk.n and stop[0] == 0 and len(packs) > 4
    check_prefix(oracle, p, texts, pk.n, outs, acc)


@pytest.mark.parametrize("mate", [1, 2])
@pytest.mark.parametrize("kind", ["data", "long", "short", "crc"])
def test_bad_member_stops_the_stream(lib, oracle, c3_stream, mate, kind):
    """The first member of the third window of one mate does not inflate: stop = 2, no pairs, every
    byte of the carry and the window still to be read; the packs before it are the oracle's."""
    pk, texts, chains = c3_stream
    p = config("C3", max_cycles=512)
    packs, outs, _, acc, stop, log = run_raw_bgzf(lib, p, chains, 4096, 160, random.Random(11 * mate), tamper=(mate - 1, kind))
    assert len(packs) == 3 and packs[2] == 0 and packs[0] > 0 and packs[1] > 0, packs
    before, r = log[2]
    assert r.stop == abi.FQ_RAW_STOP_INFLATE and r.pairs == 0
    win = stop[3]
    assert [r.carry[m] for m in range(2)] == [before[m] + win[m][1] for m in range(2)]
    check_prefix(oracle, p, texts, sum(packs), outs, acc)


@pytest.mark.parametrize("mate", [1, 2])
def test_bgzf_stream_stops_at_irregular_record(lib, oracle, mate):
    p = config("C3", max_cycles=512)
    pk = synth_pack(oracle, 3000, True, first=5)
    rng = random.Random(31 + mate)
    bad = 1234
    texts = [plain_fastq(pk, m, rng, irregular_at=bad if m == mate else None) for m in (1, 2)]
    packs, outs, _, acc, stop, _ = run_raw_bgzf(lib, p, make_chains(texts, 30000, (1, 6)), 4096, 160, rng)
    assert stop[0] == 1 or stop[2] == 0
    assert stop[0] != abi.FQ_RAW_STOP_INFLATE
    assert sum(packs) == bad
    assert stop[1] == [texts[0][1][bad], texts[1][1][bad]]
    check_prefix(oracle, p, texts, bad, outs, acc)


def test_refusals_leave_the_engine_usable(lib, oracle, c3_stream):
    pk, texts, chains = c3_stream
    p = config("C3", max_cycles=512)
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, 4096, 160, ctypes.byref(h)) == 0
    keep = []

    def good(n=50000):
        w = abi.FqRawBgzfWindow()
        for m in range(2):
            assert fill_bgzf(w, keep, m, chains[m], 0, n) == n
        return w

    def refused(w):
        assert lib.fq_engine_raw_enqueue_bgzf(h, ctypes.byref(w)) == -1
        assert lib.fq_engine_last_error(h)

    try:
        refused(good())  # before fq_engine_raw_begin
        assert lib.fq_engine_raw_begin(h, WCAP, 4096) == 0
        refused(good())  # a carry capacity below 65536
        assert lib.fq_engine_raw_end(h) == 0
        assert lib.fq_engine_raw_begin(h, WCAP, CCAP) == 0
        for m in range(2):
            w = good()
            w.members[m] = abi.FQ_RAW_BGZF_MEMBERS + 1
            refused(w)
            for field, value in (("in_len", abi.FQ_INFLATE_MAX + 1), ("isize", abi.FQ_INFLATE_MAX + 1)):
                w = good()
                setattr(w.m[m][1], field, value)
                refused(w)
            w = good()
            w.m[m][1].in_off = w.comp_bytes[m] - w.m[m][1].in_len + 1  # the payload's last byte outside
            refused(w)
            w = good()
            w.m[m][0].in_off = 1 << 40
            refused(w)
            w = good()
            w.comp_bytes[m] = WCAP + 1
            refused(w)
            w = good()
            w.skip[m] = CCAP + 1
            refused(w)
            w = good()  # members of 60000 bytes in all: skip + n beyond them
            w.n[m] = 60001
            refused(w)
            w = good()
            w.skip[m], w.n[m] = 30000, 30001
            refused(w)
            w = good()  # members of 210000 bytes after a skip of 9999: one more than the window capacity
            a = (abi.FqInflateMember * 7)()
            for i in range(7):
                a[i].in_off, a[i].in_len, a[i].isize = 0, 2, 30000
            keep.append(a)
            w.m[m] = ctypes.cast(a, ctypes.POINTER(abi.FqInflateMember))
            w.members[m], w.skip[m], w.n[m] = 7, 9999, 1000
            refused(w)
        # a good window still runs, and so do three; the fourth waiting one is refused
        for _ in range(3):
            w = good()
            assert lib.fq_engine_raw_enqueue_bgzf(h, ctypes.byref(w)) == 0, lib.fq_engine_last_error(h).decode()
        refused(good())
        r = abi.FqRawResult()
        assert lib.fq_engine_raw_wait(h, ctypes.byref(r)) == 0
        assert r.stop == 0
        assert r.pairs == min(sum(1 for o in texts[m][1][1:] if o <= 50000) for m in range(2))
        assert lib.fq_engine_raw_end(h) == 0
    finally:
        lib.fq_engine_destroy(h)
