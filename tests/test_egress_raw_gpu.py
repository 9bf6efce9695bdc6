"""The routed egress through the raw stream (fq_engine_raw_begin with an egress set,
fq_engine_raw_launch_routed): windows cut at random bytes, so records straddle them (the device
carry), every pack's six streams in buffers of exactly fq_egress_bound over its fq_raw_result, the
concatenated streams byte-identical to the Python model (tests/egress_util.py) over the oracle's
records, the accumulator bit-exact, and the trimmed-adapter entries per mate as in
tests/test_raw_gpu.py -- with -c the corrected reads' bytes."""
import ctypes
import random
from collections import Counter

import numpy as np
import pytest

import egress_util as G
from batch_util import Pack, config, run_oracle, synth_pack
from fqtool_amd import abi
from kmer_util import correct_pair
from test_raw_gpu import adapter_strings, decode_entries, plain_fastq

pytestmark = pytest.mark.gpu

PAIR = G.mask(G.OUT1, G.OUT2)


@pytest.fixture(scope="module")
def lib():
    return abi.load_engine()


def corrected_pack(pk, res):
    """The pack's rows as -c leaves them (fq_correct_pair_text on the FQ_RF_CORRECTED pairs)."""
    out = Pack(pk.n, pk.stride, True)
    for k in ("seq1", "qual1", "len1", "seq2", "qual2", "len2"):
        getattr(out, k)[:] = getattr(pk, k)
    for i in range(pk.n):
        a, b = res[2 * i], res[2 * i + 1]
        if not (int(a["flags"]) | int(b["flags"])) & abi.FQ_RF_CORRECTED:
            continue
        l1, l2, s1, s2 = int(pk.len1[i]), int(pk.len2[i]), int(a["start"]), int(b["start"])
        x1, y1 = bytearray(pk.seq1[i, s1:l1].tobytes()), bytearray(pk.qual1[i, s1:l1].tobytes())
        x2, y2 = bytearray(pk.seq2[i, s2:l2].tobytes()), bytearray(pk.qual2[i, s2:l2].tobytes())
        correct_pair(x1, y1, x2, y2, int(np.int16(b["m_len1"])), int(b["m_len2"]), int(b["reserved"]))
        out.seq1[i, s1:l1], out.qual1[i, s1:l1] = np.frombuffer(bytes(x1), np.uint8), np.frombuffer(bytes(y1), np.uint8)
        out.seq2[i, s2:l2], out.qual2[i, s2:l2] = np.frombuffer(bytes(x2), np.uint8), np.frombuffer(bytes(y2), np.uint8)
    return out


def descriptor(lib, p, r, open_mask, shrink=None):
    """Buffers of exactly the bounds over the pack's result (one byte less for stream `shrink`)."""
    mates = 2 if p.paired else 1
    out = abi.FqRawEgressOut()
    keep = []
    for s in range(G.STREAMS):
        if not (open_mask >> s) & 1:
            continue
        cap = lib.fq_egress_bound(s, r.text_bytes[0], r.text_bytes[1] if mates == 2 else 0, max(r.pairs, 0))
        cap -= 1 if s == shrink else 0
        buf = np.zeros(max(cap, 1), np.uint8)
        keep.append(buf)
        out.eg.text[s], out.eg.cap[s] = buf.ctypes.data, cap
    for m in range(mates):
        cap = r.text_bytes[m] + 3 * max(r.pairs, 0) + 16
        buf = np.zeros(cap, np.uint8)
        keep.append(buf)
        out.adapters[m], out.adapter_cap[m] = buf.ctypes.data, cap
    return out, keep


def run_raw_routed(lib, p, texts, open_mask, max_batch, stride, rng, wcap, ccap=600000):
    """tests/test_raw_gpu.py's driver with the routed launch: (pairs per pack, the six streams,
    adapter entry counts per mate, accumulator, largest carry)."""
    mates = len(texts)
    h = ctypes.c_void_p()
    assert lib.fq_engine_create(ctypes.byref(p), 0, max_batch, stride, ctypes.byref(h)) == 0, \
        lib.fq_engine_last_error(None).decode()
    try:
        if p.correction_enabled or (p.merge_enabled and p.discard_unmerged):  # the old refusal, until an egress is set
            assert lib.fq_engine_raw_begin(h, wcap, ccap) == abi.FQ_E_INVALID
        eg = abi.FqEgress(open_mask, 0)
        assert lib.fq_engine_set_egress(h, ctypes.byref(eg)) == 0, lib.fq_engine_last_error(h).decode()
        assert lib.fq_engine_raw_begin(h, wcap, ccap) == 0, lib.fq_engine_last_error(h).decode()
        assert lib.fq_engine_set_egress(h, None) == abi.FQ_E_INVALID  # not inside a raw stream
        pos, queued = [0, 0], [0]

        def enqueue(empty=False):
            w = abi.FqRawWindow()
            for m in range(mates):
                n = 0 if empty else min(wcap - rng.randint(0, 3000), texts[m].size - pos[m])
                w.bytes[m] = texts[m].ctypes.data + pos[m] if n else None
                w.n[m] = n
                pos[m] += n
            assert lib.fq_engine_raw_enqueue(h, ctypes.byref(w)) == 0, lib.fq_engine_last_error(h).decode()
            queued[0] += 1

        def more():
            return any(pos[m] < texts[m].size for m in range(mates))

        packs, outs, ads = [], [bytearray() for _ in range(G.STREAMS)], [Counter(), Counter()]
        adapters = [bytes(p.adapter1), bytes(p.adapter2)]
        pending, carry_max, k = [], 0, 0

        def collect():
            seq = ctypes.c_uint64()
            assert lib.fq_engine_poll(h, 1, ctypes.byref(seq)) == 1, lib.fq_engine_last_error(h).decode()
            kk, oo, _ = pending.pop(0)
            assert seq.value == kk
            for s in range(G.STREAMS):
                assert oo.eg.bytes[s] <= oo.eg.cap[s]
                if oo.eg.bytes[s]:
                    outs[s] += ctypes.string_at(oo.eg.text[s], oo.eg.bytes[s])
            for m in range(mates):
                ads[m] += decode_entries(ctypes.string_at(oo.adapters[m], oo.adapter_bytes[m]), adapters[m])

        enqueue()
        while True:
            if more() and queued[0] - k < 2:
                enqueue()
            r = abi.FqRawResult()
            assert lib.fq_engine_raw_wait(h, ctypes.byref(r)) == 0
            if k == 0 and r.pairs > 0:  # refusals come before the launch and leave the window enqueued
                small, keep_s = descriptor(lib, p, r, open_mask, shrink=G.OUT1)
                assert lib.fq_engine_raw_launch_routed(h, ctypes.byref(r), ctypes.byref(small), k) == abi.FQ_E_INVALID
                if p.correction_enabled or (p.merge_enabled and p.discard_unmerged):
                    old = abi.FqRawOut()
                    big = [np.zeros(ccap + wcap + 28 * max_batch + 64, np.uint8) for _ in range(2)]
                    for m in range(mates):
                        old.text.text[m] = big[m].ctypes.data
                    assert lib.fq_engine_raw_launch(h, ctypes.byref(r), ctypes.byref(old), k) == abi.FQ_E_INVALID
                assert lib.fq_engine_pending(h) == 0
            o, keep = descriptor(lib, p, r, open_mask)
            assert lib.fq_engine_raw_launch_routed(h, ctypes.byref(r), ctypes.byref(o), k) == 0, \
                lib.fq_engine_last_error(h).decode()
            pending.append((k, o, keep))
            packs.append(r.pairs)
            carry_max = max(carry_max, max(r.carry[m] for m in range(mates)))
            while len(pending) > 2:
                collect()
            left = any(r.carry[m] for m in range(mates))
            k += 1
            last = not more() and queued[0] == k
            assert not r.stop
            if last and not (left and r.pairs > 0):
                break
            if last:
                enqueue(empty=True)
        while pending:
            collect()
        assert lib.fq_engine_sync(h) == 0
        acc = np.zeros(lib.fq_engine_acc_words(h), np.uint64)
        assert lib.fq_engine_read_acc(h, acc.ctypes.data, acc.size) == 0
        assert lib.fq_engine_raw_end(h) == 0
        return packs, [bytes(x) for x in outs], ads[:mates], acc, carry_max
    finally:
        lib.fq_engine_destroy(h)


# -c with every stream the config feeds; -m --discard_unmerged with the pair and merged streams
@pytest.mark.parametrize("cfg,discard,open_mask", [
    ("PE_correct", 0, PAIR | G.mask(G.UNPAIRED1, G.UNPAIRED2, G.FAILED)),
    ("C4", 1, PAIR | G.mask(G.MERGED)),
])
def test_routed_raw_stream_matches_model(lib, oracle, cfg, discard, open_mask):
    p = config(cfg, max_cycles=512)
    p.discard_unmerged = discard
    pk = synth_pack(oracle, 3000, True, first=17)
    rng = random.Random(11)
    texts = [plain_fastq(pk, m, rng) for m in (1, 2)]
    res_o, acc_o = run_oracle(oracle, p, pk)
    packs, got, ads, acc, carry_max = run_raw_routed(lib, p, [t[0] for t in texts], open_mask, 4096, pk.stride, rng,
                                                      wcap=max(t[0].size for t in texts) // 2 + 2000)
    assert sum(packs) == pk.n and sum(1 for n in packs if n) >= 2 and carry_max > 0  # two windows with a carry
    assert np.array_equal(acc, acc_o)
    reads = [G.reads_of_pack(pk, m + 1, texts[m][2], texts[m][3]) for m in range(2)]
    exp = G.model(reads, res_o, True, bool(p.merge_enabled), bool(discard), open_mask)
    for s in range(G.STREAMS):
        assert got[s] == exp[s], "stream %s differs" % G.STREAM_NAMES[s]
        assert bool(exp[s]) == bool((open_mask >> s) & 1), G.STREAM_NAMES[s]
    corrected = bool((res_o["flags"] & abi.FQ_RF_CORRECTED).any())
    assert corrected == bool(p.correction_enabled)
    want = adapter_strings(res_o, corrected_pack(pk, res_o) if corrected else pk, p, True)
    assert sum(want[0].values()) > 0 and sum(want[1].values()) > 0
    assert ads == want
    if corrected:  # (some entry does hold corrected bytes: the uncorrected rows give other strings)
        assert want != adapter_strings(res_o, pk, p, True)


@pytest.mark.parametrize("case", ["td_pe_correct", "td_pe_all", "td_pe_merge_discard"])
def test_fqtool_takes_the_raw_stream(case, tmp_path):
    """Plain input files on one engine: the closing log line names the raw stream with the routed
    egress, over many small windows (4 KiB first window, 500-pair packs), and the outputs and
    reports are the reference's."""
    import gzip
    import os
    import shutil
    import subprocess

    import e2e_util as E
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    outd.mkdir()
    argv = E.argv_for(abi.FQTOOL_BIN, case, str(outd))
    for k, a in enumerate(argv):
        if a.startswith(E.INPUTS) and a.endswith(".fq.gz"):
            plain = ind / os.path.basename(a)[:-3]
            with gzip.open(a, "rb") as f, open(plain, "wb") as g:
                shutil.copyfileobj(f, g)
            argv[k] = str(plain)
    argv += ["--pack_pairs", "500"]
    p = subprocess.run(argv, capture_output=True, cwd=outd, timeout=300, env=dict(os.environ, FQ_RAW_WINDOW0="4096"))
    err = p.stderr.decode()
    assert p.returncode == 0, err[-2000:]
    closing = [l for l in err.splitlines() if "fqtool-amd: " in l and " reads on " in l]
    assert len(closing) == 1 and "(raw stream" in closing[0] and "routed egress of" in closing[0], err[-2000:]
    E.check_outputs(case, str(outd))
