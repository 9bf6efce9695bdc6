#!/usr/bin/env python3
"""Times the overrepresented-sequence passes (fq_ora_*, fqtool_amd/csrc/ora.hip) against the pack's
main kernels.

The bench's synthetic 2x150 pairs with the C3 parameters, resident in HBM, one pack through
fq_engine_process_device per run: fq_ora_last_kernel_ms (both passes with their scan and count
kernels, device events) next to fq_engine_last_kernel_ms (the main kernels, device events) for each
--sampling, best of --runs after a warm-up run; and the main kernels alone with no handle attached.
The hot sets are the evaluator's for a pair of input files (--in1 / --in2, through the host
library's session with FQ_ORA=1; default: the generated test inputs).  Prints one JSON line.

  python3 tools/ora_bench.py --pairs 16777216 --sampling 100,1 --runs 3
  python3 tools/ora_bench.py --in1 tests/golden/inputs/r1.fq.gz --in2 tests/golden/inputs/r2.fq.gz
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

READ_LEN, STRIDE, SEED = 150, 160, 20261015  # bench.py's
INPUTS = os.path.join(REPO, "tests", "golden", "inputs")


def hot_sets(host, in1, in2):
    """The evaluator's hot sets of two input files, as (bytes, offsets, n) per set, and the evaluated lengths."""
    import numpy as np
    os.environ["FQ_ORA"] = "1"
    with tempfile.TemporaryDirectory() as tmp:
        argv = ["fqtool", "-i", in1, "-I", in2, "-o", os.path.join(tmp, "o1.fq"), "-O", os.path.join(tmp, "o2.fq"),
                "-J", os.path.join(tmp, "r.json"), "-H", os.path.join(tmp, "r.html"), "--ora"]
        enc = [a.encode() for a in argv]
        arr = (ctypes.c_char_p * len(enc))(*enc)
        s = ctypes.c_void_p()
        assert host.fqh_session_open(len(enc), arr, ctypes.byref(s)) == 0, host.fqh_session_error(s)
        try:
            ci = ctypes.c_int
            on, smp, e1, e2 = ci(), ci(), ci(), ci()
            host.fqh_session_ora_params(s, ctypes.byref(on), ctypes.byref(smp), ctypes.byref(e1), ctypes.byref(e2))
            sets = []
            for which in range(2):
                seq, off, n = ctypes.c_void_p(), ctypes.c_void_p(), ci()
                host.fqh_session_ora_hot_set(s, which, ctypes.byref(seq), ctypes.byref(off), ctypes.byref(n))
                o = np.ctypeslib.as_array(ctypes.cast(off, ctypes.POINTER(ctypes.c_uint32)), (n.value + 1,)).copy()
                data = np.frombuffer(ctypes.string_at(seq, int(o[-1])) if n.value else b"\0", np.uint8).copy()
                sets.append((data, o, n.value))
            return sets, e1.value, e2.value
        finally:
            host.fqh_session_close(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16 << 20)
    ap.add_argument("--sampling", default="100,1")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--in1", default=os.path.join(INPUTS, "ora_r1.fq.gz"))
    ap.add_argument("--in2", default=os.path.join(INPUTS, "ora_r2.fq.gz"))
    args = ap.parse_args()

    import torch
    from fqtool_amd import abi

    lib = abi.load_engine()
    sets, e1, e2 = hot_sets(abi.load_host(), args.in1, args.in2)
    vp = ctypes.c_void_p
    p = abi.default_params(paired=True, max_cycles=256)  # C3: -q -a -g
    p.qual_filter_enabled = p.adapter_trimming = p.polyg_enabled = 1
    n = args.pairs
    dev = torch.device("cuda", 0)
    planes = [torch.empty(abi.batch_bytes(n, STRIDE), dtype=torch.uint8, device=dev) for _ in range(4)]
    lens = [torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2)]
    results = torch.empty(n * 2 * 16, dtype=torch.uint8, device=dev)
    b = abi.FqBatch()
    b.n, b.stride = n, STRIDE
    b.seq1, b.qual1, b.seq2, b.qual2 = [t.data_ptr() for t in planes]
    b.len1, b.len2 = lens[0].data_ptr(), lens[1].data_ptr()
    assert lib.fq_synth_fill_device(ctypes.byref(b), SEED, 0, READ_LEN, None) == 0
    torch.cuda.synchronize()
    h = vp()
    assert lib.fq_engine_create(ctypes.byref(p), 0, 0, 0, ctypes.byref(h)) == 0

    def run():
        assert lib.fq_engine_process_device(h, ctypes.byref(b), results.data_ptr(), None) == 0
        assert lib.fq_engine_sync(h) == 0
        ms = lib.fq_engine_last_kernel_ms(h)
        lib.fq_engine_reset_acc(h)
        return ms

    out = {"pairs": n, "read_len": READ_LEN, "config": "C3", "runs": args.runs, "in1": os.path.basename(args.in1),
           "hot_sequences": [sets[0][2], sets[1][2]], "eval_len": [e1, e2]}
    run()  # warm-up
    out["main_ms_no_handle"] = [round(run(), 3) for _ in range(args.runs)]
    out["sampling"] = {}
    for smp in [int(x) for x in args.sampling.split(",")]:
        t = vp()
        assert lib.fq_ora_create(0, smp, e1, e2, sets[0][0].ctypes.data, sets[0][1].ctypes.data, sets[0][2],
                                 sets[1][0].ctypes.data, sets[1][1].ctypes.data, sets[1][2], ctypes.byref(t)) == 0
        assert lib.fq_engine_set_ora(h, t) == 0
        run()  # warm-up
        main_ms, ora_ms = [], []
        for _ in range(args.runs):
            main_ms.append(run())
            ora_ms.append(lib.fq_ora_last_kernel_ms(t))
        assert lib.fq_engine_set_ora(h, None) == 0
        lib.fq_ora_destroy(t)
        out["sampling"][str(smp)] = {"main_ms": [round(x, 3) for x in main_ms], "ora_ms": [round(x, 3) for x in ora_ms],
                                     "ora_over_main": round(min(ora_ms) / min(main_ms), 3)}
    lib.fq_engine_destroy(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
