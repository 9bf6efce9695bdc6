#!/usr/bin/env python3
"""Times the k-mer passes (fq_kstat_*, fqtool_amd/csrc/kstat.hip) against the pack's main kernels.

The bench's synthetic 2x150 pairs with the C3 parameters, resident in HBM, one pack through
fq_engine_process_device per run: fq_kstat_last_kernel_ms (both k-mer passes, device events) next
to fq_engine_last_kernel_ms (the main kernels, device events) for each --k, after a warm-up run;
and the main kernels alone with no tables attached (--k none), which is also all an engine library
without the fq_kstat_* calls can run (--lib: e.g. the parent commit's build, to compare that path).
Prints one JSON line.

  python3 tools/kstat_bench.py --pairs 16777216 --k 5,6,7,8,12 --runs 3
  python3 tools/kstat_bench.py --pairs 16777216 --k none --runs 5 [--lib PATH/libfqengine.so]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

READ_LEN, STRIDE, SEED = 150, 160, 20261015  # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16 << 20)
    ap.add_argument("--k", default="5,6,7,8,12", help="comma-separated k-mer lengths, or 'none'")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--lib", default=None, help="engine library to load (default: this tree's)")
    args = ap.parse_args()

    import torch
    from fqtool_amd import abi

    lib = ctypes.CDLL(args.lib or abi.ENGINE_LIB)
    vp = ctypes.c_void_p
    lib.fq_engine_create.argtypes = [ctypes.POINTER(abi.FqParams), ctypes.c_int, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.POINTER(vp)]
    lib.fq_engine_destroy.argtypes = [vp]
    lib.fq_engine_process_device.argtypes = [vp, ctypes.POINTER(abi.FqBatch), vp, vp]
    lib.fq_engine_sync.argtypes = [vp]
    lib.fq_engine_reset_acc.argtypes = [vp]
    lib.fq_engine_last_kernel_ms.argtypes = [vp]
    lib.fq_engine_last_kernel_ms.restype = ctypes.c_double
    lib.fq_synth_fill_device.argtypes = [ctypes.POINTER(abi.FqBatch), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, vp]
    ks = [] if args.k == "none" else [int(x) for x in args.k.split(",")]
    if ks:
        lib.fq_kstat_create.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.POINTER(vp)]
        lib.fq_kstat_destroy.argtypes = [vp]
        lib.fq_engine_set_kstat.argtypes = [vp, vp]
        lib.fq_kstat_last_kernel_ms.argtypes = [vp]
        lib.fq_kstat_last_kernel_ms.restype = ctypes.c_double

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

    seq_bytes = 2.0 * n * READ_LEN  # sequence bytes one pass reads (each of the two passes reads them)
    out = {"pairs": n, "read_len": READ_LEN, "config": "C3", "lib": args.lib or "tree", "runs": args.runs}
    run()  # warm-up
    out["main_ms_no_tables"] = [round(run(), 3) for _ in range(args.runs)]
    out["k"] = {}
    for k in ks:
        t = vp()
        assert lib.fq_kstat_create(0, k, ctypes.byref(t)) == 0
        assert lib.fq_engine_set_kstat(h, t) == 0
        run()  # warm-up
        main_ms, kmer_ms = [], []
        for _ in range(args.runs):
            main_ms.append(run())
            kmer_ms.append(lib.fq_kstat_last_kernel_ms(t))
        assert lib.fq_engine_set_kstat(h, None) == 0
        lib.fq_kstat_destroy(t)
        best = min(kmer_ms)
        out["k"][str(k)] = {"main_ms": [round(x, 3) for x in main_ms], "kmer_ms": [round(x, 3) for x in kmer_ms],
                            "kmer_over_main": round(best / min(main_ms), 3),
                            # both passes together read the sequence planes twice
                            "kmer_seq_GBps": round(2 * seq_bytes / (best * 1e-3) / 1e9, 1)}
    lib.fq_engine_destroy(h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
