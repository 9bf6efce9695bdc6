"""Profiling aid: time the fast PE kernel with phases switched off (fq_params.reserved[0] bits,
see pe_fast.hip).  Outputs are NOT valid in ablated runs; only the timings matter."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fqtool_amd import abi

lib = abi.load_engine()
dev = torch.device("cuda:0")
n, stride = int(os.environ.get("PAIRS", 20_000_000)), 160
bufs = [torch.empty(abi.batch_bytes(n, stride), dtype=torch.uint8, device=dev) for _ in range(4)]
lens = [torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2)]
b = abi.FqBatch(); b.n, b.stride = n, stride
b.seq1, b.qual1, b.seq2, b.qual2 = [t.data_ptr() for t in bufs]
b.len1, b.len2 = lens[0].data_ptr(), lens[1].data_ptr()
assert lib.fq_synth_fill_device(ctypes.byref(b), 20261015, 0, 150, None) == 0
res = torch.empty(n * 32, dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
variants = [("full", 0), ("no_overlap", 1), ("no_filter", 2), ("no_stats", 4), ("no_polyg", 8),
            ("no_lds_atomics", 16), ("no_overlap_filter_stats", 7), ("stage_only", 15), ("no_polyg_counters", 32),
            ("no_ov_exact", 64), ("no_ov_scan", 128),
            ("plus_512_valu", 256), ("one_wg_per_cu", 70 << 16)]
if "--phases" in sys.argv:  # only the stamped launch below (phase shares, the waves' end times)
    variants = []
only = os.environ.get("VARIANTS")
if only:
    variants = [v for v in variants if v[0] in only.split(",")]
results = {}
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import config_params  # (the BASELINE config's engine parameters, CONFIG=C3 by default)
CFG = os.environ.get("CONFIG", "C3")
for rep in range(int(os.environ.get("REPS", 3))):
    for name, bits in variants:
        p = config_params(abi, CFG)
        p.reserved[0] = bits & 0xFFFF
        p.reserved[2] = (bits >> 16) * 1024  # extra LDS KiB per workgroup (occupancy probe)
        h = ctypes.c_void_p(); assert lib.fq_engine_create(ctypes.byref(p), 0, 0, 0, ctypes.byref(h)) == 0
        lib.fq_engine_process_device(h, ctypes.byref(b), res.data_ptr(), None); lib.fq_engine_sync(h)
        lib.fq_engine_process_device(h, ctypes.byref(b), res.data_ptr(), None); lib.fq_engine_sync(h)
        ms = lib.fq_engine_last_kernel_ms(h)
        results.setdefault(name, []).append(ms)
        lib.fq_engine_destroy(h)
for name in results:
    v = sorted(results[name])
    print(f"{name:28s} median {v[len(v)//2]:8.2f} ms  min {v[0]:8.2f}  -> {n / (v[len(v)//2] / 1e3) / 1e9:.2f} G pairs/s", flush=True)

# per-phase wave cycles (fq_params.reserved[1] = 1)
names = ["staging", "trim", "polyG", "overlap", "polyX/maxlen", "filter", "stats", "store"]
from bench import config_params
p = config_params(abi, os.environ.get("CONFIG", "C3"))
p.reserved[1] = 1
h = ctypes.c_void_p(); assert lib.fq_engine_create(ctypes.byref(p), 0, 0, 0, ctypes.byref(h)) == 0
lib.fq_debug_phase_cycles.argtypes = [ctypes.c_void_p, ctypes.c_int]
out = (ctypes.c_ulonglong * 8)()
lib.fq_engine_process_device(h, ctypes.byref(b), res.data_ptr(), None); lib.fq_engine_sync(h)
lib.fq_debug_phase_cycles(out, 8)
lib.fq_engine_process_device(h, ctypes.byref(b), res.data_ptr(), None); lib.fq_engine_sync(h)
print("stamped run ms", lib.fq_engine_last_kernel_ms(h))
lib.fq_debug_phase_cycles(out, 8)
tot = sum(out)
if tot == 0:
    print("no phase stamps (build with make STAMPS=1)")
for nm, v in (zip(names, out) if tot else []):
    print(f"phase {nm:14s} {100.0 * v / tot:6.1f}%  {v / 2048:14.0f} cycles/wave")

# The waves' clocks (device clock at 100 MHz) at their start and at the end of their tile loops, before
# the flush: how long the launch's SIMDs wait for its last waves.  Relative to the launch's first
# start stamp and last end stamp; per XCD (workgroup index % 8) as well.
import numpy as np
NW = 8192
ws = np.zeros(2 * NW, np.uint64)
lib.fq_debug_wave_ends.argtypes = [ctypes.c_void_p, ctypes.c_int]
if tot and lib.fq_debug_wave_ends(ws.ctypes.data, NW) == 0:
    start, end = ws[0::2].astype(np.int64), ws[1::2].astype(np.int64)
    on = end > 0
    nw = int(on.sum())
    start, end = start[on], end[on]
    wg_waves = int(os.environ.get("WG_WAVES", 8))  # waves per workgroup of the variant run (C3: 8)
    xcd = (np.nonzero(on)[0] // wg_waves) % 8
    t0, t1 = int(start.min()), int(end.max())
    span = t1 - t0
    us = lambda ticks: ticks / 100.0
    rel = end - t0
    q = lambda v, f: float(np.quantile(v, f))
    print(f"waves {nw}  launch span (first start to last loop end) {us(span):.1f} us  start spread {us(int(start.max()) - t0):.1f} us")
    print(f"loop end, us after the first start: min {us(rel.min()):.1f}  median {us(q(rel, 0.5)):.1f}  p99 {us(q(rel, 0.99)):.1f}  max {us(rel.max()):.1f}")
    idle = t1 - end
    print(f"idle before the last wave's end: mean {us(idle.mean()):.1f} us = {100.0 * idle.mean() / span:.2f}% of the span, "
          f"median {us(q(idle, 0.5)):.1f} us, max {us(idle.max()):.1f} us = {100.0 * idle.max() / span:.2f}%")
    for x in range(8):
        r = rel[xcd == x]
        if r.size:
            print(f"  XCD {x}: waves {r.size:5d}  end min {us(r.min()):9.1f}  median {us(q(r, 0.5)):9.1f}  max {us(r.max()):9.1f}  "
                  f"mean idle {100.0 * (t1 - end[xcd == x]).mean() / span:.2f}%")
lib.fq_engine_destroy(h)
