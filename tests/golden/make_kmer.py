#!/usr/bin/env python3
"""Generate the --kmer golden fixtures by running the REFERENCE binary (oracle/_ref/fqtool_ref,
built by oracle/Makefile.ref) with -w 1 on the existing inputs under tests/golden/inputs/ (which
tests/golden/make_e2e.py wrote; this script does not touch them).

For every case in CASES, tests/golden/kmer/manifest.json records (in the shape of the e2e
manifest) the arguments, the exit status, sha256 + line count of each (decompressed) output, the
error text of a failed run, and the reports:
  - k <= 5, or no effective k-mer length: the JSON and HTML report texts, gzipped ("json", "html");
  - larger k (a k = 8 report is 0.5 - 1.1 MB gzipped): only the sha256 of the report texts with
    the run-dependent parts masked as tests/e2e_util.py masks them ("json_sha256", "html_sha256").

Run from the repo root:  python3 tests/golden/make_kmer.py [case ...]
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "kmer")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from make_e2e import REF_BIN, run_case  # noqa: E402

TD_PE = "-i {in}/r1.fq.gz -I {in}/r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq "
EDGE_PE = "-i {in}/edge_r1.fq -I {in}/edge_r2.fq -o {out}/o1.fq -O {out}/o2.fq "
SYNTH_PE = "-i {in}/synth_r1.fq.gz -I {in}/synth_r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq "

# name -> (arguments, k-mer length the reports carry; 0 = none)
CASES = {
    "td_pe_k5": (TD_PE + "-q -a -g --kmer --kmer_length 5", 5),
    "td_pe_k6": (TD_PE + "-q -a -g --kmer --kmer_length 6", 6),
    "td_se_k8": ("-i {in}/r1.fq.gz -o {out}/o1.fq -q -a -g -x --kmer --kmer_length 8", 8),
    # kmer.kmerLen defaults to 0: --kmer alone counts nothing, the reports are the plain run's
    "td_pe_nolen": (TD_PE + "-q --kmer", 0),
    "td_pe_plain_q": (TD_PE + "-q", 0),
    "edge_pe_merge_k4": (EDGE_PE + "-q -a -g -m --merge_output {out}/merged.fq --kmer --kmer_length 4", 4),
    "edge_pe_correct_k5": (EDGE_PE + "-c -q -a -g -x --kmer --kmer_length 5", 5),
    "synth_pe_correct_umi_merge_k5": (SYNTH_PE + "-c -q -a -g -u --umi_location 6 --umi_length 6 -m "
                                      "--merge_output {out}/merged.fq --kmer --kmer_length 5", 5),
    "inter_k4": ("-i {in}/inter.fq --in_fq_interleaved -o {out}/o1.fq -q -g -x --kmer --kmer_length 4", 4),
    "td_pe_index_k4": (TD_PE + "-q -a -g --enable_index_filter --index1_file {in}/idx_a.txt "
                       "--index2_file {in}/idx_b.txt --kmer --kmer_length 4", 4),
    "err_kmer_needs": ("-i {in}/r1.fq.gz -o {out}/o1.fq --kmer_length 5", 0),
    "err_kmer_range": ("-i {in}/r1.fq.gz -o {out}/o1.fq --kmer --kmer_length 3", 0),
}


def main():
    if not os.path.exists(REF_BIN):
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    from e2e_util import mask_html, mask_software

    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:]
    manifest = {}
    if only:
        with open(os.path.join(OUT, "manifest.json")) as f:
            manifest = json.load(f)
    with tempfile.TemporaryDirectory() as tmp:
        for name, (args, k) in CASES.items():
            if only and name not in only:
                continue
            r = run_case(REF_BIN, name, args, tmp)
            r["k"] = k
            for kind, mask in (("json", mask_software), ("html", mask_html)):
                text = r[kind]
                r[kind] = None
                if text is None:
                    continue
                if k <= 5:
                    r[kind] = name + "." + kind + ".gz"
                    with gzip.GzipFile(os.path.join(OUT, r[kind]), "wb", compresslevel=9, mtime=0) as f:
                        f.write(text.encode())
                else:
                    r[kind + "_sha256"] = hashlib.sha256(mask(text).encode()).hexdigest()
            manifest[name] = r
            print(name, r["exit"], sorted(r["outputs"]), file=sys.stderr)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
