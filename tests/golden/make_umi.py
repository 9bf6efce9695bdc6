#!/usr/bin/env python3
"""Generate the UMI (-u) golden fixtures of the routed egress by running the REFERENCE binary
(oracle/_ref/fqtool_ref, built by oracle/Makefile.ref) with -w 1 on the existing inputs under
tests/golden/inputs/ (which tests/golden/make_e2e.py wrote; this script does not touch them).

The cases cover what the UMI cases of tests/golden/e2e do not: location 4 on pairs (the quality
part bounded by read 1's length), --umi_not_trim at locations 3 and 6, location 6 without
--umi_drop_comment on names with comments, location 5 with the failed and unpaired outputs,
location 3 with -m --discard_unmerged, a UMI longer than some reads (the edge inputs have reads of
1 and 2 bases), single end at location 3 with --failed_out, and -u without --umi_location (location
0: no tag and no cut, the run of the same options without -u).

For every case tests/golden/umi/manifest.json records (in the shape of the e2e manifest) the
arguments, the exit status, sha256 + line count of each output, and the names of the gzipped JSON
and HTML report texts next to it.

Run from the repo root:  python3 tests/golden/make_umi.py [case ...]
"""
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "umi")
sys.path.insert(0, HERE)

from make_e2e import REF_BIN, run_case  # noqa: E402

TD_PE = "-i {in}/r1.fq.gz -I {in}/r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq "
EDGE_PE = "-i {in}/edge_r1.fq -I {in}/edge_r2.fq -o {out}/o1.fq -O {out}/o2.fq "

CASES = {
    # location 4 on pairs: read 2's quality part is bounded by read 1's length
    "edge_pe_umi_r2": EDGE_PE + "-q -a -g -u --umi_location 4 --umi_length 9 --umi_skip_length 2 --failed_out {out}/failed.fq",
    "td_pe_umi_r2": TD_PE + "-q -a -u --umi_location 4 --umi_length 7",
    # --umi_not_trim at locations 3 and 6
    "edge_pe_umi_r1_notrim": EDGE_PE + "-q -g -u --umi_location 3 --umi_length 12 --umi_not_trim",
    "edge_pe_umi_perread_notrim": EDGE_PE + "-q -a -u --umi_location 6 --umi_length 10 --umi_skip_length 4 --umi_not_trim "
                                            "--failed_out {out}/failed.fq",
    # location 6 keeping the comments
    "td_pe_umi_perread_comment": TD_PE + "-q -a -g -u --umi_location 6 --umi_length 8 --unpaired_read1 {out}/u1.fq "
                                         "--unpaired_read2 {out}/u2.fq --failed_out {out}/failed.fq",
    # location 5 with the side outputs
    "td_pe_umi_perindex_side": TD_PE + "-q -a -u --umi_location 5 --failed_out {out}/failed.fq --unpaired_read1 {out}/u1.fq",
    # location 3 with -m --discard_unmerged
    "td_pe_umi_r1_discard": TD_PE + "-q -a -g -u --umi_location 3 --umi_length 6 --umi_skip_length 2 -m "
                                    "--merge_output {out}/merged.fq --discard_unmerged",
    # a UMI (+ skip) longer than some reads, pairs merged without --discard_unmerged
    "edge_pe_umi_long_merge": EDGE_PE + "-q -a -u --umi_location 6 --umi_length 40 --umi_skip_length 20 -m "
                                        "--merge_output {out}/merged.fq",
    "edge_pe_umi_long_drop": EDGE_PE + "-q -u --umi_location 6 --umi_length 60 --umi_drop_comment --failed_out {out}/failed.fq",
    # -u alone: location 0, nothing is tagged or cut
    "td_pe_umi_noloc": TD_PE + "-q -a -g -u",
    "edge_pe_umi_noloc_failed": EDGE_PE + "-q -u --umi_length 5 --failed_out {out}/failed.fq",
    # single end, location 3, failed output
    "edge_se_umi_r1_failed": "-i {in}/edge_r1.fq -o {out}/o1.fq -q -a -u --umi_location 3 --umi_length 12 --umi_skip_length 1 "
                             "--failed_out {out}/failed.fq",
}


def main():
    if not os.path.exists(REF_BIN):
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:]
    manifest = {}
    if only:
        with open(os.path.join(OUT, "manifest.json")) as f:
            manifest = json.load(f)
    with tempfile.TemporaryDirectory() as tmp:
        for name, args in CASES.items():
            if only and name not in only:
                continue
            r = run_case(REF_BIN, name, args, tmp)
            for kind in ("json", "html"):
                text = r[kind]
                r[kind] = None
                if text is not None:
                    r[kind] = name + "." + kind + ".gz"
                    with gzip.GzipFile(os.path.join(OUT, r[kind]), "wb", compresslevel=9, mtime=0) as f:
                        f.write(text.encode())
            manifest[name] = r
            print(name, r["exit"], sorted(r["outputs"]), file=sys.stderr)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
