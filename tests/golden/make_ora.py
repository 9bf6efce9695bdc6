#!/usr/bin/env python3
"""Generate the --ora golden fixtures by running the REFERENCE binary (oracle/_ref/fqtool_ref,
built by oracle/Makefile.ref) with -w 1 on the inputs under tests/golden/inputs/ (the existing
ones, which tests/golden/make_e2e.py wrote, and the ora_* ones of tests/golden/make_ora_inputs.py;
this script touches neither).

For every case in CASES, tests/golden/ora/manifest.json records (in the shape of the e2e manifest)
the arguments, the exit status, sha256 + line count of each output, the error text of a failed run,
and the JSON and HTML report texts, gzipped ("json", "html").

The generated inputs must make the fixtures worth having; the script refuses to write them
otherwise (change tests/golden/make_ora_inputs.py then, not this condition): in at least one case
each of the four Stats sections lists >= 3 sequences of >= 3 different lengths, and in the -m case
MergedAndFiltered lists some.

Run from the repo root:  python3 tests/golden/make_ora.py [case ...]
"""
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ora")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from make_e2e import REF_BIN, run_case  # noqa: E402

TD_PE = "-i {in}/r1.fq.gz -I {in}/r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq -q -a -g "
ORA_PE = "-i {in}/ora_r1.fq.gz -I {in}/ora_r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq -q -a -g "

CASES = {
    # the real-data input: 18.7 k and 16.9 k hot sequences, nearly all 100-mers (large tables, the
    # elimination at scale), of which the reports list a few (the reference takes about a minute each)
    "td_pe": TD_PE + "--ora",
    "td_pe_s1": TD_PE + "--ora --ora_sample 1",
    "td_pe_merge_s7": TD_PE + "-m --merge_output {out}/merged.fq --ora --ora_sample 7",
    # an existing input where nothing is overrepresented: every section is null
    "synth_pe_null": "-i {in}/synth_r1.fq.gz -I {in}/synth_r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq -q -a -g --ora",
    # the generated pairs
    "ora_pe": ORA_PE + "--ora",
    "ora_pe_s1": ORA_PE + "--ora --ora_sample 1",
    "ora_pe_s7": ORA_PE + "--ora --ora_sample 7",
    "ora_pe_s100": ORA_PE + "--ora --ora_sample 100",
    "ora_se_s1": "-i {in}/ora_r1.fq.gz -o {out}/o1.fq -q -a -g -x --ora --ora_sample 1",
    "ora_pe_merge_s1": ORA_PE + "-m --merge_output {out}/merged.fq --ora --ora_sample 1",
    "ora_pe_merge_discard": ORA_PE + "-m --discard_unmerged --merge_output {out}/merged.fq --ora --ora_sample 3",
    "ora_pe_correct": ORA_PE + "-c --ora --ora_sample 2",
    "ora_pe_umi": ORA_PE + "-u --umi_location 6 --umi_length 6 --ora --ora_sample 2",
    "ora_pe_kmer": ORA_PE + "--kmer --kmer_length 5 --ora --ora_sample 5",
    "ora_inter": "-i {in}/ora_inter.fq.gz --in_fq_interleaved -o {out}/o1.fq -q -g --ora --ora_sample 2",
    "ora100_pe": "-i {in}/ora100_r1.fq.gz -I {in}/ora100_r2.fq.gz -o {out}/o1.fq -O {out}/o2.fq -q -a -g --ora --ora_sample 1",
    # the reference's own refusals
    "err_ora_sample_needs": "-i {in}/r1.fq.gz -o {out}/o1.fq --ora_sample 5",
    "err_ora_sample_range": "-i {in}/r1.fq.gz -o {out}/o1.fq --ora --ora_sample 0",
    "err_ora_sample_range_hi": "-i {in}/r1.fq.gz -o {out}/o1.fq --ora --ora_sample 10001",
}


def listed(report, section):
    o = (report.get(section) or {}).get("OverrepresentedSequences")
    return o or {}


def check_condition(reports):
    rich = False
    for name, rep in reports.items():
        secs = [listed(rep, s) for s in ("Read1BeforeFiltering", "Read2BeforeFiltering", "Read1AfterFiltering",
                                         "Read2AfterFiltering")]
        if all(len(s) >= 3 and len({len(k) for k in s}) >= 3 for s in secs):
            rich = True
    if not rich:
        sys.exit("no case lists >= 3 sequences of >= 3 lengths in all four Stats sections: change the generator")
    if not listed(reports["ora_pe_merge_s1"], "MergedAndFiltered"):
        sys.exit("the -m case's MergedAndFiltered lists nothing: change the generator")


def main():
    if not os.path.exists(REF_BIN):
        sys.exit("build the reference first: make -f oracle/Makefile.ref")
    os.makedirs(OUT, exist_ok=True)
    only = sys.argv[1:]
    manifest = {}
    if only:
        with open(os.path.join(OUT, "manifest.json")) as f:
            manifest = json.load(f)
    reports, texts = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, args in CASES.items():
            if only and name not in only:
                continue
            r = run_case(REF_BIN, name, args, tmp)
            if r["json"] is not None:
                reports[name] = json.loads(r["json"])
            for kind in ("json", "html"):
                texts[name, kind] = r[kind]
                r[kind] = (name + "." + kind + ".gz") if r[kind] is not None else None
            manifest[name] = r
            print(name, r["exit"], sorted(r["outputs"]),
                  {s: len(listed(reports[name], s)) for s in reports.get(name, {}) if "Filter" in s and s != "FilterResult"},
                  file=sys.stderr)
    if not only:
        check_condition(reports)
    for (name, kind), text in texts.items():
        if text is not None:
            with gzip.GzipFile(os.path.join(OUT, name + "." + kind + ".gz"), "wb", compresslevel=9, mtime=0) as f:
                f.write(text.encode())
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
