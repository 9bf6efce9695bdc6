#!/usr/bin/env python3
"""Generate the --ora test inputs under tests/golden/inputs/ (seeded, so a rerun writes the same
bytes): 2000 pairs of 151-cycle reads with planted repeats of several lengths, so that every Stats
section of an --ora report lists sequences of several lengths, before and after filtering and in
merged reads:

  ora_r1.fq.gz / ora_r2.fq.gz      the pairs
  ora100_r1.fq.gz / ora100_r2.fq.gz  the same pairs cut to 100 cycles (the fifth step is then 98, which
                                   no hot sequence's length equals)
  ora_inter.fq.gz                  the first 1000 pairs interleaved

Planted, independently in read 1 and read 2 (read 2 has its own sequences):
  * a full-length duplicate population (the same 151 bases): hot 149-mers;
  * a 105-mer and a 44-mer at the start and a 22-mer at random positions of otherwise random reads:
    hot 100-, 40- and 20-mers whose shorter substrings the elimination drops;
  * a 22-mer carrying an N and two lower-case bases;
  * an adapter-dimer population: adapter, then a short insert, then the other adapter and poly-G;
  * a poly-A tail population.
About a third of the pairs overlap (inserts of 170 - 260 bases) so that -m merges them, and about
one pair in six has a low-quality mate and fails -q.

Run from the repo root:  python3 tests/golden/make_ora_inputs.py
"""
import gzip
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "inputs")
N = 2000
L = 151
COMP = bytes.maketrans(b"ACGTacgtN", b"TGCAtgcaN")
AD1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
AD2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"


def rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def plant(rng, read, piece):
    at = rng.randint(0, len(read) - len(piece))
    return read[:at] + piece + read[at + len(piece):]


def main():
    rng = random.Random(20240611)
    dup = [rand(rng, L), rand(rng, L)]
    p105 = [rand(rng, 105), rand(rng, 105)]
    p44 = [rand(rng, 44), rand(rng, 44)]
    p22 = [rand(rng, 22), rand(rng, 22)]
    odd = [b"ACGTNACGgTTAGCcATGCATG", b"TTGNCAtGGACCTAaGTCAGTC"]
    pairs = []
    for i in range(N):
        if rng.random() < 0.35:  # an overlapping pair
            ins = rng.randint(170, 260)
            frag = rand(rng, ins)
            r = [frag[:L], frag[-L:].translate(COMP)[::-1]]
        else:
            r = [rand(rng, L), rand(rng, L)]
        kind = rng.random()  # (plants go into either sort of pair)
        if kind < 0.04:
            r = [dup[0], dup[1]]
        elif kind < 0.09:
            r = [p105[m] + r[m][105:] for m in range(2)]  # (at the read's start, as a primer is)
        elif kind < 0.17:
            r = [p44[m] + r[m][44:] for m in range(2)]
        elif kind < 0.33:
            r = [plant(rng, r[m], p22[m]) for m in range(2)]
        elif kind < 0.49:
            r = [plant(rng, r[m], odd[m]) for m in range(2)]
        elif kind < 0.55:  # adapter dimer: a 12-base insert between the adapters
            ins = rand(rng, 12)
            r = [(ins + AD1 + b"G" * L)[:L], (ins.translate(COMP)[::-1] + AD2 + b"G" * L)[:L]]
        elif kind < 0.70:
            r = [r[m][:L - t] + b"A" * t for m, t in ((0, rng.randint(30, 70)), (1, rng.randint(30, 70)))]
        q = [b"I" * L, b"I" * L]
        if rng.random() < 0.17:
            m = rng.randrange(2)
            q[m] = b"I" * 60 + b"#" * (L - 60)
        pairs.append((r, q))

    def write(name, mates, cut, count=N):
        with gzip.GzipFile(os.path.join(OUT, name), "wb", compresslevel=9, mtime=0) as f:
            for i in range(count):
                r, q = pairs[i]
                for m in mates:
                    f.write(b"@ora.%d %d\n%s\n+\n%s\n" % (i + 1, m + 1, r[m][:cut], q[m][:cut]))

    write("ora_r1.fq.gz", [0], L)
    write("ora_r2.fq.gz", [1], L)
    write("ora100_r1.fq.gz", [0], 100)
    write("ora100_r2.fq.gz", [1], 100)
    write("ora_inter.fq.gz", [0, 1], L, 1000)


if __name__ == "__main__":
    main()
