#!/usr/bin/env python3
"""tests/golden/extract_chr.npz from the REFERENCE ITSELF: the rule by which DNA_ExtractChrPileupData
(dna_sv_tensor/src/extract_chr_pileup_data/main.cpp) cuts a whole-genome mpileup text into <chr>.mpileup files.

Runs only in the development container, where the upstream tree is mounted read-only (NANOSNP_REFERENCE, default /root/reference):
the program is compiled into a temporary directory, run on one small text that holds the corner cases of its name rule (a space in
front of the tab, a leading tab, names that are prefixes of one another, a name that is not listed, a listed name in two runs, CRLF, no
final newline), and only its input and the files it wrote are kept - data, no program text.

    python tests/golden/make_golden_extract_chr.py
"""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("NANOSNP_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "dna_sv_tensor", "src")
WANTED = ["chr1", "chr10", "chr1_KI270706v1_random", "chrA", "chrS"]


def text():
    line = lambda name, p, sep=b"\t": name + sep + b"%d\tN\t3\tAc.\tIII" % p
    L = []
    L += [line(b"chr1", p) for p in range(1, 13)]
    L += [line(b"chr10", p) for p in range(1, 9)]
    L += [line(b"chr1_KI270706v1_random", p) for p in range(1, 7)]
    L += [line(b"chr1", p) for p in range(40, 44)]                     # chr1 a second time: its file is opened again with "w"
    L += [line(b"chrUn_unlisted", p) for p in range(1, 6)]
    L += [line(b"chrA", p) for p in range(1, 5)]
    L += [line(b"chrB_unlisted", p) for p in range(1, 4)]
    L += [line(b"chrA", p) for p in range(9, 12)]                      # A B A with B not listed
    L += [line(b"chrS", p, b" \t") for p in range(1, 4)]               # a space ends the name in front of the tab
    L += [line(b"chrS extra", p) for p in range(4, 6)]                 # the same name: what follows the space is not part of it
    L += [b"\tchrS\t7\tN\t1\tA\tI", b"\tchrS\t8\tN\t1\tA\tI"]          # a leading tab: the empty name
    L += [line(b"chr10", p) + b"\r" for p in range(20, 23)]            # CRLF lines (and chr10 a second time)
    L += [line(b"chr1_KI270706v1_random", 9)]                          # the text ends without a newline
    return b"\n".join(L)


def main():
    t = text()
    assert t.count(b"\n") < 200
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "extract_chr")
        subprocess.run(["g++", "-O1", "-std=c++11", "-o", exe, os.path.join(SRC, "extract_chr_pileup_data", "main.cpp"),
                        os.path.join(SRC, "common", "cpp_aux.cpp"), os.path.join(SRC, "common", "line_reader.cpp")], check=True)
        src, out = os.path.join(d, "pileup_data"), os.path.join(d, "out")
        os.mkdir(out)
        with open(src, "wb") as f:
            f.write(t)
        subprocess.run([exe, src, out] + WANTED, check=True, stderr=subprocess.DEVNULL)
        files = sorted(os.listdir(out))
        arrays = {"text": np.frombuffer(t, np.uint8), "wanted": np.array(WANTED), "files": np.array(files)}
        for k, name in enumerate(files):
            with open(os.path.join(out, name), "rb") as f:
                arrays[f"file_{k}"] = np.frombuffer(f.read(), np.uint8)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "extract_chr.npz"), **arrays)
    print("extract_chr.npz:", files)


if __name__ == "__main__":
    main()
