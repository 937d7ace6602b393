"""Write tests/golden/bns_cases.npz: small FASTA texts and the .ann / .amb / .pac bytes the reference's own bns_fasta2bntseq
(src/bntseq.cpp:269-372, for_only = 1, as bwa_idx_build_mem2 calls it) writes for them.

Run where the reference tree is present:
    python tests/make_bns_golden.py
It compiles bntseq.cpp, utils.cpp, kstring.cpp and memcpy_bwamem.cpp with the `scale` build's defines, a stand-in for the
un-vendored safestringlib (our own few lines, below) and a short main, all in a temporary directory.  Nothing of the
reference enters the repository; only the bytes it writes do.  Elsewhere it exits without writing anything.
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _ref_dir() -> str:
    """The reference sources: BWAMS_REF_SRC, else the REF default of oracle/Makefile (one place names the tree)."""
    if os.environ.get("BWAMS_REF_SRC"):
        return os.environ["BWAMS_REF_SRC"]
    for line in open(os.path.join(ROOT, "oracle", "Makefile")):
        m = re.match(r"\s*REF\s*\?=\s*(\S+)", line)
        if m:
            return m.group(1)
    return ""


REF = _ref_dir()
OUT = os.path.join(HERE, "golden", "bns_cases.npz")
DEFINES = ["-DMEMSCALE", "-DUSE_SHM", "-DPERFECT_MATCH", "-DSMEM_ACCEL", "-DDEFAULT_USE_ERT=1", "-DOPT_RW",
           "-DENABLE_PREFETCH", "-DV17=1", "-DSAIS=1"]

# the safestringlib calls these sources make, with the library's argument order
SAFE = r"""
#pragma once
#include <string.h>
#include <stddef.h>
#include <stdio.h>
typedef size_t rsize_t;
typedef int errno_t;
#define RSIZE_MAX_MEM (256UL << 20)
#define RSIZE_MAX_STR (4UL << 10)
static inline errno_t memcpy_s(void *d, rsize_t dm, const void *s, rsize_t n) { if (n > dm) return 1; memcpy(d, s, n); return 0; }
static inline errno_t memmove_s(void *d, rsize_t dm, const void *s, rsize_t n) { if (n > dm) return 1; memmove(d, s, n); return 0; }
static inline errno_t memset_s(void *d, rsize_t n, int v) { memset(d, v, n); return 0; }
static inline errno_t strcpy_s(char *d, rsize_t dm, const char *s) { if (strlen(s) >= dm) return 1; strcpy(d, s); return 0; }
static inline errno_t strncpy_s(char *d, rsize_t dm, const char *s, rsize_t n) { (void)dm; strncpy(d, s, n); d[n] = 0; return 0; }
static inline errno_t strcat_s(char *d, rsize_t dm, const char *s) { if (strlen(d) + strlen(s) >= dm) return 1; strcat(d, s); return 0; }
static inline errno_t strncat_s(char *d, rsize_t dm, const char *s, rsize_t n) { (void)dm; strncat(d, s, n); return 0; }
static inline rsize_t strnlen_s(const char *s, rsize_t m) { return strnlen(s, m); }
"""
PRE = "#include <x86intrin.h>\n#define __rdtsc __ref_rdtsc\n"
MAIN = r"""
#include <zlib.h>
#include <stdint.h>
#include "macro.h"
#include "bntseq.h"
uint64_t tprof[LIM_R][LIM_C];
int main(int argc, char **argv) { gzFile fp = gzopen(argv[1], "r"); bns_fasta2bntseq(fp, argv[2], 1); gzclose(fp); return 0; }
"""

# (name, FASTA text): every rule of kseq_read / add1 / the .pac tail
CASES = [
    ("issue_example", b"junk\n>chr1 first contig\nACGTNNNNacgtRYnnNNA\nCCGT\n>chr2\nNNNNGGGG\n\n>c3 x y\r\nAC\r\n\r\nGT\n>e\n>f\tt\nA-A A\n"),
    ("preamble_midline", b"xx yy zz>s1 c\nACGT\nNNAC\n"),
    ("at_headers", b"@a one\nACGTACGTAC\n@b\nTTTT\n>c two words\nGGCC\n"),
    ("tabs_and_spaces", b">t1\tcomment with\ttab\nAC GT\tAC\n>t2 \nACG\n"),
    ("crlf_file", b">r1 desc\r\nACGTN\r\nNNNA\r\n>r2\r\nGGGG\r\nCC\r\n"),
    ("lone_cr_first_base", b">x\n\r\nACGT\n>y\nA\n\r\nCG\n>z\n\n\r\nT\n"),
    ("empty_lines", b"\n\n>e1\n\n\nAC\n\n\nGT\n\n>e2\n\nT\n\n"),
    ("empty_contigs", b">e\n>f\n>g\nACGTA\n>h\n"),
    ("lowercase_runs", b">lc\nacgtnnnnacgtACGTnnnNNNnnn\nttttgggg\n"),
    ("iupac_codes", b">iu\nARYKMSWBDHVNaryk\nmswbdhvn\nACGT\n"),
    ("dash_and_dots", b">d\nAC--GT..NN-\n"),
    ("adjacent_distinct", b">ad\nNRNRRNNYYnN\n"),
    ("hole_across_contigs", b">h1\nACGTNNN\n>h2\nNNNACGT\n>h3\nNN\n>h4\nNNA\n"),
    ("lpac_mod0", b">m0\nACGTACGT\n"),
    ("lpac_mod1", b">m1\nACGTACGTA\n"),
    ("lpac_mod2", b">m2\nACGTACGTAC\n"),
    ("lpac_mod3", b">m3\nACGTACGTACG\n"),
    ("no_final_newline", b">nf comment\r\nACGTN\r\nNA\r"),
    ("long_wrapped", b">w1 wrapped\n" + b"".join(b"ACGTNacgtnRYACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTAC\n" for _ in range(40))
     + b">w2\n" + b"N" * 70 + b"\n" + b"ACGT" * 30 + b"\n"),
]


def main():
    if not REF or not os.path.exists(os.path.join(REF, "bntseq.cpp")):
        print(f"reference tree not present at {REF}: nothing written")
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        shim = os.path.join(tmp, "shim")
        os.makedirs(shim)
        for h in ("safe_lib.h", "safe_mem_lib.h", "safe_str_lib.h", "snprintf_s.h"):
            open(os.path.join(shim, h), "w").write(SAFE)
        open(os.path.join(tmp, "pre.h"), "w").write(PRE)
        open(os.path.join(tmp, "main.cpp"), "w").write(MAIN)
        exe = os.path.join(tmp, "fa2bns")
        srcs = [os.path.join(REF, f) for f in ("bntseq.cpp", "utils.cpp", "kstring.cpp", "memcpy_bwamem.cpp")]
        subprocess.check_call(["g++", "-O2", "-fpermissive", "-w", "-include", os.path.join(tmp, "pre.h")] + DEFINES +
                              ["-I" + REF, "-I" + shim, "-o", exe, os.path.join(tmp, "main.cpp")] + srcs + ["-lz", "-lpthread", "-lm", "-lrt"])
        out = {}
        for name, text in CASES:
            fa = os.path.join(tmp, name + ".fa")
            open(fa, "wb").write(text)
            pre = os.path.join(tmp, name)
            subprocess.check_call([exe, fa, pre])
            out[name + "/fa"] = np.frombuffer(text, np.uint8)
            for ext in ("ann", "amb", "pac"):
                out[name + "/" + ext] = np.frombuffer(open(pre + "." + ext, "rb").read(), np.uint8)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(CASES)} cases, {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
