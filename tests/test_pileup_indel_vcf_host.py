"""host/pileup_indel_vcf.cpp (the VCF text of rule 17's indel calls and its merge with the SNV rows) and host/pileup_vcf.cpp built
apart from the library with their own main (tools/pileup_indel_vcf_check.cpp) under -fsanitize=address,undefined and run on the CPU;
what it prints against the literal texts of tests/test_pileup_indels.py, which bwams/pileup.py gives too, and against rows written out
here: 32 inserted and 32 deleted bases, N in REF, an SNV and two indels at one position, the largest value of every field, no call at
all.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

import test_pileup_indels as TI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTREMES = (TI.VCF_HEAD % ("##contig=<ID=chrA,length=2147483647>\n##contig=<ID=b,length=0>\n", "a sample") +
            "chrA\t7\t.\tC\tA\t0\t.\tDP=1\tGT:AD:DP:GQ:PL\t0/1:1,1:1:0:2,0,1\n"
            "chrA\t7\t.\tG\tG" + "T" * 32 + "\t0\t.\tDP=1;INDEL\tGT:AD:DP:GQ:PL\t1/1:0,1:1:0:0,0,0\n"
            "chrA\t7\t.\tT\tT" + "ACGT" * 8 + "\t21\t.\tDP=9;INDEL\tGT:AD:DP:GQ:PL\t0/1:4,3:9:3:21,0,3\n"
            "chrA\t8\t.\tC\tA\t0\t.\tDP=1\tGT:AD:DP:GQ:PL\t0/1:1,1:1:0:2,0,1\n"
            "chrA\t2147483001\t.\tA\tA\t1\t.\tDP=1;INDEL\tGT:AD:DP:GQ:PL\t0/1:1,1:1:1:1,0,1\n"
            "chrA\t2147483647\t.\tT\tA,G\t5\t.\tDP=7\tGT:AD:DP:GQ:PL\t1/2:4,1,3:7:6:19,16,10,18,13,15\n"
            "chrA\t2147483647\t.\tA" + "ACGTNACGTNACGTNACGTNACGTNACGTNAC" + "\tA\t2147483647\t.\tDP=4294967295;INDEL\tGT:AD:DP:GQ:PL\t"
            "1/1:4294967295,4294967294:4294967295:99:2147483647,12,0\n")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pileupiv") / "pileup_indel_vcf_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "pileup_vcf.cpp"),
                           os.path.join(host, "pileup_indel_vcf.cpp"), os.path.join(ROOT, "tools", "pileup_indel_vcf_check.cpp"), "-o", exe])
    return exe


def test_indel_vcf(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode() == ("== example\n" + TI.EX_INDEL_VCF + "== all\n" + TI.EX_VCF_ALL + "== extremes\n" + EXTREMES +
                                 "== none\n" + TI.VCF_HEAD % ("", ""))
    want = TI.example()
    assert want.indel_vcf(TI.T.EX_NAMES, "s1") == TI.EX_INDEL_VCF and want.vcf_all(TI.T.EX_NAMES, "s1") == TI.EX_VCF_ALL
