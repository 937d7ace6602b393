"""host/pileup_vcf.cpp (the VCF text of rule 13's calls) built apart from the library with its own main (tools/pileup_vcf_check.cpp)
under -fsanitize=address,undefined and run on the CPU; what it prints against the literal texts of tests/test_pileup_calls.py, which
bwams/pileup.py gives too, and against rows written out here.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

import test_pileup_calls as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# REF above, between and below the two other alleles; the largest values of every field; a second reference of length 0
ORDERS = (TC.VCF_HEAD % ("##contig=<ID=chrA,length=2147483647>\n##contig=<ID=b,length=0>\n", "a sample") +
          "chrA\t7\t.\tC\tA\t0\t.\tDP=1\tGT:AD:DP:GQ:PL\t0/1:1,1:1:0:2,0,1\n"
          "chrA\t2147483647\t.\tC\tA,T\t2147483647\t.\tDP=4294967295\tGT:AD:DP:GQ:PL\t"
          "1/2:7,4294967295,4294967294:4294967295:99:2147483647,11,10,17,0,19\n"
          "chrA\t2147483647\t.\tT\tA,G\t5\t.\tDP=7\tGT:AD:DP:GQ:PL\t1/2:4,1,3:7:6:19,16,10,18,13,15\n"
          "chrA\t2147483647\t.\tA\tG,T\t5\t.\tDP=7\tGT:AD:DP:GQ:PL\t1/2:1,3,4:7:6:10,13,15,16,18,19\n")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pileupv") / "pileup_vcf_check")
    host = os.path.join(ROOT, "bwa-mem-scale_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + host, os.path.join(host, "pileup_vcf.cpp"),
                           os.path.join(ROOT, "tools", "pileup_vcf_check.cpp"), "-o", exe])
    return exe


def test_vcf(program):
    p = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    assert p.stdout.decode() == "== example\n" + TC.EX_VCF + "== hand\n" + TC.HAND_VCF + "== orders\n" + ORDERS + "== none\n" + TC.VCF_HEAD % ("", "")
    assert TC.example().vcf(TC.T.EX_NAMES, "s1") == TC.EX_VCF and TC.hand().vcf(TC.HAND_NAMES, "smp") == TC.HAND_VCF
