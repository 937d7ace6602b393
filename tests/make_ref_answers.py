"""Write tests/golden/ref_answers.npz: the answers of the reference objects (oracle/_ref) that the pinning tests ask for.

Run where the reference tree is present and oracle/_ref is built (`make -C oracle all`):
    python tests/make_ref_answers.py
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "bwa-mem-scale_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_answers  # noqa: E402
from oracle import loader  # noqa: E402

FILES = ["test_oracle_bsw.py", "test_oracle_ksw.py", "test_oracle_aln.py", "test_oracle_dedup.py", "test_oracle_chain.py",
         "test_oracle_pair.py", "test_oracle_emf.py", "test_oracle_fmi_ref.py", "test_oracle_kswv.py"]

if __name__ == "__main__":
    need = ["libref_emf.so", "libref_bwa.so", "libref_kswv.so"]
    if loader.ref_lib() is None or loader.ref_chain_lib() is None or loader.ref_fmi_lib() is None or \
            not all(os.path.exists(os.path.join(ROOT, "oracle", "_ref", f)) for f in need) or "avx512bw" not in loader._cpu_flags():
        raise SystemExit("oracle/_ref is not built: the answers can only be recorded from the reference objects")
    ref_answers.RECORD = True
    rc = pytest.main(["-q", "-p", "no:cacheprovider"] + [os.path.join(HERE, f) for f in FILES])
    if rc != 0:
        raise SystemExit(f"the pinning tests failed against the reference objects (pytest exit {rc}); nothing written")
    out = ref_answers.save()
    print(f"{ref_answers.PATH}: {len(out) // 4} tests, {os.path.getsize(ref_answers.PATH)} bytes")
