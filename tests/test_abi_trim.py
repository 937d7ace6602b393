"""The trimming structs of include/bwams.h as the C compiler lays them out, against what ctypes and numpy see in bwams/capi.py, and the
library's default options against the restatement's (no compute without a GPU)."""
import ctypes as C
import dataclasses
import os
import subprocess

import pytest

from bwams import capi, trim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def _c_layout(tmp_path, struct, fields):
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf("{f} %zu\\n", offsetof({struct}, {f}));\n' for f in fields)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "bwams.h"\nint main(void) {{\n    printf("sizeof %zu\\n", sizeof({struct}));\n'
                   f'{lines}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)]).decode().split()
    return dict(zip(out[0::2], map(int, out[1::2])))


@pytest.mark.parametrize("struct,ctype,size", [("bwams_trim_opt_t", capi.TrimOpt, 328), ("bwams_trim_stats_t", capi.TrimStats, 176)])
def test_ctypes_struct_equals_the_header(tmp_path, struct, ctype, size):
    names = [n for n, _ in ctype._fields_]
    want = _c_layout(tmp_path, struct, names)
    assert want.pop("sizeof") == C.sizeof(ctype) == size
    assert want == {n: getattr(ctype, n).offset for n in names}


def test_report_dtype_equals_the_header(tmp_path):
    for dt in (capi.TRIM_READ_DTYPE, trim.READ_DTYPE):
        want = _c_layout(tmp_path, "bwams_trim_read_t", list(dt.names))
        assert want.pop("sizeof") == dt.itemsize == 40
        assert want == {n: dt.fields[n][1] for n in dt.names}
    assert capi.TRIM_READ_DTYPE == trim.READ_DTYPE


def test_constants_equal_the_header():
    hdr = open(os.path.join(ROOT, "include", "bwams.h")).read()
    assert f"#define BWAMS_TRIM_OVERLAP_MAX_LEN {trim.OVERLAP_MAX_LEN}\n" in hdr
    assert f"#define BWAMS_TRIM_STEP_SKIPPED 0x{trim.STEP_SKIPPED:x}\n" in hdr
    assert "BWAMS_TRIM_KEPT = 0, BWAMS_TRIM_LEN = 1, BWAMS_TRIM_N = 2, BWAMS_TRIM_QUAL = 3, BWAMS_TRIM_MATE = 4" in hdr
    assert (trim.KEPT, trim.LEN, trim.N, trim.QUAL, trim.MATE) == (0, 1, 2, 3, 4)


def test_library_defaults_equal_the_restatement(lib):
    o = capi.trim_opt()
    for f in dataclasses.fields(trim.Opt):
        assert getattr(o, f.name) == f.default, f.name
    assert bytes(o.pad_) == b""
