"""CPU checks of the star query's ABI (hj.h "Star query"): both symbols are
declared, bound with 19 arguments and exported; the Python struct is as large
as the header's under the host compiler; a null star is reported first, before
any device is touched; the Python side has its names."""
import ctypes as C
import os
import shutil
import subprocess

import hashjoin
from hashjoin import _lib

L = hashjoin.lib
NAMES = ("hj_dev_star_query_i64", "hj_dev_star_query_i32")


def test_star_query_symbols_declared_bound_and_exported():
    names = hashjoin.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in NAMES:
        assert n in names, n
        assert len(getattr(L, n).argtypes) == 19, n
        assert getattr(L, n).argtypes[8] == C.POINTER(_lib.StarFact), n   # fact goes right after gbase
        assert n in exported, n
    text = open(_lib.HEADER_PATH).read()
    assert "Star query" in text and text.index("Star query") > text.index("Star aggregate")
    for define in ("#define HJ_STAR_MAX_PREDS 4", "#define HJ_STAR_MAX_FACT_GROUPS 2", "#define HJ_PRED_IN  0",
                   "#define HJ_PRED_OUT 1", "#define HJ_VALUE_A   0", "#define HJ_VALUE_ADD 1", "#define HJ_VALUE_SUB 2",
                   "#define HJ_VALUE_MUL 3"):
        assert define in text, define
    assert (_lib.HJ_STAR_MAX_PREDS, _lib.HJ_STAR_MAX_FACT_GROUPS) == (4, 2)
    assert (_lib.HJ_PRED_IN, _lib.HJ_PRED_OUT) == (0, 1)
    assert (_lib.HJ_VALUE_A, _lib.HJ_VALUE_ADD, _lib.HJ_VALUE_SUB, _lib.HJ_VALUE_MUL) == (0, 1, 2, 3)


def test_struct_size_and_offsets_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a host C compiler"
    fields = [name for name, _ in _lib.StarFact._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hj.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(hj_star_fact));\n'
                   + "".join(f'    printf(" %zu", offsetof(hj_star_fact, {f}));\n' for f in fields)
                   + '    return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call([cc, "-I", os.path.dirname(_lib.HEADER_PATH), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(_lib.StarFact)
    assert got[1:] == [getattr(_lib.StarFact, f).offset for f in fields]


def test_null_star_is_an_argument_error():
    # everything else wrong too: the star comes first
    bad = _lib.StarFact()
    bad.npreds, bad.vop, bad.nfact = 9, 9, 9
    for n in NAMES:
        args = (None, 9, None, None, None, None, None, None, C.byref(bad), None, -1, None, None, None, None, None, -1,
                None, None)
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG, n
        assert b"null star" in L.hj_last_error(), n


def test_python_side_has_the_names():
    assert hashjoin.star_query is hashjoin.join.star_query and "star_query" in hashjoin.__all__
    for m in ("query_into", "query"):
        assert callable(getattr(hashjoin.StarProbe, m)), m
    assert hashjoin.join.STAR_PREDS == {"in": 0, "out": 1}
    assert hashjoin.join.STAR_VALUE_OPS == {"add": 1, "sub": 2, "mul": 3}
