"""CPU checks of the star probe's ABI (hj.h "Star probe"): every symbol is
declared, bound with the right arity and exported, the kind constants and
HJ_STAR_MAX_DIMS agree between the header and the Python side, the Python side
has its names, and a null star is reported first -- before any device is
touched -- by every entry point."""
import subprocess

import hashjoin
from hashjoin import _lib

L = hashjoin.lib
ARGC = {"hj_star_create": 1, "hj_star_destroy": 1, "hj_star_reserve": 2, "hj_star_last_plan": 6,
        "hj_dev_star_i64": 12, "hj_dev_star_i32": 13}


def test_star_symbols_declared_bound_and_exported():
    names = hashjoin.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n, argc in ARGC.items():
        assert n in names, n
        assert len(getattr(L, n).argtypes) == argc, n
        assert n in exported, n


def test_star_constants():
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("HJ_STAR_MAX_DIMS", 4), ("HJ_STAR_INNER", 0), ("HJ_STAR_LEFT", 1), ("HJ_STAR_ANTI", 2)):
        assert f"#define {name} {value}" in text, name
        assert getattr(_lib, name) == value, name
    assert hashjoin.join.STAR_KINDS == {"inner": 0, "left": 1, "anti": 2}
    assert "typedef struct hj_star hj_star;" in text
    # the sizes the GPU tests take from here
    assert _lib.STAR_TILE == 2048 and _lib.STAR_LDS_TABLE_BYTES == 65536 and _lib.STAR_LDS_BUDGET_BYTES == 131072


def test_python_side_has_the_names():
    assert hashjoin.StarProbe is hashjoin.join.StarProbe and hashjoin.star_join is hashjoin.join.star_join
    for m in ("reserve", "probe_into", "probe", "count", "close"):
        assert callable(getattr(hashjoin.StarProbe, m)), m
    assert isinstance(hashjoin.StarProbe.last_plan, property)
    assert "StarProbe" in hashjoin.__all__ and "star_join" in hashjoin.__all__


def test_null_star_is_an_argument_error():
    # everything else wrong too: the star comes first
    calls = {"hj_star_reserve": (None, -1),
             "hj_star_last_plan": (None, None, None, None, None, None),
             "hj_dev_star_i64": (None, 9, None, None, None, None, -1, None, None, -1, None, None),
             "hj_dev_star_i32": (None, 9, None, None, None, None, -1, -1, None, None, -1, None, None)}
    for n, args in calls.items():
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG, n
        assert b"null star" in L.hj_last_error(), n
    L.hj_star_destroy(None)   # a no-op
