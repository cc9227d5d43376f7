"""CPU checks of the star aggregate's ABI (hj.h "Star aggregate"): every symbol
is declared, bound with the right arity and exported, the Python side has its
names, and a null star is reported first -- before any device is touched -- by
all four entry points."""
import subprocess

import hashjoin
from hashjoin import _lib

L = hashjoin.lib
ARGC = {"hj_star_reserve_groups": 2, "hj_star_group_capacity": 1, "hj_dev_star_aggregate_i64": 18,
        "hj_dev_star_aggregate_i32": 18}


def test_star_aggregate_symbols_declared_bound_and_exported():
    names = hashjoin.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n, argc in ARGC.items():
        assert n in names, n
        assert len(getattr(L, n).argtypes) == argc, n
        assert n in exported, n
    text = open(_lib.HEADER_PATH).read()
    assert "Star aggregate" in text and text.index("Star aggregate") > text.index("Star probe")
    # the size the GPU tests take from here
    assert _lib.STAR_GROUP_MIN_CAPACITY == 2048


def test_python_side_has_the_names():
    assert hashjoin.star_aggregate is hashjoin.join.star_aggregate and "star_aggregate" in hashjoin.__all__
    for m in ("reserve_groups", "aggregate_into", "aggregate"):
        assert callable(getattr(hashjoin.StarProbe, m)), m
    assert isinstance(hashjoin.StarProbe.group_capacity, property)


def test_null_star_is_an_argument_error():
    # everything else wrong too: the star comes first
    calls = {"hj_star_reserve_groups": (None, -1),
             "hj_star_group_capacity": (None,),
             "hj_dev_star_aggregate_i64": (None, 9, None, None, None, None, None, None, None, -1, None, None, None, None,
                                           None, -1, None, None),
             "hj_dev_star_aggregate_i32": (None, 9, None, None, None, None, None, None, None, -1, None, None, None, None,
                                           None, -1, None, None)}
    for n, args in calls.items():
        assert getattr(L, n)(*args) == _lib.HJ_ERR_ARG, n
        assert b"null star" in L.hj_last_error(), n
