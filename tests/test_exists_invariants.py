"""CPU check of k_join_exists's compile-time invariant (hipcc front end only,
-fsyntax-only: no GPU): a build round loads exactly the rows it steps over."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlir-hashjoin_amd")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _instantiate(tmp_path, inst):
    src = tmp_path / "inst.hip"
    src.write_text('#include "hj_radix.hip"\nnamespace hj { namespace { ' + inst + " } }\n")
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only",
                           "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", os.path.join(PKG, "csrc"),
                           str(src)], capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_exists_round_must_load_every_row(tmp_path):
    """768 threads do not divide a 5120-row round: RI = 6 rows per thread would
    load 4608 of the 5120 rows the run cursor steps over, and the rest would
    never be built (a semi-join would miss them, an anti-join emit them)."""
    bad = _instantiate(tmp_path, "template __global__ void k_join_exists<true, 768, 3, 6>(JoinArgs, unsigned);")
    assert bad.returncode != 0
    assert "a build round must load exactly RCAP rows" in bad.stderr
    good = _instantiate(tmp_path, "template __global__ void k_join_exists<false, kExistsNT, kExistsSI, kExistsWPS>"
                                  "(JoinArgs, unsigned);")
    assert good.returncode == 0, good.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lookup_round_must_load_every_row(tmp_path):
    """The same bad shape for k_join_lookup: the assert is the shared round
    shape's, so every kernel built on it refuses 768 threads."""
    bad = _instantiate(tmp_path, "template __global__ void k_join_lookup<true, 768, 3, 6>"
                                 "(JoinArgs, int *, unsigned long long, unsigned long long);")
    assert bad.returncode != 0
    assert "a build round must load exactly RCAP rows" in bad.stderr
