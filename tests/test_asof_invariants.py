"""CPU check of k_join_asof's compile-time invariant (hipcc front end only,
-fsyntax-only: no GPU): it is a user of the shared round shape, so a build
round loads exactly the rows it steps over."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlir-hashjoin_amd")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ARGS = "(JoinArgs, const void *, unsigned long long, unsigned long long);"


def _instantiate(tmp_path, inst):
    src = tmp_path / "inst.hip"
    src.write_text('#include "hj_radix.hip"\nnamespace hj { namespace { ' + inst + " } }\n")
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only",
                           "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", os.path.join(PKG, "csrc"),
                           str(src)], capture_output=True, text=True, timeout=300)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_asof_round_must_load_every_row(tmp_path):
    """768 threads do not divide a 5120-row round: the build rows past 4608
    would claim no slot, and a probe row whose nearest partner is among them
    would get an earlier one, or none."""
    bad = _instantiate(tmp_path, "template __global__ void k_join_asof<true, 768, 3, 6>" + ARGS)
    assert bad.returncode != 0
    assert "a build round must load exactly RCAP rows" in bad.stderr
    good = _instantiate(tmp_path, "template __global__ void k_join_asof<false, kAsofNT, kAsofSI, kAsofWPS, 3>" + ARGS)
    assert good.returncode == 0, good.stderr[-2000:]
