"""bench.py --dump-outputs (CPU): the files are float64, bounded in size, and
depend on the join's result pairs only, not on the order the join emitted
them in, so two builds that compute the same join write the same files."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = ("fingerprint", "out_r", "out_s", "result_rows", "sample_pos")


def load(d, suffix=""):
    assert sorted(os.listdir(d)) == sorted(f"{n}{suffix}.npy" for n in NAMES)
    return {n: np.load(os.path.join(d, f"{n}{suffix}.npy")) for n in NAMES}


@pytest.mark.parametrize("m", [0, 1, 1000, bench.DUMP_SAMPLE_ROWS, bench.DUMP_SAMPLE_ROWS + 3])
def test_dump_is_order_independent(tmp_path, m):
    g = torch.Generator().manual_seed(7)
    # repeated S rows (a duplicate-heavy join) so the second sort key matters
    s = torch.randint(0, max(1, m // 2), (m,), generator=g)
    r = torch.randint(0, 1 << 40, (m,), generator=g)
    p = torch.randperm(m, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), r, s, 0x5EED)
    bench.dump_outputs(str(tmp_path / "b"), r[p], s[p], 0x5EED)
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    for n in NAMES:
        assert a[n].dtype == np.float64
        assert np.array_equal(a[n], b[n]), n
    assert a["result_rows"].tolist() == [m]
    k = min(m, bench.DUMP_SAMPLE_ROWS)
    assert len(a["out_r"]) == len(a["out_s"]) == len(a["sample_pos"]) == k
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    # the sample is rows of the canonical order: sorted by (out_s, out_r)
    o = np.lexsort((r.numpy(), s.numpy()))
    pos = a["sample_pos"].astype(np.int64)
    assert np.array_equal(a["out_r"], r.numpy()[o][pos]) and np.array_equal(a["out_s"], s.numpy()[o][pos])
    assert int(a["fingerprint"][0]) + int(a["fingerprint"][1]) * (1 << 24) == int(r.sum())


def test_dump_sees_a_changed_pair(tmp_path):
    """One pair re-matched outside the sample still changes the fingerprint."""
    m = bench.DUMP_SAMPLE_ROWS + 3
    s = torch.arange(m)
    r = torch.arange(m).flip(0)
    bench.dump_outputs(str(tmp_path / "a"), r, s, 1)
    pos = set(np.load(tmp_path / "a" / "sample_pos.npy").astype(np.int64).tolist())
    i, j = [x for x in range(m) if x not in pos][:2]
    r2 = r.clone()
    r2[i], r2[j] = r[j], r[i]      # same columns as multisets, other pairs
    bench.dump_outputs(str(tmp_path / "b"), r2, s, 1, "_rank1")
    a, b = load(tmp_path / "a"), load(tmp_path / "b", "_rank1")
    assert np.array_equal(a["out_r"], b["out_r"]) and np.array_equal(a["fingerprint"][:4], b["fingerprint"][:4])
    assert a["fingerprint"][4] != b["fingerprint"][4]
