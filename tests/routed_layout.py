"""N ranks' folded exchange emulated on one device (a helper module, not a
conftest; imported like test_abi's helpers).

The folded routing (include/hj.h "Folded routing") sends a row to part =
owner << sub | bin, the top log2(N) + sub bits of the radix hash.  An 8-GPU
run has N senders route their slices (hj_dev_route_i64), exchanges the rows
(hashjoin/dist.py RoutedExchange) and hands every owner, for a bin range
[b0, b1) of its 2^sub bins, the concatenation over senders s = 0 .. N-1 of
sender s's rows of parts q * F + b0 .. q * F + b1 - 1, with the count matrix
counts_s[q * F + b0 : q * F + b1] stacked into an (N, b1 - b0) tensor
(RoutedExchange.part_counts[k] / bounds[k]).  folded_join builds exactly those
buffers from N route() calls on one device and joins them owner by owner with
build_routed / probe_routed, so the receiving side sees nsrc = N sources
without a second GPU.

check_layout is the one statement of that layout: the CPU stand-in
(test_dist_gloo._CpuJoin) asserts it on what the product's exchange delivers,
and the GPU tests assert it on the buffers assembled from the real
hj_dev_route_i64 output."""
import numpy as np
import torch

GOLDEN = np.uint64(0x9E3779B97F4A7C15)   # radix_hash's multiplier (csrc/hj_internal.h)


def rparts(keys, bits):
    """Top `bits` bits of the radix hash key * 0x9E37...15 mod 2^64 (0 bits: 0)."""
    keys = np.asarray(keys)
    if bits == 0:
        return np.zeros(len(keys), np.int64)
    with np.errstate(over="ignore"):
        h = keys.astype(np.uint64) * GOLDEN
    return (h >> np.uint64(64 - bits)).astype(np.int64)


def check_layout(t, counts, bin0, nranks, sub, owner):
    """Rows of source s, bin bin0 + j sit where counts (nsrc x nbins) says,
    and carry `owner`'s bits and that bin.  t: (n, 2) rows, host."""
    g = nranks.bit_length() - 1
    keys = np.asarray(t)[:, 0]
    part = rparts(keys, g + sub)
    c = np.asarray(counts)
    assert c.ndim == 2 and c.sum() == len(keys)
    # row by row: the part the counts place there (sources outermost, bins in order)
    want = np.repeat(np.tile((owner << sub) | (bin0 + np.arange(c.shape[1])), c.shape[0]), c.ravel())
    bad = np.flatnonzero(part != want)
    assert bad.size == 0, "row %d holds part %d, the counts say %d" % (bad[0], part[bad[0]], want[bad[0]])


def slice_bounds(n, N):
    """N + 1 offsets cutting n rows into N deliberately uneven sender slices:
    slice 1 is empty and the last one holds a single row (N >= 3; two senders
    get 1 and n - 1 rows, one sender everything); the others' sizes go as
    1, 2, 3, ... so no two senders' bin counts agree."""
    if N == 1:
        return [0, n]
    if N == 2:
        return [0, min(1, n), n]
    tail = min(1, n)
    free = [s for s in range(N) if s not in (1, N - 1)]
    w = np.arange(1, len(free) + 1, dtype=np.float64)
    cut = np.floor(np.cumsum(w) / w.sum() * (n - tail)).astype(np.int64)
    sizes = np.zeros(N, np.int64)
    sizes[free] = np.diff(np.concatenate([[0], cut]))
    sizes[N - 1] = tail
    assert sizes.sum() == n
    return np.concatenate([[0], np.cumsum(sizes)]).tolist()


class Routed:
    """Every sender's routed rows and part counts of one relation, and the
    receive buffers an exchange would assemble from them."""

    def __init__(self, hj, key, pay, N, sub, bounds=None):
        self.N, self.sub, self.F = N, sub, 1 << sub
        self.bounds = slice_bounds(key.shape[0], N) if bounds is None else list(bounds)
        assert len(self.bounds) == N + 1
        self.rows, self.counts, self.off = [], [], []
        for s in range(N):
            a, b = self.bounds[s], self.bounds[s + 1]
            t, c = hj.route(key[a:b], pay[a:b], N, sub)
            assert t.shape == (b - a, 2) and c.shape == (N << sub,)
            self.rows.append(t)
            self.counts.append(c)
            self.off.append(np.concatenate([[0], np.cumsum(c.cpu().numpy())]).astype(np.int64))

    def received(self, q, b0=0, b1=None):
        """Owner q's receive buffer of bins [b0, b1) and its (N, b1 - b0) counts."""
        b1 = self.F if b1 is None else b1
        p0, p1 = q * self.F + b0, q * self.F + b1
        t = torch.cat([self.rows[s][self.off[s][p0]:self.off[s][p1]] for s in range(self.N)])
        c = torch.stack([self.counts[s][p0:p1] for s in range(self.N)]).contiguous()
        return t, c


def probe_exact(probe, rows, device, cap=None):
    """probe(out_r, out_s) -> count tensor, into outputs of max(1, rows) (or
    cap) rows, once more at the exact M if that was too small; a count with
    bit 63 set (hj.h: a work list overflowed) is an error."""
    cap = max(1, rows if cap is None else cap)
    for _ in range(2):
        o_r = torch.empty(cap, dtype=torch.int64, device=device)
        o_s = torch.empty_like(o_r)
        m = int(probe(o_r, o_s).item())
        assert m >= 0, "count flagged (bit 63): %#x" % (m & ((1 << 64) - 1))
        if m <= cap:
            return o_r[:m], o_s[:m]
        cap = m
    raise AssertionError("output did not fit at the exact M")


def folded_join(hj, rk, rp, sk, sp, N, sub, s_parts=1, bounds_r=None, bounds_s=None, check=True):
    """Split R and S into N sender slices, route each (hj.route), assemble
    every owner's receive buffers and join them with hj.build_routed /
    hj.probe_routed, S in s_parts bin ranges.  hj: a HashJoin or anything with
    its route / build_routed / probe_routed.  Returns one (o_r, o_s) per owner.

    check: assert check_layout on every buffer handed to the join."""
    R = Routed(hj, rk, rp, N, sub, bounds_r)
    S = Routed(hj, sk, sp, N, sub, bounds_s)
    F = 1 << sub
    s_parts = max(1, min(int(s_parts), F))
    outs = []
    for q in range(N):
        if hasattr(hj, "owner"):
            hj.owner = q   # (the CPU stand-in checks the layout itself, against this owner)
        t, c = R.received(q)
        if check:
            check_layout(t.cpu().numpy(), c.cpu().numpy(), 0, N, sub, q)
        hj.build_routed(t, c, N, sub)
        rs, ss = [], []
        for k in range(s_parts):
            b0, b1 = F * k // s_parts, F * (k + 1) // s_parts
            ts, cs = S.received(q, b0, b1)
            if check:
                check_layout(ts.cpu().numpy(), cs.cpu().numpy(), b0, N, sub, q)

            def probe(o_r, o_s, ts=ts, cs=cs, b0=b0):
                return hj.probe_routed(ts, cs, b0, o_r, o_s)
            o_r, o_s = probe_exact(probe, ts.shape[0], ts.device)
            rs.append(o_r); ss.append(o_s)
        outs.append((torch.cat(rs), torch.cat(ss)))
    return outs


def union(outs):
    """All owners' pairs as two host arrays."""
    return (np.concatenate([o[0].cpu().numpy() for o in outs]), np.concatenate([o[1].cpu().numpy() for o in outs]))
