"""Host-side mirror of the reference's join program over device tensors.

The reference's host functions (join_v2.mlir:25-199) map one-to-one:

    @allocateHashTable     -> HashJoin.allocate_hash_table   (hj_ctx_reserve)
    @initializeHashTable   -> HashJoin.build_table           (init + build
    @buildTable               kernels, hj_dev_build_*)
    @countRows             -> HashJoin.count_rows            (hj_dev_count_*)
    @probeRelation         -> HashJoin.probe_relation        (hj_dev_probe_*)
    @main's join sequence  -> HashJoin.join

Tensors are PyTorch device tensors (plumbing only: allocation and the HIP
stream); every computation runs in libhj.so's HIP kernels.  Key dtype picks
the table layout: int64 keys -> 64-bit key/payload columns, int32 keys -> the
reference's i32 keys with i32 row ids.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import torch

from ._lib import (HJ_ASOF_BACKWARD, HJ_ASOF_FORWARD, HJ_ASOF_STRICT, HJ_ERR_RANGE, HJ_EXISTS_ANTI, HJ_EXISTS_SEMI, HJ_EXPAND_INNER, HJ_EXPAND_OUTER, HJ_FILTER_PASS, HJ_FILTER_REJECT, HJ_GROUP_ALL, HJ_GROUP_MATCHED, HJ_KEYS_MAX_COLS, HJ_OK, HJ_OUTER_BUILD, HJ_OUTER_FULL, HJ_STAR_ANTI, HJ_STAR_INNER, HJ_STAR_LEFT, HJ_STAR_MAX_DIMS, HJ_STRATEGY_AUTO,
                   HJ_PRED_IN, HJ_PRED_OUT, HJ_STAR_MAX_FACT_GROUPS, HJ_STAR_MAX_PREDS, HJ_STRATEGY_GLOBAL, HJ_STRATEGY_RADIX, HJ_VALUE_ADD,
                   HJ_VALUE_MUL, HJ_VALUE_SUB, HJError, StarFact, check, lib)

STRATEGIES = {"auto": HJ_STRATEGY_AUTO, "global": HJ_STRATEGY_GLOBAL, "radix": HJ_STRATEGY_RADIX}
EXISTS_KINDS = {"semi": HJ_EXISTS_SEMI, "anti": HJ_EXISTS_ANTI}
FULL_KINDS = {"build": HJ_OUTER_BUILD, "full": HJ_OUTER_FULL}
GROUP_KINDS = {"matched": HJ_GROUP_MATCHED, "all": HJ_GROUP_ALL}
GROUP_AGGS = ("count", "sum", "min", "max")
EXPAND_KINDS = {"inner": HJ_EXPAND_INNER, "outer": HJ_EXPAND_OUTER}
FILTER_KINDS = {"pass": HJ_FILTER_PASS, "reject": HJ_FILTER_REJECT}
ASOF_DIRECTIONS = {"backward": HJ_ASOF_BACKWARD, "forward": HJ_ASOF_FORWARD}
STAR_KINDS = {"inner": HJ_STAR_INNER, "left": HJ_STAR_LEFT, "anti": HJ_STAR_ANTI}
STAR_PREDS = {"in": HJ_PRED_IN, "out": HJ_PRED_OUT}
STAR_VALUE_OPS = {"add": HJ_VALUE_ADD, "sub": HJ_VALUE_SUB, "mul": HJ_VALUE_MUL}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device, stream=None):
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return C.c_void_p(s.cuda_stream)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("hash join inputs must be contiguous device tensors")


def _flagged(m):
    """m, a count read back from the device, unless bit 63 flags it (hj.h)."""
    if m < 0:
        raise RuntimeError("hash join: internal work list overflow (count flagged)")
    return m


def _counted(cnt, sync):
    """A count form's result: the number (synchronises), or the device tensor."""
    return int(cnt.item()) if sync else cnt


def _tuples(t):
    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 2:
        raise ValueError("tuples must be an (n, 2) int64 tensor")


def _key_dtype(k):
    if k.dtype not in (torch.int64, torch.int32):
        raise TypeError("keys must be int32 or int64")


def _relation(skey, spay, row_base, payload_required):
    """The column forms' dispatch: ("i64", (key, payload, n)) or ("i32", (key, n, row_base)) -- the suffix of
    hj_dev_<op>_<suffix> and its leading relation arguments -- behind the payload checks of each form."""
    _key_dtype(skey)
    n = skey.numel()
    if skey.dtype == torch.int64:
        if spay is None and payload_required:
            raise ValueError("int64 probe needs an int64 payload column")
        if spay is not None and (spay.dtype != torch.int64 or spay.numel() != n):
            raise ValueError("int64 probe needs an int64 payload column of the same length")
        return "i64", (_ptr(skey), _ptr(spay), n)
    if spay is not None:
        raise ValueError("i32 joins carry row ids, not payloads (reference types)")
    return "i32", (_ptr(skey), n, int(row_base))


def _pair_outputs(out_r, out_s, dtype, what):
    """cap of a probe's two outputs: both, of one length and of `dtype`, or neither (the count form).
    dtype None: a tuples twin, which checks no dtype and answers either fault with one message."""
    both = (out_r is None) == (out_s is None)
    cap = 0 if out_r is None else out_r.numel()
    level = out_s is None or out_s.numel() == cap
    if dtype is None:
        if not both or not level:
            raise ValueError(f"{what} probe needs two outputs of one length, or neither to count")
        return cap
    if not both:
        raise ValueError(f"{what} probe needs both outputs, or neither to count")
    if not level:
        raise ValueError("output columns differ in length")
    for o in (out_r, out_s):
        if o is not None and o.dtype != dtype:
            raise ValueError(f"{what} outputs carry the probe key's dtype")
    return cap


def _sized(cap, alloc, probe, trim, what):
    """The capacity loop of every call that returns trimmed outputs: alloc(cap) makes the outputs, probe(outs)
    fills them and returns M as a checked int, trim(outs, M) is the result; a cap below M is grown to M once."""
    for _ in range(2):
        cap = max(1, cap)
        outs = alloc(cap)
        m = probe(outs)
        if m <= cap:
            return trim(outs, m)
        cap = m
    raise RuntimeError(f"{what} output did not fit after resizing")


class KeyCodec:
    """Composite keys (hj.h "Composite keys"): exact range packing of up to
    four int32 / int64 key columns into one int64 key that every join, probe
    and aggregate of HashJoin takes as it takes any int64 key -- build_table,
    probe_lookup, probe_expand, probe_group and the rest are called with
    pack()'s output directly.

        kc = KeyCodec([torch.int32, torch.int64])
        kc.observe([r_a, r_b]); kc.observe([s_a, s_b]); kc.seal()
        rk, sk = kc.pack([r_a, r_b]), kc.pack([s_a, s_b])

    observe every relation that will be packed, then seal, then pack / unpack;
    reset() starts over.  Columns are 1-D contiguous device tensors of the
    codec's dtypes and of one length.  info() (synchronises) tells whether the
    joint range fits 64 bits; while it does not, pack and unpack write nothing."""

    def __init__(self, dtypes, device=0):
        dtypes = tuple(dtypes)
        if not 1 <= len(dtypes) <= HJ_KEYS_MAX_COLS:
            raise ValueError(f"a key codec takes 1..{HJ_KEYS_MAX_COLS} columns")
        if any(d not in (torch.int32, torch.int64) for d in dtypes):
            raise TypeError("key columns must be int32 or int64")
        if not torch.cuda.is_available():
            raise RuntimeError("KeyCodec needs a HIP device (no CPU fallback)")
        self.dtypes = dtypes
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        bits = (C.c_int * len(dtypes))(*[64 if d == torch.int64 else 32 for d in dtypes])
        self._kc = lib.hj_keycodec_create(self.device.index, len(dtypes), bits)
        if not self._kc:
            raise HJError("hj_keycodec_create failed: " + lib.hj_last_error().decode())

    def close(self):
        if getattr(self, "_kc", None):
            lib.hj_keycodec_destroy(self._kc)
            self._kc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _cols(self, cols, what="columns"):
        """(pointer array, n) of a column set; raises TypeError / ValueError on a bad one."""
        cols = list(cols)
        if len(cols) != len(self.dtypes):
            raise ValueError(f"{what}: expected {len(self.dtypes)} columns, got {len(cols)}")
        for t, d in zip(cols, self.dtypes):
            if not isinstance(t, torch.Tensor) or t.dtype != d:
                raise TypeError(f"{what}: column dtypes must be {self.dtypes}")
            if not t.is_cuda or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"{what}: columns must be 1-D contiguous device tensors")
        n = cols[0].numel()
        if any(t.numel() != n for t in cols):
            raise ValueError(f"{what}: columns differ in length")
        return (C.c_void_p * len(cols))(*[t.data_ptr() for t in cols]), n

    def reset(self, stream=None):
        check(lib.hj_dev_keycodec_reset(self._kc, _stream(self.device, stream)), "hj_dev_keycodec_reset")

    def observe(self, cols, stream=None):
        """Fold one relation's key columns into the per-column [lo, hi]."""
        ptrs, n = self._cols(cols)
        check(lib.hj_dev_keycodec_observe(self._kc, ptrs, n, _stream(self.device, stream)), "hj_dev_keycodec_observe")

    def seal(self, stream=None):
        """Fix the plan (one tiny kernel; the widths stay on the device)."""
        check(lib.hj_dev_keycodec_seal(self._kc, _stream(self.device, stream)), "hj_dev_keycodec_seal")

    def pack(self, cols, out=None, stream=None):
        """The int64 key column of a relation's key columns; exactly len rows of `out` are written."""
        ptrs, n = self._cols(cols)
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or not out.is_cuda
              or not out.is_contiguous() or out.numel() < n):
            raise ValueError("out must be a contiguous int64 device tensor of at least the columns' length")
        check(lib.hj_dev_keycodec_pack(self._kc, ptrs, n, _ptr(out), _stream(self.device, stream)),
              "hj_dev_keycodec_pack")
        return out

    def pack_tuples(self, cols, pay, out=None, stream=None):
        """(n, 2) int64 {key, pay} rows: the exchange format of build_tuples / probe_tuples."""
        ptrs, n = self._cols(cols)
        if (not isinstance(pay, torch.Tensor) or pay.dtype != torch.int64 or not pay.is_cuda or pay.dim() != 1
                or not pay.is_contiguous() or pay.numel() != n):
            raise ValueError("pay must be a 1-D contiguous int64 device tensor of the columns' length")
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or not out.is_cuda
              or not out.is_contiguous() or out.numel() < 2 * n):
            raise ValueError("out must be a contiguous int64 device tensor of at least 2 x the columns' length")
        check(lib.hj_dev_keycodec_pack_tuples(self._kc, ptrs, _ptr(pay), n, _ptr(out), _stream(self.device, stream)),
              "hj_dev_keycodec_pack_tuples")
        return out

    def unpack(self, keys, outs=None, stream=None):
        """The key columns of packed keys (the inverse of pack): a list with one
        tensor per column.  outs: a list of output tensors of the codec's
        dtypes, None entries are skipped (and stay None in the result)."""
        if (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or not keys.is_cuda or keys.dim() != 1
                or not keys.is_contiguous()):
            raise ValueError("keys must be a 1-D contiguous int64 device tensor")
        n = keys.numel()
        if outs is None:
            outs = [torch.empty(n, dtype=d, device=self.device) for d in self.dtypes]
        outs = list(outs)
        if len(outs) != len(self.dtypes):
            raise ValueError(f"outs: expected {len(self.dtypes)} entries")
        for t, d in zip(outs, self.dtypes):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != d:
                raise TypeError(f"outs: column dtypes must be {self.dtypes}")
            if not t.is_cuda or not t.is_contiguous() or t.numel() < n:
                raise ValueError("outs: contiguous device tensors of at least the keys' length")
        ptrs = (C.c_void_p * len(outs))(*[None if t is None else t.data_ptr() for t in outs])
        check(lib.hj_dev_keycodec_unpack(self._kc, _ptr(keys), n, ptrs, _stream(self.device, stream)),
              "hj_dev_keycodec_unpack")
        return outs

    def info(self):
        """The sealed plan (synchronises): {"total_bits", "bits", "lo", "hi",
        "rows_observed", "rows_out_of_range", "fits"}; fits is False when the
        joint range needs more than 64 bits (HJ_ERR_RANGE) -- the widths say
        which column is to blame."""
        total = C.c_int(0)
        bits = (C.c_int * 4)()
        lo = (C.c_int64 * 4)()
        hi = (C.c_int64 * 4)()
        rows, oor = C.c_uint64(0), C.c_uint64(0)
        rc = lib.hj_keycodec_info(self._kc, C.byref(total), bits, lo, hi, C.byref(rows), C.byref(oor))
        if rc not in (HJ_OK, HJ_ERR_RANGE):
            check(rc, "hj_keycodec_info")
        k = len(self.dtypes)
        return {"total_bits": total.value, "bits": list(bits)[:k], "lo": list(lo)[:k], "hi": list(hi)[:k],
                "rows_observed": rows.value, "rows_out_of_range": oor.value, "fits": rc == HJ_OK}


class KeyFilter:
    """A key filter (hj.h "Key filter"): a split-block Bloom filter of a build
    side's keys, applied to a probe side before the expensive step.  No false
    negatives: a row that fails certainly has no partner.

        f = KeyFilter(n_keys=rkey.numel())          # 16 bits per key: ~0.13 % false positives
        f.clear(); f.insert(rkey)
        skey, spay = f.apply(skey, spay)            # the rows that may have a partner, in input order

    The words live in `words`, a torch.int64 tensor of nblocks * 4 elements
    that the filter uses in place, so the filters of several ranks combine
    with one bitwise-OR all-reduce of that tensor (or merge() on one device).
    Keys are 1-D int64 or int32 columns or (n, 2) int64 {key, pay} tuples."""

    def __init__(self, n_keys=None, bits_per_key=16, nblocks=None, device=0, words=None):
        if words is not None:   # a filter over the caller's words (e.g. another rank's, gathered)
            if (not isinstance(words, torch.Tensor) or words.dtype != torch.int64 or not words.is_cuda
                    or not words.is_contiguous() or words.numel() % 4 or words.numel() == 0):
                raise ValueError("words must be a contiguous int64 device tensor of nblocks * 4 elements")
            nblocks, device = words.numel() // 4, words.device.index
        if nblocks is None:
            if n_keys is None:
                raise ValueError("a key filter needs n_keys or nblocks")
            nblocks = lib.hj_filter_blocks_for(int(n_keys), int(bits_per_key))
            if nblocks < 0:
                raise ValueError("key filter: " + lib.hj_last_error().decode())
        nblocks = int(nblocks)
        if not 1 <= nblocks < (1 << 31):
            raise ValueError("key filter: nblocks must be in [1, 2^31)")
        if not torch.cuda.is_available():
            raise RuntimeError("KeyFilter needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self.nblocks = nblocks
        self.bits_per_key = int(bits_per_key)
        self.words = torch.empty(nblocks * 4, dtype=torch.int64, device=self.device) if words is None else words
        self._merged = []
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._f = lib.hj_filter_create(self.device.index, nblocks, _ptr(self.words))
        if not self._f:
            raise HJError("hj_filter_create failed: " + lib.hj_last_error().decode())

    def close(self):
        for o in getattr(self, "_merged", []):
            o.close()
        self._merged = []
        if getattr(self, "_f", None):
            lib.hj_filter_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _form(keys, what="keys"):
        """'i64' | 'tuples' | 'i32' of a key tensor; raises on anything else."""
        if not isinstance(keys, torch.Tensor) or not keys.is_cuda or not keys.is_contiguous():
            raise ValueError(f"{what} must be a contiguous device tensor")
        if keys.dtype == torch.int64 and keys.dim() == 1:
            return "i64"
        if keys.dtype == torch.int64 and keys.dim() == 2 and keys.shape[1] == 2:
            return "tuples"
        if keys.dtype == torch.int32 and keys.dim() == 1:
            return "i32"
        raise TypeError(f"{what} must be a 1-D int64 / int32 column or (n, 2) int64 tuples")

    def reserve(self, rows):
        """Size apply's workspace for `rows` rows (grow-only); after it clear /
        insert / apply launch kernels only and can be captured in a graph."""
        check(lib.hj_filter_reserve(self._f, int(rows)), "hj_filter_reserve")

    def clear(self, stream=None):
        check(lib.hj_dev_filter_clear(self._f, _stream(self.device, stream)), "hj_dev_filter_clear")

    def insert(self, keys, stream=None):
        form = self._form(keys)
        f = {"i64": lib.hj_dev_filter_insert_i64, "tuples": lib.hj_dev_filter_insert_tuples_i64,
             "i32": lib.hj_dev_filter_insert_i32}[form]
        check(f(self._f, _ptr(keys), keys.shape[0], _stream(self.device, stream)), "hj_dev_filter_insert")

    def merge(self, other, stream=None):
        """self |= other (same nblocks, same device)."""
        check(lib.hj_dev_filter_merge(self._f, other._f, _stream(self.device, stream)), "hj_dev_filter_merge")

    def merge_words(self, words, stream=None):
        """self |= a filter given as its words tensor (nblocks * 4 int64, this
        device).  The wrapper object lives until close(): the merge is
        asynchronous and destroying a filter waits for the device."""
        other = KeyFilter(words=words)
        self._merged.append(other)
        self.merge(other, stream=stream)

    def apply_into(self, skey, spay=None, kind="pass", out_key=None, out_pay=None, out_row=None, count=None,
                   row_base=0, stream=None):
        """The raw call: writes min(M, cap) qualifying rows, in input order,
        into the outputs given (cap = their common length; none: the count
        form); `count` (int64 device tensor) receives M.  Returns count."""
        form = self._form(skey, "skey")
        outs = [o for o in (out_key, out_pay, out_row) if o is not None]
        _need_cuda(spay, *outs)
        cap = outs[0].shape[0] if outs else 0
        if any(o.shape[0] != cap for o in outs):
            raise ValueError("output columns differ in length")
        count = self._count if count is None else count
        st, k, n = _stream(self.device, stream), FILTER_KINDS[kind], skey.shape[0]
        if form == "i64":
            if spay is not None and (spay.dtype != torch.int64 or spay.numel() != n):
                raise ValueError("spay must be an int64 column of skey's length")
            check(lib.hj_dev_filter_apply_i64(self._f, k, _ptr(skey), _ptr(spay), n, _ptr(out_key), _ptr(out_pay),
                                              _ptr(out_row), cap, _ptr(count), st), "hj_dev_filter_apply_i64")
        elif form == "tuples":
            if spay is not None or out_pay is not None:
                raise ValueError("tuples carry their payloads")
            check(lib.hj_dev_filter_apply_tuples_i64(self._f, k, _ptr(skey), n, _ptr(out_key), _ptr(out_row), cap,
                                                     _ptr(count), st), "hj_dev_filter_apply_tuples_i64")
        else:
            if spay is not None or out_pay is not None:
                raise ValueError("i32 relations carry row ids, not payloads")
            check(lib.hj_dev_filter_apply_i32(self._f, k, _ptr(skey), n, int(row_base), _ptr(out_key), _ptr(out_row),
                                              cap, _ptr(count), st), "hj_dev_filter_apply_i32")
        return count

    def apply(self, skey, spay=None, kind="pass", with_rows=False, capacity=None, stream=None):
        """The rows of S whose key passes (kind='pass') / fails ('reject'),
        compacted in input order: the key column (tuples: the rows), then the
        payload column if spay is given, then the source positions (i32: row
        ids) if with_rows -- one tensor, or a tuple of them.  Outputs are sized
        |S| rows, or `capacity` with one more call at the exact M.
        Synchronises to read M."""
        form = self._form(skey, "skey")
        n = skey.shape[0]

        def alloc(cap):
            return (torch.empty((cap, 2) if form == "tuples" else (cap,), dtype=skey.dtype, device=self.device),
                    torch.empty(cap, dtype=torch.int64, device=self.device) if spay is not None else None,
                    torch.empty(cap, dtype=skey.dtype, device=self.device) if with_rows else None)

        def trim(outs, m):
            outs = [o[:m] for o in outs if o is not None]
            return outs[0] if len(outs) == 1 else tuple(outs)

        return _sized(n if capacity is None else int(capacity), alloc,
                      lambda o: int(self.apply_into(skey, spay, kind, *o, stream=stream).item()), trim, "filter")

    def count(self, skey, kind="pass", stream=None, sync=True):
        """How many rows of S pass ('pass') / fail ('reject')."""
        return _counted(self.apply_into(skey, kind=kind, stream=stream), sync)


class StarProbe:
    """A star probe (hj.h "Star probe"): one pass of n probe rows (a fact
    table) over up to four built dimensions; the rows every dimension admits
    come back in input order with each dimension's payload beside them.

        star = StarProbe(0)
        rows, (d_pay, p_pay) = star.probe([(date_hj, f_date, "inner"), (part_hj, f_part, "left", -1)])

    A dimension is (HashJoin, skey, how[, null]): a context holding a build
    under the global strategy, this dimension's key column of the probe rows,
    how in "inner" | "left" | "anti", and for "left" the payload of a row
    without a partner (default -1).  The dimensions are walked in the order
    given: put the most selective first.  All key columns share a dtype (int64,
    or int32 for hj_dev_build_i32 builds) and a length."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("StarProbe needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._s = lib.hj_star_create(self.device.index)
        if not self._s:
            raise HJError("hj_star_create failed: " + lib.hj_last_error().decode())

    def close(self):
        if getattr(self, "_s", None):
            lib.hj_star_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, rows):
        """Size the workspace for `rows` probe rows (grow-only); after it the
        probes launch kernels only and can be captured in a graph."""
        check(lib.hj_star_reserve(self._s, int(rows)), "hj_star_reserve")

    @property
    def last_plan(self):
        """Host facts of the last probe: kernel launches, the probe launch's
        grid and tiles, the dimensions probed from LDS (a list of booleans up
        to the highest one set; lds_mask the bits) and their tables' bytes."""
        la, g, ld = C.c_int(0), C.c_int(0), C.c_int(0)
        t, b = C.c_int64(0), C.c_int64(0)
        check(lib.hj_star_last_plan(self._s, C.byref(la), C.byref(g), C.byref(t), C.byref(ld), C.byref(b)),
              "hj_star_last_plan")
        return dict(launches=la.value, grid=g.value, tiles=t.value, lds_mask=ld.value,
                    lds_dims=[bool((ld.value >> d) & 1) for d in range(HJ_STAR_MAX_DIMS)], lds_bytes=b.value)

    @staticmethod
    def _dims(dims, least=1):
        """(contexts, key columns, kinds, nulls) of a dimension list; raises on a malformed one."""
        if not least <= len(dims) <= HJ_STAR_MAX_DIMS:
            raise ValueError(f"a star probe takes {least}..{HJ_STAR_MAX_DIMS} dimensions")
        hjs, keys, kinds, nulls = [], [], [], []
        for d in dims:
            if len(d) not in (3, 4):
                raise ValueError("a dimension is (HashJoin, skey, how[, null])")
            hj, skey, how = d[:3]
            if not isinstance(hj, HashJoin):
                raise TypeError("a dimension's first element is the HashJoin holding its build")
            if not isinstance(skey, torch.Tensor) or skey.dim() != 1 or skey.dtype not in (torch.int64, torch.int32):
                raise TypeError("a dimension's key column must be a 1-D int64 / int32 tensor")
            _need_cuda(skey)
            hjs.append(hj)
            keys.append(skey)
            kinds.append(STAR_KINDS[how])
            nulls.append(int(d[3]) if len(d) == 4 and d[3] is not None else -1)
        if any(k.dtype != keys[0].dtype or k.numel() != keys[0].numel() for k in keys):
            raise ValueError("the dimensions' key columns must share a dtype and a length")
        return hjs, keys, kinds, nulls

    @staticmethod
    def _arrays(hjs, keys, kinds, nulls, wide):
        """The ctypes arrays (contexts, kinds, key columns, nulls) of _dims' lists; None each without a dimension."""
        nd = len(hjs)
        if not nd:
            return None, None, None, None
        return ((C.c_void_p * nd)(*[h._ctx for h in hjs]), (C.c_int * nd)(*kinds),
                (C.c_void_p * nd)(*[k.data_ptr() for k in keys]), ((C.c_int64 if wide else C.c_int32) * nd)(*nulls))

    def _grouped(self, nd, group, base, inputs, outs, what):
        """A grouped call's group / base as ctypes arrays (None each without a dimension) and its outputs' common
        length, all checked; `what` names the call in the messages."""
        group = [-1] * nd if group is None else [-1 if g is None else int(g) for g in group]
        base = [0] * nd if base is None else [int(b) for b in base]
        if len(group) != nd or len(base) != nd:
            raise ValueError("group and base need one entry per dimension")
        outs = [o for o in outs if o is not None]
        _need_cuda(*inputs, *outs)
        if any(o.dtype != torch.int64 or o.dim() != 1 for o in outs):
            raise ValueError(f"the {what}'s output columns are int64")
        cap = outs[0].shape[0] if outs else 0
        if any(o.shape[0] != cap for o in outs):
            raise ValueError("output columns differ in length")
        return (C.c_int * nd)(*group) if nd else None, (C.c_int64 * nd)(*base) if nd else None, cap

    def _collect(self, into, aggs, max_groups, capacity, what):
        """{"key": tensor, agg: tensor, ...} trimmed to G from into(out_key, out_cnt, out_sum, out_min, out_max):
        into() counts the groups first unless a capacity is given; one below G is grown to G and the call repeated."""
        if any(a not in GROUP_AGGS for a in aggs):
            raise ValueError("aggs are among 'count', 'sum', 'min', 'max'")
        if max_groups is not None:
            self.reserve_groups(max_groups)

        def groups(cnt):
            g = int(cnt.item())
            if g < 0:   # bit 63 (hj.h)
                raise HJError(f"{what}: more groups than the group table of {self.group_capacity} slots "
                              "admits (reserve_groups)")
            return g

        return _sized(groups(into()) if capacity is None else int(capacity),
                      lambda cap: {c: torch.empty(cap, dtype=torch.int64, device=self.device) for c in ("key", *aggs)},
                      lambda o: groups(into(o["key"], o.get("count"), o.get("sum"), o.get("min"), o.get("max"))),
                      lambda o, g: {c: t[:g] for c, t in o.items()}, what)

    def probe_into(self, dims, out_pay=None, out_row=None, count=None, row_base=0, stream=None):
        """The raw call: writes min(M, cap) qualifying rows, in input order,
        into the outputs given -- out_pay a list with one column or None per
        dimension, out_row the source positions (i32: row ids) -- cap being
        their common length (none: the count form); `count` (int64 device
        tensor) receives M.  Returns count."""
        hjs, keys, kinds, nulls = self._dims(dims)
        nd, dt, n = len(dims), keys[0].dtype, keys[0].numel()
        out_pay = [None] * nd if out_pay is None else list(out_pay)
        if len(out_pay) != nd:
            raise ValueError("out_pay needs one entry (a column or None) per dimension")
        outs = [o for o in out_pay + [out_row] if o is not None]
        _need_cuda(*outs)
        if any(o.dtype != dt or o.dim() != 1 for o in outs):
            raise ValueError("output columns take the key columns' dtype")
        cap = outs[0].shape[0] if outs else 0
        if any(o.shape[0] != cap for o in outs):
            raise ValueError("output columns differ in length")
        count = self._count if count is None else count
        a_ctx, a_kind, a_key, a_null = self._arrays(hjs, keys, kinds, nulls, dt == torch.int64)
        a_out = (C.c_void_p * nd)(*[None if o is None else o.data_ptr() for o in out_pay])
        st = _stream(self.device, stream)
        if dt == torch.int64:
            check(lib.hj_dev_star_i64(self._s, nd, a_ctx, a_kind, a_key, a_null, n, a_out, _ptr(out_row), cap,
                                      _ptr(count), st), "hj_dev_star_i64")
        else:
            check(lib.hj_dev_star_i32(self._s, nd, a_ctx, a_kind, a_key, a_null, n, int(row_base), a_out,
                                      _ptr(out_row), cap, _ptr(count), st), "hj_dev_star_i32")
        return count

    def probe(self, dims, capacity=None, row_base=0, stream=None):
        """(rows, [payload columns]): the source positions (i32: row ids) of
        the qualifying rows in input order and, per dimension, its payload
        column (None for an "anti" dimension).  Outputs are sized |S| rows, or
        `capacity` with one more call at the exact M.  Synchronises to read M."""
        _, keys, kinds, _ = self._dims(dims)
        n, dt = keys[0].numel(), keys[0].dtype

        def alloc(cap):   # (rows, one payload column per dimension)
            return (torch.empty(cap, dtype=dt, device=self.device),
                    [None if k == HJ_STAR_ANTI else torch.empty(cap, dtype=dt, device=self.device) for k in kinds])

        return _sized(n if capacity is None else int(capacity), alloc,
                      lambda o: int(self.probe_into(dims, o[1], o[0], row_base=row_base, stream=stream).item()),
                      lambda o, m: (o[0][:m], [None if p is None else p[:m] for p in o[1]]), "star probe")

    def count(self, dims, stream=None, sync=True):
        """How many rows qualify under every dimension."""
        return _counted(self.probe_into(dims, stream=stream), sync)

    # ---- star aggregate (hj.h "Star aggregate"): GROUP BY over the qualifying rows, one fused pass
    def reserve_groups(self, max_groups):
        """Size the group table for `max_groups` distinct groups (grow-only);
        after it aggregate_into launches kernels only and can be captured."""
        check(lib.hj_star_reserve_groups(self._s, int(max_groups)), "hj_star_reserve_groups")

    @property
    def group_capacity(self):
        """Slots of the group table (0 before the first reserve_groups)."""
        return int(lib.hj_star_group_capacity(self._s))

    def aggregate_into(self, dims, val=None, out_key=None, out_cnt=None, out_sum=None, out_min=None, out_max=None,
                       count=None, group=None, base=None, stream=None):
        """The raw call: one row (key, count, sum, min, max of val) per
        distinct group key over the rows every dimension admits, aligned at the
        same index of each int64 column passed (any may be None: not computed;
        all None counts the groups).  group: per dimension the bit position of
        its payload's field in the key, or -1 / None to leave it out (default:
        none -- one group); base: per dimension the value subtracted first
        (default 0).  val: a column of the key columns' dtype, needed for sum,
        min and max.  Needs reserve_groups.  `count` (int64 device tensor)
        receives G; negative: the group table overflowed (bit 63).  Returns count."""
        hjs, keys, kinds, nulls = self._dims(dims)
        nd, dt, n = len(dims), keys[0].dtype, keys[0].numel()
        a_shift, a_base, cap = self._grouped(nd, group, base, [val], (out_key, out_cnt, out_sum, out_min, out_max),
                                             "star aggregate")
        if val is not None and (val.dtype != dt or val.dim() != 1 or val.numel() != n):
            raise ValueError("the value column takes the key columns' dtype and length")
        count = self._count if count is None else count
        wide = dt == torch.int64
        a_ctx, a_kind, a_key, a_null = self._arrays(hjs, keys, kinds, nulls, wide)
        f = lib.hj_dev_star_aggregate_i64 if wide else lib.hj_dev_star_aggregate_i32
        check(f(self._s, nd, a_ctx, a_kind, a_key, a_null, a_shift, a_base, _ptr(val), n, _ptr(out_key), _ptr(out_cnt),
                _ptr(out_sum), _ptr(out_min), _ptr(out_max), cap, _ptr(count), _stream(self.device, stream)),
              "hj_dev_star_aggregate_i64" if wide else "hj_dev_star_aggregate_i32")
        return count

    def aggregate(self, dims, val=None, aggs=("count", "sum"), group=None, base=None, max_groups=None, capacity=None,
                  stream=None):
        """{"key": tensor, agg: tensor, ...} trimmed to G, for aggs among
        "count", "sum", "min", "max" (all int64).  max_groups: reserve_groups
        first (None: the table as it stands).  capacity=None counts the groups
        first and allocates exactly; a capacity below G is grown to G and the
        call repeated.  Raises HJError when the group table overflowed.
        Synchronises to read G."""
        def into(*o):   # (the count call passes no value column)
            return self.aggregate_into(dims, val if o else None, *o, group=group, base=base, stream=stream)

        return self._collect(into, aggs, max_groups, capacity, "star aggregate")

    # ---- star query (hj.h "Star query"): the star aggregate with fact-side predicates, a two-column value
    # expression and fact-side group fields in the same pass
    def query_into(self, dims, val=None, out_key=None, out_cnt=None, out_sum=None, out_min=None, out_max=None,
                   count=None, where=None, expr=None, fact_group=None, group=None, base=None, stream=None):
        """aggregate_into over the rows that also pass every predicate of
        `where` -- (col, lo, hi[, "in" | "out"]): lo <= col <= hi, or outside it
        -- with the value val <op> col_b under expr = (op, col_b), op in "add" |
        "sub" | "mul" (wrapping int64), and each fact_group entry (col, shift,
        base) adding the field (col - base) << shift to the group key.  Every
        fact column has the key columns' dtype and length.  dims may be empty:
        a filtered GROUP BY over the fact columns alone, dtype and length then
        taken from the first fact column given.  Returns count."""
        hjs, keys, kinds, nulls = self._dims(dims, least=0)
        nd = len(dims)
        where = [] if where is None else [tuple(w) for w in where]
        fact_group = [] if fact_group is None else [tuple(f) for f in fact_group]
        if len(where) > HJ_STAR_MAX_PREDS or any(len(w) not in (3, 4) for w in where):
            raise ValueError(f"where takes up to {HJ_STAR_MAX_PREDS} predicates (col, lo, hi[, 'in' | 'out'])")
        if len(fact_group) > HJ_STAR_MAX_FACT_GROUPS or any(len(f) != 3 for f in fact_group):
            raise ValueError(f"fact_group takes up to {HJ_STAR_MAX_FACT_GROUPS} entries (col, shift, base)")
        if expr is not None and (len(expr) != 2 or expr[0] not in STAR_VALUE_OPS):
            raise ValueError("expr is None or (op, col_b) with op in 'add', 'sub', 'mul'")
        fcols = [w[0] for w in where] + [f[0] for f in fact_group] + ([expr[1]] if expr is not None else [])
        shape = keys + [c for c in fcols + [val] if c is not None]
        if not shape:
            raise ValueError("a star query without a dimension needs a fact column")
        dt, n = shape[0].dtype, shape[0].numel()
        for c in shape:
            if not isinstance(c, torch.Tensor) or c.dim() != 1 or c.dtype != dt or c.numel() != n or \
                    dt not in (torch.int64, torch.int32):
                raise ValueError("the fact columns are 1-D int64 / int32 tensors of the key columns' dtype and length")
        a_shift, a_base, cap = self._grouped(nd, group, base, shape, (out_key, out_cnt, out_sum, out_min, out_max),
                                             "star query")
        fact = StarFact()
        fact.npreds = len(where)
        for p, w in enumerate(where):
            fact.pcol[p], fact.plo[p], fact.phi[p] = w[0].data_ptr(), int(w[1]), int(w[2])
            fact.pkind[p] = STAR_PREDS[w[3] if len(w) == 4 else "in"]
        if expr is not None:
            fact.vop, fact.vb = STAR_VALUE_OPS[expr[0]], _ptr(expr[1])
        fact.nfact = len(fact_group)
        for f, (col, shift, fbase) in enumerate(fact_group):
            fact.fcol[f], fact.fshift[f], fact.fbase[f] = col.data_ptr(), int(shift), int(fbase)
        count = self._count if count is None else count
        wide = dt == torch.int64
        a_ctx, a_kind, a_key, a_null = self._arrays(hjs, keys, kinds, nulls, wide)
        f = lib.hj_dev_star_query_i64 if wide else lib.hj_dev_star_query_i32
        check(f(self._s, nd, a_ctx, a_kind, a_key, a_null, a_shift, a_base, C.byref(fact), _ptr(val), n, _ptr(out_key),
                _ptr(out_cnt), _ptr(out_sum), _ptr(out_min), _ptr(out_max), cap, _ptr(count),
                _stream(self.device, stream)), "hj_dev_star_query_i64" if wide else "hj_dev_star_query_i32")
        return count

    def query(self, dims, val=None, aggs=("count", "sum"), where=None, expr=None, fact_group=None, group=None,
              base=None, max_groups=None, capacity=None, stream=None):
        """aggregate's dict over query_into: {"key": tensor, agg: tensor, ...}
        trimmed to G.  Raises HJError when the group table overflowed.
        Synchronises to read G."""
        kw = dict(where=where, expr=expr, fact_group=fact_group, group=group, base=base, stream=stream)
        return self._collect(lambda *o: self.query_into(dims, val, *o, **kw), aggs, max_groups, capacity, "star query")


class HashJoin:
    """One device's hash-join context (table workspace + phase timing)."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("HashJoin needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._ctx = lib.hj_ctx_create(self.device.index)
        if not self._ctx:
            raise RuntimeError("hj_ctx_create failed: " + lib.hj_last_error().decode())
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.key_bits = None
        self._routed = {}   # slot -> (rows, 2) int64 routed-tuple buffer (route(..., slot=))
        self.asof_out = None   # the last probe_asof's result column (the one it allocated when given none)

    def close(self):
        self._routed = {}
        if getattr(self, "_ctx", None):
            lib.hj_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------- workspace
    def allocate_hash_table(self, num_tuples, key_bits=64):
        """@allocateHashTable (join_v2.mlir:25-39): size the workspace once."""
        check(lib.hj_ctx_reserve(self._ctx, int(num_tuples), int(key_bits)), "hj_ctx_reserve")

    def reserve_probe(self, num_tuples, key_bits=64):
        check(lib.hj_ctx_reserve_probe(self._ctx, int(num_tuples), int(key_bits)), "hj_ctx_reserve_probe")

    def reserve_group(self, num_tuples, key_bits=64):
        """Size the global-table group probe's accumulators for builds of up to
        num_tuples rows (hj_ctx_reserve_group), so probe_group allocates nothing."""
        check(lib.hj_ctx_reserve_group(self._ctx, int(num_tuples), int(key_bits)), "hj_ctx_reserve_group")

    def reserve_aggregate(self, num_tuples, key_bits=64):
        """Size the workspace for aggregates of up to num_tuples rows under the
        current strategy (hj_ctx_reserve_aggregate), so aggregate_into allocates nothing."""
        check(lib.hj_ctx_reserve_aggregate(self._ctx, int(num_tuples), int(key_bits)), "hj_ctx_reserve_aggregate")

    def probe_hint(self, num_tuples):
        """The probe side's expected rows, given before the build (None or < 0:
        unknown).  AUTO spares a mid-size build the radix partition it keeps
        only for probe sides of >= 2^24 rows (hj_ctx_probe_hint)."""
        check(lib.hj_ctx_probe_hint(self._ctx, -1 if num_tuples is None else int(num_tuples)), "hj_ctx_probe_hint")

    def set_strategy(self, name, radix_bits=0):
        """'auto' | 'global' (one HBM table) | 'radix' (partitioned, LDS tables);
        radix_bits > 0 fixes the partition count to 2^radix_bits."""
        check(lib.hj_ctx_set_strategy(self._ctx, STRATEGIES[name]), "hj_ctx_set_strategy")
        check(lib.hj_ctx_set_radix_bits(self._ctx, int(radix_bits)), "hj_ctx_set_radix_bits")

    @property
    def strategy_used(self):
        return {HJ_STRATEGY_GLOBAL: "global", HJ_STRATEGY_RADIX: "radix"}.get(
            lib.hj_ctx_strategy_used(self._ctx), None)

    @property
    def capacity(self):
        return int(lib.hj_ctx_table_capacity(self._ctx))

    @property
    def radix_plan(self):
        """Fan-out bits per partition pass of the current radix build ([] for global)."""
        n = C.c_int(0)
        bits = (C.c_int * 3)()
        check(lib.hj_ctx_radix_plan(self._ctx, C.byref(n), bits), "hj_ctx_radix_plan")
        return [bits[i] for i in range(n.value)]

    @property
    def radix_passes(self):
        return len(self.radix_plan)

    def has_duplicates(self):
        r = lib.hj_ctx_build_has_duplicates(self._ctx)
        if r < 0:
            check(r, "hj_ctx_build_has_duplicates")
        return bool(r)

    JOIN_KERNELS = {1: "k_join_b", 2: "k_join_u", 3: "k_join_u_stream", 4: "k_join_grp", 5: "k_join",
                    6: "k_join_exists", 7: "k_join_lookup", 8: "k_join_group", 9: "aggregate",
                    10: "k_join_expand", 11: "k_join_asof"}

    @property
    def join_kernel(self):
        """Kernel of the last radix join (hj_ctx_join_kernel): 'k_join_b',
        'k_join_u_stream', 'k_join_grp', 'k_join', 'k_join_exists' (a radix
        semi- / anti-join), 'k_join_lookup' (a radix lookup), 'k_join_group' (a
        radix group probe), 'aggregate' (a radix hash aggregate: k_join_aggregate),
        'k_join_expand' (a radix expand), 'k_join_asof' (a radix as-of probe),
        or None (no radix join)."""
        r = lib.hj_ctx_join_kernel(self._ctx)
        if r < 0:
            check(r, "hj_ctx_join_kernel")
        return self.JOIN_KERNELS.get(r)

    def set_timing(self, enable=True):
        check(lib.hj_ctx_set_timing(self._ctx, 1 if enable else 0), "hj_ctx_set_timing")

    def last_timing(self):
        """ms of the last (init, build, probe, routing partition) launches and
        the probe's split into probe-side partitioning and the join kernel."""
        a = (C.c_float * 8)()
        check(lib.hj_ctx_last_timing_ex(self._ctx, a), "hj_ctx_last_timing_ex")
        return dict(zip(("init", "build", "probe", "partition", "probe_partition", "probe_join"), list(a)[:6]))

    def accumulate_timing(self, enable=True):
        """Per-step phase times with no host synchronisation between steps:
        each build starts a new event set (hj_ctx_timing_accumulate);
        timing_totals() sums them.  Enabling again drops what was recorded."""
        check(lib.hj_ctx_timing_accumulate(self._ctx, 1 if enable else 0), "hj_ctx_timing_accumulate")

    def timing_totals(self):
        """Summed ms of every build + probe step since accumulate_timing() or
        the last call (synchronises), with "steps": how many."""
        a = (C.c_float * 8)()
        n = C.c_longlong(0)
        check(lib.hj_ctx_timing_totals(self._ctx, a, C.byref(n)), "hj_ctx_timing_totals")
        d = dict(zip(("init", "build", "probe", "partition", "probe_partition", "probe_join"), list(a)[:6]))
        d["steps"] = n.value
        return d

    # -------------------------------------------------------------- phases
    def build_table(self, rkey, rpay=None, row_base=0, stream=None):
        """@initializeHashTable + @buildTable (join_v2.mlir:54-108)."""
        _need_cuda(rkey, rpay)
        st = _stream(self.device, stream)
        if rkey.dtype == torch.int64:
            if rpay is None or rpay.dtype != torch.int64 or rpay.numel() != rkey.numel():
                raise ValueError("int64 build needs an int64 payload column of the same length")
            check(lib.hj_dev_build_i64(self._ctx, _ptr(rkey), _ptr(rpay), rkey.numel(), st), "hj_dev_build_i64")
            self.key_bits = 64
        elif rkey.dtype == torch.int32:
            if rpay is not None:
                raise ValueError("i32 joins carry row ids, not payloads (reference types)")
            check(lib.hj_dev_build_i32(self._ctx, _ptr(rkey), rkey.numel(), int(row_base), st), "hj_dev_build_i32")
            self.key_bits = 32
        else:
            raise TypeError("keys must be int32 or int64")

    def _built(self, rkey, rpay, n_probe, stream, default=None):
        """build_table under the probe hint n_probe, as every build-then-probe method starts.  default "zeros" |
        "rows" (R's row index) stands in for the payload column an int64 build was given none of."""
        self.probe_hint(n_probe)
        try:
            if default is not None and rkey.dtype == torch.int64 and rpay is None:
                rpay = (torch.zeros_like(rkey) if default == "zeros"
                        else torch.arange(rkey.numel(), dtype=torch.int64, device=self.device))
            self.build_table(rkey, rpay, stream=stream)
        finally:
            self.probe_hint(None)

    def _pair_sized(self, dt, cap, probe, what):
        """_sized for the joins that return (out_r, out_s): probe(out_r, out_s) returns the count tensor."""
        return _sized(cap, lambda cap: (torch.empty(cap, dtype=dt, device=self.device),
                                        torch.empty(cap, dtype=dt, device=self.device)),
                      lambda o: _flagged(int(probe(*o).item())), lambda o, m: (o[0][:m], o[1][:m]), what)

    def build_tuples(self, tuples, stream=None):
        """Build from packed (n, 2) int64 {key, payload} rows (exchange format)."""
        _need_cuda(tuples)
        _tuples(tuples)
        check(lib.hj_dev_build_tuples_i64(self._ctx, _ptr(tuples), tuples.shape[0], _stream(self.device, stream)),
              "hj_dev_build_tuples_i64")
        self.key_bits = 64

    def count_rows(self, skey, stream=None, sync=True):
        """@countRows (join_v2.mlir:110-147): M, the result size."""
        _need_cuda(skey)
        st = _stream(self.device, stream)
        if skey.dtype == torch.int64:
            check(lib.hj_dev_count_i64(self._ctx, _ptr(skey), skey.numel(), _ptr(self._count), st), "hj_dev_count_i64")
        else:
            check(lib.hj_dev_count_i32(self._ctx, _ptr(skey), skey.numel(), _ptr(self._count), st), "hj_dev_count_i32")
        return int(self._count.item()) if sync else self._count

    def probe_relation(self, skey, spay=None, out_r=None, out_s=None, count=None, row_base=0, stream=None):
        """@probeRelation (join_v2.mlir:149-199).  Writes min(M, cap) rows into
        out_r / out_s; `count` (int64 device tensor) receives M.  Returns count."""
        _need_cuda(skey, spay, out_r, out_s)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        cap = 0 if out_r is None else out_r.numel()
        if out_s is not None and out_s.numel() != cap:
            raise ValueError("output columns differ in length")
        if skey.dtype == torch.int64:
            if spay is None or spay.dtype != torch.int64:
                raise ValueError("int64 probe needs an int64 payload column")
            check(lib.hj_dev_probe_i64(self._ctx, _ptr(skey), _ptr(spay), skey.numel(), _ptr(out_r), _ptr(out_s),
                                       cap, _ptr(count), st), "hj_dev_probe_i64")
        else:
            check(lib.hj_dev_probe_i32(self._ctx, _ptr(skey), skey.numel(), int(row_base), _ptr(out_r), _ptr(out_s),
                                       cap, _ptr(count), st), "hj_dev_probe_i32")
        return count

    def probe_tuples(self, tuples, out_r, out_s, count=None, stream=None):
        _need_cuda(tuples, out_r, out_s)
        count = self._count if count is None else count
        check(lib.hj_dev_probe_tuples_i64(self._ctx, _ptr(tuples), tuples.shape[0], _ptr(out_r), _ptr(out_s),
                                          out_r.numel(), _ptr(count), _stream(self.device, stream)),
              "hj_dev_probe_tuples_i64")
        return count

    # ---- semi- / anti-join probes (hj.h "Semi- and anti-join probes")
    def probe_exists(self, skey, spay=None, kind="semi", out_s=None, out_key=None, count=None, row_base=0,
                     stream=None):
        """EXISTS ('semi') / NOT EXISTS ('anti') probe of the built table: the S
        rows with / without a partner, each at most once.  Writes min(M, cap)
        S payloads (i32: row ids row_base + row) into out_s and, if given,
        their keys into out_key; `count` (int64 device tensor) receives M.
        out_s None is the count-only form.  Returns count."""
        _need_cuda(skey, spay, out_s, out_key)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        k = EXISTS_KINDS[kind]
        cap = 0 if out_s is None else out_s.numel()
        if out_key is not None and (out_s is None or out_key.numel() != cap):
            raise ValueError("out_key needs an out_s of the same length")
        for o in (out_s, out_key):
            if o is not None and o.dtype != skey.dtype:
                raise ValueError("exists outputs carry the probe key's dtype")
        sfx, rel = _relation(skey, spay, row_base, out_s is not None)
        name = "hj_dev_exists_" + sfx
        check(getattr(lib, name)(self._ctx, k, *rel, _ptr(out_key), _ptr(out_s), cap, _ptr(count), st), name)
        return count

    def probe_exists_tuples(self, tuples, kind, out_s, out_key=None, count=None, stream=None):
        """probe_exists over packed (n, 2) int64 {key, payload} rows."""
        _need_cuda(tuples, out_s, out_key)
        _tuples(tuples)
        count = self._count if count is None else count
        cap = 0 if out_s is None else out_s.numel()
        if out_key is not None and (out_s is None or out_key.numel() != cap):
            raise ValueError("out_key needs an out_s of the same length")
        check(lib.hj_dev_exists_tuples_i64(self._ctx, EXISTS_KINDS[kind], _ptr(tuples), tuples.shape[0], _ptr(out_key),
                                           _ptr(out_s), cap, _ptr(count), _stream(self.device, stream)),
              "hj_dev_exists_tuples_i64")
        return count

    def count_exists(self, skey, kind="semi", stream=None, sync=True):
        """How many S rows have ('semi') / have no ('anti') partner."""
        return _counted(self.probe_exists(skey, kind=kind, stream=stream), sync)

    def _exists_join(self, kind, rkey, skey, spay, rpay, with_keys, capacity, stream):
        self._built(rkey, rpay, skey.numel(), stream, "zeros")   # (the build ABI wants a column; never read here)
        return _sized(skey.numel() if capacity is None else int(capacity),
                      lambda cap: (torch.empty(cap, dtype=skey.dtype, device=self.device),
                                   torch.empty(cap, dtype=skey.dtype, device=self.device) if with_keys else None),
                      lambda o: _flagged(int(self.probe_exists(skey, spay, kind, *o, stream=stream).item())),
                      lambda o, m: (o[1][:m], o[0][:m]) if with_keys else o[0][:m], "exists")

    def semi_join(self, rkey, skey, spay=None, rpay=None, with_keys=False, capacity=None, stream=None):
        """Build R, then the S payloads (row ids for int32 keys) of the rows
        whose key R holds -- (keys, payloads) if with_keys.  The output is
        sized |S| rows, or `capacity` with one re-probe at the exact M."""
        return self._exists_join("semi", rkey, skey, spay, rpay, with_keys, capacity, stream)

    def anti_join(self, rkey, skey, spay=None, rpay=None, with_keys=False, capacity=None, stream=None):
        """As semi_join, for the S rows whose key R does not hold."""
        return self._exists_join("anti", rkey, skey, spay, rpay, with_keys, capacity, stream)

    # ---- positional lookup probe (hj.h "Positional lookup probe")
    def probe_lookup(self, skey, out_r=None, out_cnt=None, null=-1, count=None, stream=None):
        """One result per probe row, in input order: out_r[j] = the smallest R
        payload (i32: R row id) among the R rows with key skey[j], or `null`
        written verbatim; out_cnt[j] (int32) = how many there are.  Either
        output may be None, not both; each has the length of skey at least and
        only its first len(skey) elements are written.  `count` (int64 device
        tensor) receives the number of S rows with a partner.  Returns count."""
        _need_cuda(skey, out_r, out_cnt)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        n = skey.numel()
        _key_dtype(skey)
        if out_r is None and out_cnt is None and n > 0:
            raise ValueError("lookup needs out_r or out_cnt (count_exists counts the rows with a partner)")
        if out_r is not None and (out_r.dtype != skey.dtype or out_r.numel() < n):
            raise ValueError("out_r carries the probe key's dtype and at least its length")
        if out_cnt is not None and (out_cnt.dtype != torch.int32 or out_cnt.numel() < n):
            raise ValueError("out_cnt is an int32 column of at least the probe key's length")
        f, name = ((lib.hj_dev_lookup_i64, "hj_dev_lookup_i64") if skey.dtype == torch.int64
                   else (lib.hj_dev_lookup_i32, "hj_dev_lookup_i32"))
        check(f(self._ctx, _ptr(skey), n, int(null), _ptr(out_r), _ptr(out_cnt), _ptr(count), st), name)
        return count

    def lookup(self, rkey, rpay, skey, null=-1, with_counts=False, stream=None):
        """Build R, then probe_lookup: out_r of length |S| (the R payload each S
        key maps to, the smallest when R repeats the key, `null` when R lacks
        it), or (out_r, out_cnt) if with_counts.  int64 keys with rpay None:
        the payload is R's row index (the id -> index mapping); int32 keys
        always carry R's row ids.  Composite keys: pass KeyCodec.pack's
        output of both relations as rkey / skey."""
        self._built(rkey, rpay, skey.numel(), stream, "rows")
        out_r = torch.empty(skey.numel(), dtype=skey.dtype, device=self.device)
        out_cnt = torch.empty(skey.numel(), dtype=torch.int32, device=self.device) if with_counts else None
        _flagged(int(self.probe_lookup(skey, out_r, out_cnt, null=null, stream=stream).item()))
        return (out_r, out_cnt) if with_counts else out_r

    # ---- as-of probe (hj.h "As-of probe"): per probe row, the nearest partner at or before a bound
    def probe_asof(self, skey, sbound, out_r=None, direction="backward", strict=False, null=-1, count=None,
                   stream=None):
        """One result per probe row, in input order: out_r[j] = the largest R
        payload (i32: R row id) <= sbound[j] among the R rows with key skey[j]
        (direction "forward": the smallest >= it; strict: < / >), or `null`
        written verbatim.  skey and sbound share dtype and length; out_r has
        that dtype and at least that length, and only its first len(skey)
        elements are written.  out_r None: a fresh column, kept as
        self.asof_out.  `count` (int64 device tensor) receives the number of S
        rows with a candidate.  Returns count."""
        _need_cuda(skey, sbound, out_r)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        n = skey.numel()
        _key_dtype(skey)
        if sbound is None or sbound.dtype != skey.dtype or sbound.numel() != n:
            raise ValueError("sbound carries the probe key's dtype and length")
        if out_r is None:
            out_r = torch.empty(n, dtype=skey.dtype, device=self.device)
        elif out_r.dtype != skey.dtype or out_r.numel() < n:
            raise ValueError("out_r carries the probe key's dtype and at least its length")
        kind = ASOF_DIRECTIONS[direction] | (HJ_ASOF_STRICT if strict else 0)
        f, name = ((lib.hj_dev_asof_i64, "hj_dev_asof_i64") if skey.dtype == torch.int64
                   else (lib.hj_dev_asof_i32, "hj_dev_asof_i32"))
        check(f(self._ctx, kind, _ptr(skey), _ptr(sbound), n, int(null), _ptr(out_r), _ptr(count), st), name)
        self.asof_out = out_r
        return count

    def asof(self, rkey, rpay, skey, sbound, direction="backward", strict=False, null=-1, stream=None):
        """Build R, then probe_asof: out_r of length |S|.  int64 keys with rpay
        None: the payload is R's row index ("the last R row with this key at or
        before row b"); int32 keys always carry R's row ids."""
        self._built(rkey, rpay, skey.numel(), stream, "rows")
        out_r = torch.empty(skey.numel(), dtype=skey.dtype, device=self.device)
        _flagged(int(self.probe_asof(skey, sbound, out_r, direction=direction, strict=strict, null=null,
                                     stream=stream).item()))
        return out_r

    def asof_join(self, rkey, rtime, skey, stime, direction="backward", allow_exact_matches=True, tolerance=None,
                  stream=None):
        """pandas merge_asof(by=key, on=time) without its sortedness
        requirement: per S row, the index of the R row with its key whose time
        is the nearest at or before ("forward": at or after; "nearest": either,
        a distance tie going to backward) stime, or -1.  Among R rows of equal
        key and time backward takes the last and forward the first, as pandas
        does.  allow_exact_matches=False excludes equal times; tolerance drops
        matches further than it.  Plumbing over probe_asof: the build payload is
        (rtime - t0) << rowbits | row, with t0 the minimum over both time
        columns and rowbits the width of len(R) - 1; ValueError if that needs
        more than 63 bits."""
        if direction not in ("backward", "forward", "nearest"):
            raise ValueError("direction must be 'backward', 'forward' or 'nearest'")
        for t in (rkey, rtime, skey, stime):
            if t.dtype != torch.int64:
                raise TypeError("asof_join takes int64 key and time columns")
        if rtime.numel() != rkey.numel() or stime.numel() != skey.numel():
            raise ValueError("key and time columns of a relation share their length")
        nr, ns = rkey.numel(), skey.numel()
        none = torch.full((ns,), -1, dtype=torch.int64, device=self.device)
        if nr == 0 or ns == 0:
            return none
        t0 = min(int(rtime.min().item()), int(stime.min().item()))
        span = max(int(rtime.max().item()), int(stime.max().item())) - t0
        rowbits = (nr - 1).bit_length()
        if span.bit_length() + rowbits > 63:
            raise ValueError(f"asof_join: times spanning {span.bit_length()} bits and {rowbits} row bits do not "
                             "pack into 63 bits")
        low = (1 << rowbits) - 1
        rpay = ((rtime - t0) << rowbits) | torch.arange(nr, dtype=torch.int64, device=self.device)
        sbase = (stime - t0) << rowbits
        self._built(rkey, rpay, ns, stream)

        def probe(fwd):
            # backward: the low bits all ones admit every row of an equal time and the max takes the last;
            # without exact matches the low bits are zero and the compare strict.  forward: the mirror image
            ones = (not fwd) == bool(allow_exact_matches)
            out = torch.empty(ns, dtype=torch.int64, device=self.device)
            self.probe_asof(skey, sbase | low if ones else sbase, out, direction="forward" if fwd else "backward",
                            strict=not allow_exact_matches, null=-1, stream=stream)
            hit = out >= 0   # (payloads are non-negative)
            return hit, out & low, (out >> rowbits) + t0

        if direction == "nearest":
            hb, ib, tb = probe(False)
            hf, i_f, tf = probe(True)
            take_b = hb & (~hf | ((stime - tb) <= (tf - stime)))
            hit, idx, tm = hb | hf, torch.where(take_b, ib, i_f), torch.where(take_b, tb, tf)
        else:
            hit, idx, tm = probe(direction == "forward")
        if tolerance is not None:
            hit = hit & ((tm - stime).abs() <= int(tolerance))
        return torch.where(hit, idx, none)

    # ---- expand probe (hj.h "Expand probe"): all partners per probe row, as a CSR in input order
    def reserve_expand(self, num_tuples, key_bits=64):
        """Size the expand probe's count column and scan sums for probe sides of
        up to num_tuples rows (hj_ctx_reserve_expand), so probe_expand allocates nothing."""
        check(lib.hj_ctx_reserve_expand(self._ctx, int(num_tuples), int(key_bits)), "hj_ctx_reserve_expand")

    def probe_expand(self, skey, out_off, out_r=None, how="inner", null=-1, count=None, stream=None):
        """Every partner of every probe row, in input order: out_off (int64, at
        least len(skey) + 1 long; exactly that many are written) receives the
        segment starts and M, out_r[out_off[j] : out_off[j + 1]] the R payloads
        (i32: R row ids) of the R rows with key skey[j], in unspecified order
        inside the segment; how='outer' gives a row without a partner the one
        entry `null`.  Entries at or past len(out_r) are dropped; out_r None is
        the count form.  `count` (int64 device tensor) receives M.  Returns count."""
        _need_cuda(skey, out_off, out_r)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        n = skey.numel()
        _key_dtype(skey)
        if out_off is None or out_off.dtype != torch.int64 or out_off.numel() < n + 1:
            raise ValueError("out_off is an int64 column of at least len(skey) + 1 elements")
        if out_r is not None and out_r.dtype != skey.dtype:
            raise ValueError("out_r carries the probe key's dtype")
        cap = 0 if out_r is None else out_r.numel()
        f, name = ((lib.hj_dev_expand_i64, "hj_dev_expand_i64") if skey.dtype == torch.int64
                   else (lib.hj_dev_expand_i32, "hj_dev_expand_i32"))
        check(f(self._ctx, EXPAND_KINDS[how], _ptr(skey), n, int(null), _ptr(out_off), _ptr(out_r) if cap else None,
                cap, _ptr(count), st), name)
        return count

    def count_expand(self, skey, how="inner", stream=None):
        """The count form: (offsets, M) of probe_expand, nothing else written."""
        off = torch.empty(skey.numel() + 1, dtype=torch.int64, device=self.device)
        return off, _flagged(int(self.probe_expand(skey, off, None, how=how, stream=stream).item()))

    def expand(self, rkey, rpay, skey, how="inner", null=-1, stream=None):
        """Build R, then probe_expand sized exactly: (offsets, out_r), a CSR over
        S's rows in input order.  int64 keys with rpay None: the payload is R's
        row index; int32 keys always carry R's row ids.  Composite keys: pass
        KeyCodec.pack's output of both relations as rkey / skey."""
        self._built(rkey, rpay, skey.numel(), stream, "rows")
        off, m = self.count_expand(skey, how=how, stream=stream)
        out_r = torch.empty(m, dtype=skey.dtype, device=self.device)
        if m:
            self.probe_expand(skey, off, out_r, how=how, null=null, stream=stream)
        return off, out_r

    def ordered_join(self, rkey, rpay, skey, spay=None, how="inner", null=-1, stream=None):
        """The pandas-order merge: (out_r, out_s) with the pairs in S's order --
        how='inner' | 'left' ('left' keeps the S rows without a partner, with
        `null` as their R payload).  out_s repeats spay (the row index when
        None) over the segment lengths."""
        if how not in ("inner", "left"):
            raise ValueError("how must be 'inner' or 'left'")
        off, out_r = self.expand(rkey, rpay, skey, how="outer" if how == "left" else "inner", null=null,
                                 stream=stream)
        src = torch.arange(skey.numel(), dtype=torch.int64, device=self.device) if spay is None else spay
        out_s = torch.repeat_interleave(src, off[1:] - off[:-1], output_size=out_r.numel())
        return out_r, out_s

    # ---- group probe (hj.h "Group probe"): join, then aggregate per build row
    def _group_outputs(self, dt, out_r, out_cnt, out_sum, out_min, out_max):
        cols = (out_r, out_cnt, out_sum, out_min, out_max)
        passed = [o for o in cols if o is not None]
        cap = passed[0].numel() if passed else 0
        if any(o.numel() != cap for o in passed):
            raise ValueError("output columns differ in length")
        for o in (out_r, out_cnt, out_min, out_max):
            if o is not None and o.dtype != dt:
                raise ValueError("out_r, out_cnt, out_min and out_max carry the probe key's dtype")
        if out_sum is not None and out_sum.dtype != torch.int64:
            raise ValueError("out_sum is an int64 column")
        return cap

    def probe_group(self, skey, sval=None, how="matched", out_r=None, out_cnt=None, out_sum=None, out_min=None,
                    out_max=None, null=0, count=None, row_base=0, stream=None):
        """Group probe of the built table: one row per R row (how="all") or per
        R row with a partner (how="matched"), holding the R payload, and the
        count, wrapping int64 sum, signed min and max of sval over the S rows
        with its key, aligned at the same index of each column passed.  Any
        column may be None (not computed); all None counts only.  An empty
        group has count 0, sum 0 and min = max = `null` written verbatim.
        int32 keys: sval is the S row id row_base + row, out_sum stays int64.
        `count` (int64 device tensor) receives M.  Returns count."""
        _need_cuda(skey, sval, out_r, out_cnt, out_sum, out_min, out_max)
        st = _stream(self.device, stream)
        k = GROUP_KINDS[how]
        count = self._count if count is None else count
        _key_dtype(skey)
        cap = self._group_outputs(skey.dtype, out_r, out_cnt, out_sum, out_min, out_max)
        outs = (_ptr(out_r), _ptr(out_cnt), _ptr(out_sum), _ptr(out_min), _ptr(out_max))
        if skey.dtype == torch.int64:
            if sval is None and any(o is not None for o in (out_sum, out_min, out_max)):
                raise ValueError("sum / min / max need an int64 value column")
            if sval is not None and (sval.dtype != torch.int64 or sval.numel() != skey.numel()):
                raise ValueError("int64 probe needs an int64 value column of the same length")
            check(lib.hj_dev_group_i64(self._ctx, k, _ptr(skey), _ptr(sval), skey.numel(), int(null), *outs, cap,
                                       _ptr(count), st), "hj_dev_group_i64")
        else:
            if sval is not None:
                raise ValueError("i32 joins carry row ids, not values (reference types)")
            check(lib.hj_dev_group_i32(self._ctx, k, _ptr(skey), skey.numel(), int(row_base), int(null), *outs, cap,
                                       _ptr(count), st), "hj_dev_group_i32")
        return count

    def probe_group_tuples(self, tuples, how="matched", out_r=None, out_cnt=None, out_sum=None, out_min=None,
                           out_max=None, null=0, count=None, stream=None):
        """probe_group over packed (n, 2) int64 {key, value} rows."""
        _need_cuda(tuples, out_r, out_cnt, out_sum, out_min, out_max)
        _tuples(tuples)
        count = self._count if count is None else count
        cap = self._group_outputs(torch.int64, out_r, out_cnt, out_sum, out_min, out_max)
        check(lib.hj_dev_group_tuples_i64(self._ctx, GROUP_KINDS[how], _ptr(tuples), tuples.shape[0], int(null),
                                          _ptr(out_r), _ptr(out_cnt), _ptr(out_sum), _ptr(out_min), _ptr(out_max),
                                          cap, _ptr(count), _stream(self.device, stream)), "hj_dev_group_tuples_i64")
        return count

    def count_group(self, skey, how="matched", stream=None, sync=True):
        """M of the group probe: the R rows with a partner ("matched") or all of them."""
        return _counted(self.probe_group(skey, how=how, stream=stream), sync)

    def _agg_columns(self, cap, dt, names):
        """One empty output column of cap rows per name: the sum is int64, every other takes dt."""
        return {a: torch.empty(cap, dtype=torch.int64 if a == "sum" else dt, device=self.device) for a in names}

    def group_join(self, rkey, rpay, skey, sval, how="matched", aggs=("count", "sum"), null=0, capacity=None,
                   stream=None):
        """Build R, then probe_group into outputs of |R| rows (the most the
        result can hold) or `capacity`: returns (rpay, {agg: tensor}) trimmed
        to M, for aggs among "count", "sum", "min", "max".  int32 keys: rpay
        and sval are None (row ids).  Composite keys: pass KeyCodec.pack's
        output of both relations as rkey / skey."""
        if how not in GROUP_KINDS:
            raise ValueError("how must be 'matched' or 'all'")
        if any(a not in GROUP_AGGS for a in aggs):
            raise ValueError("aggs are among 'count', 'sum', 'min', 'max'")
        self._built(rkey, rpay, skey.numel(), stream)
        dt = torch.int64 if rkey.dtype == torch.int64 else torch.int32

        def probe(o):
            return _flagged(int(self.probe_group(skey, sval, how, o["r"], o.get("count"), o.get("sum"), o.get("min"),
                                                 o.get("max"), null=null, stream=stream).item()))

        return _sized(rkey.numel() if capacity is None else int(capacity),
                      lambda cap: self._agg_columns(cap, dt, ("r", *aggs)), probe,
                      lambda o, m: (o["r"][:m], {a: c[:m] for a, c in o.items() if a != "r"}), "group join")

    # ---- hash aggregate (hj.h "Hash aggregate"): GROUP BY key over one relation, no build
    def aggregate_into(self, key, val=None, out_key=None, out_cnt=None, out_sum=None, out_min=None, out_max=None,
                       count=None, row_base=0, stream=None):
        """GROUP BY key over one relation: one row per distinct key holding the
        key and the count, wrapping int64 sum, signed min and max of val over
        the rows with it, aligned at the same index of each column passed.  Any
        column may be None (not computed); out_key alone is DISTINCT, all None
        counts the distinct keys.  int32 keys: the value is the row id row_base
        + row (val stays None), out_sum stays int64.  Needs no build and leaves
        none: the context's table is taken, probes need a new build_table.
        `count` (int64 device tensor) receives M.  Returns count."""
        _need_cuda(key, val, out_key, out_cnt, out_sum, out_min, out_max)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        _key_dtype(key)
        cap = self._group_outputs(key.dtype, out_key, out_cnt, out_sum, out_min, out_max)
        outs = (_ptr(out_key), _ptr(out_cnt), _ptr(out_sum), _ptr(out_min), _ptr(out_max))
        if key.dtype == torch.int64:
            if val is not None and (val.dtype != torch.int64 or val.numel() != key.numel()):
                raise ValueError("int64 keys need an int64 value column of the same length")
            check(lib.hj_dev_aggregate_i64(self._ctx, _ptr(key), _ptr(val), key.numel(), *outs, cap, _ptr(count), st),
                  "hj_dev_aggregate_i64")
        else:
            if val is not None:
                raise ValueError("i32 rows carry row ids, not values (reference types)")
            check(lib.hj_dev_aggregate_i32(self._ctx, _ptr(key), key.numel(), int(row_base), *outs, cap, _ptr(count),
                                           st), "hj_dev_aggregate_i32")
        return count

    def aggregate_tuples_into(self, tuples, out_key=None, out_cnt=None, out_sum=None, out_min=None, out_max=None,
                              count=None, stream=None):
        """aggregate_into over packed (n, 2) int64 {key, value} rows."""
        _need_cuda(tuples, out_key, out_cnt, out_sum, out_min, out_max)
        _tuples(tuples)
        count = self._count if count is None else count
        cap = self._group_outputs(torch.int64, out_key, out_cnt, out_sum, out_min, out_max)
        check(lib.hj_dev_aggregate_tuples_i64(self._ctx, _ptr(tuples), tuples.shape[0], _ptr(out_key), _ptr(out_cnt),
                                              _ptr(out_sum), _ptr(out_min), _ptr(out_max), cap, _ptr(count),
                                              _stream(self.device, stream)), "hj_dev_aggregate_tuples_i64")
        return count

    def count_distinct(self, key, stream=None, sync=True):
        """The number of distinct keys (the aggregate's count-only form)."""
        return _counted(self.aggregate_into(key, stream=stream), sync)

    def aggregate(self, key, val=None, aggs=("count", "sum"), capacity=None, stream=None):
        """GROUP BY key: returns {"key": tensor, agg: tensor, ...} trimmed to M,
        for aggs among "count", "sum", "min", "max".  capacity=None counts the
        distinct keys first and allocates exactly; a capacity below M is grown
        to M and the call repeated.  int32 keys: val is None (row ids)."""
        if any(a not in GROUP_AGGS for a in aggs):
            raise ValueError("aggs are among 'count', 'sum', 'min', 'max'")
        dt = key.dtype

        def probe(o):
            return _flagged(int(self.aggregate_into(key, val, o["key"], o.get("count"), o.get("sum"), o.get("min"),
                                                    o.get("max"), stream=stream).item()))

        return _sized(self.count_distinct(key, stream=stream) if capacity is None else int(capacity),
                      lambda cap: self._agg_columns(cap, dt, ("key", *aggs)), probe,
                      lambda o, m: {c: t[:m] for c, t in o.items()}, "aggregate")

    def distinct(self, key, capacity=None, stream=None):
        """SELECT DISTINCT key: the distinct keys, in no particular order."""
        return self.aggregate(key, aggs=(), capacity=capacity, stream=stream)["key"]

    # ---- probe-side outer join (hj.h "Probe-side outer join")
    def probe_outer(self, skey, spay=None, out_r=None, out_s=None, null=-1, count=None, row_base=0, stream=None):
        """LEFT OUTER probe of the built table, S on the left: every pair of the
        inner join plus (null, S payload) for every S row without a partner.
        Writes min(M, cap) rows into out_r / out_s (i32: row ids, row_base +
        row on the S side); `count` (int64 device tensor) receives M >= |S|.
        `null` is written verbatim.  out_r and out_s None is the count-only
        form.  Returns count."""
        _need_cuda(skey, spay, out_r, out_s)
        st = _stream(self.device, stream)
        count = self._count if count is None else count
        cap = _pair_outputs(out_r, out_s, skey.dtype, "outer")
        sfx, rel = _relation(skey, spay, row_base, out_s is not None)
        name = "hj_dev_probe_outer_" + sfx
        check(getattr(lib, name)(self._ctx, *rel, int(null), _ptr(out_r), _ptr(out_s), cap, _ptr(count), st), name)
        return count

    def probe_outer_tuples(self, tuples, out_r, out_s, null=-1, count=None, stream=None):
        """probe_outer over packed (n, 2) int64 {key, payload} rows."""
        _need_cuda(tuples, out_r, out_s)
        _tuples(tuples)
        cap = _pair_outputs(out_r, out_s, None, "outer")
        count = self._count if count is None else count
        check(lib.hj_dev_probe_outer_tuples_i64(self._ctx, _ptr(tuples), tuples.shape[0], int(null), _ptr(out_r),
                                                _ptr(out_s), cap, _ptr(count), _stream(self.device, stream)),
              "hj_dev_probe_outer_tuples_i64")
        return count

    def count_outer(self, skey, stream=None, sync=True):
        """M of the outer probe: the inner join's pairs plus the S rows without a partner."""
        return _counted(self.probe_outer(skey, stream=stream), sync)

    def outer_join(self, rkey, rpay, skey, spay=None, null=-1, capacity=None, stream=None):
        """join() keeping every S row: build R, then the outer probe into an
        output sized |S| rows (exact when no S row has two partners), or
        `capacity`, re-probing once at the exact M if that was too small.
        Returns (R payloads or `null`, S payloads); row ids for int32 keys."""
        self._built(rkey, rpay, skey.numel(), stream)
        dt = torch.int64 if rkey.dtype == torch.int64 else torch.int32
        return self._pair_sized(dt, skey.numel() if capacity is None else int(capacity),
                                lambda o_r, o_s: self.probe_outer(skey, spay, o_r, o_s, null=null, stream=stream),
                                "outer join")

    # ---- build-side and full outer join (hj.h "Build-side and full outer join")
    def probe_full(self, skey, spay=None, out_r=None, out_s=None, kind="full", null_r=-1, null_s=-1, count=None,
                   row_base=0, stream=None):
        """RIGHT OUTER (kind="build") or FULL OUTER (kind="full") probe of the
        built table, S on the left: every pair of the inner join, plus
        (R payload, null_s) for every R row no S row of this call matches,
        plus (full only) (null_r, S payload) for every S row without a
        partner.  Writes min(M, cap) rows into out_r / out_s (i32: row ids,
        row_base + row on the S side); `count` (int64 device tensor) receives
        M.  Both null values are written verbatim.  out_r and out_s None is
        the count-only form.  Returns count."""
        _need_cuda(skey, spay, out_r, out_s)
        st = _stream(self.device, stream)
        k = FULL_KINDS[kind]
        count = self._count if count is None else count
        cap = _pair_outputs(out_r, out_s, skey.dtype, "full")
        sfx, rel = _relation(skey, spay, row_base, out_s is not None)
        name = "hj_dev_probe_full_" + sfx
        check(getattr(lib, name)(self._ctx, k, *rel, int(null_r), int(null_s), _ptr(out_r), _ptr(out_s), cap,
                                 _ptr(count), st), name)
        return count

    def probe_full_tuples(self, tuples, out_r, out_s, kind="full", null_r=-1, null_s=-1, count=None, stream=None):
        """probe_full over packed (n, 2) int64 {key, payload} rows."""
        _need_cuda(tuples, out_r, out_s)
        _tuples(tuples)
        cap = _pair_outputs(out_r, out_s, None, "full")
        count = self._count if count is None else count
        check(lib.hj_dev_probe_full_tuples_i64(self._ctx, FULL_KINDS[kind], _ptr(tuples), tuples.shape[0], int(null_r),
                                               int(null_s), _ptr(out_r), _ptr(out_s), cap, _ptr(count),
                                               _stream(self.device, stream)), "hj_dev_probe_full_tuples_i64")
        return count

    def count_full(self, skey, kind="full", stream=None, sync=True):
        """M of the full (or build-side) outer probe."""
        return _counted(self.probe_full(skey, kind=kind, stream=stream), sync)

    def full_join(self, rkey, rpay, skey, spay=None, how="full", null_r=-1, null_s=-1, capacity=None, stream=None):
        """join() keeping every R row and (how="full") every S row: build R,
        then the full probe into an output sized |S| + |R| rows (exact when
        no S row has two partners), or `capacity`, re-probing once at the
        exact M if that was too small.  Returns (R payloads or null_r, S
        payloads or null_s); row ids for int32 keys."""
        if how not in FULL_KINDS:
            raise ValueError("how must be 'full' or 'build'")
        self._built(rkey, rpay, skey.numel(), stream)
        dt = torch.int64 if rkey.dtype == torch.int64 else torch.int32
        return self._pair_sized(dt, skey.numel() + rkey.numel() if capacity is None else int(capacity),
                                lambda o_r, o_s: self.probe_full(skey, spay, o_r, o_s, kind=how, null_r=null_r,
                                                                 null_s=null_s, stream=stream), "full join")

    # ---- folded routing (hj.h "Folded routing"): the owner and the
    # receiver's first radix-pass bin from one hash, so receivers skip a pass
    @staticmethod
    def route_plan(n_build_global, nranks):
        """Bin bits per owner for a routed join (0: no fold -- use partition)."""
        b = C.c_int(0)
        check(lib.hj_route_plan(int(n_build_global), int(nranks), C.byref(b)), "hj_route_plan")
        return b.value

    def route(self, key, pay, nranks, sub_bits, stream=None, slot=None):
        """(n, 2) tuples grouped by (owner, bin), and the (nranks << sub_bits)
        part sizes (int64 device tensor).  slot (e.g. "r" / "s"): the tuples
        go to a buffer this HashJoin keeps for that slot -- allocated once,
        placement-probed (placed_rows) -- and stay valid until the slot's next
        route; None: a fresh tensor."""
        _need_cuda(key, pay)
        n = key.shape[0]
        if slot is None:
            out = torch.empty((n, 2), dtype=torch.int64, device=self.device)
        else:
            buf = self._routed.get(slot)
            if buf is None or buf.shape[0] < n:
                self._routed.pop(slot, None)
                buf = placed_rows(n, self.device)
                self._routed[slot] = buf
            out = buf[:n]
        counts = torch.empty(nranks << sub_bits, dtype=torch.int64, device=self.device)
        check(lib.hj_dev_route_i64(self._ctx, _ptr(key), _ptr(pay), n, nranks, sub_bits, _ptr(out), _ptr(counts),
                                   _stream(self.device, stream)), "hj_dev_route_i64")
        return out, counts

    def build_routed(self, tuples, counts, nranks, sub_bits, stream=None):
        """Build from routed tuples; counts: (nsrc, 2^sub_bits) int64 device
        tensor of every source's bin sizes (rows laid out source by source)."""
        _need_cuda(tuples, counts)
        check(lib.hj_dev_build_routed_i64(self._ctx, _ptr(tuples), tuples.shape[0], _ptr(counts), counts.shape[0],
                                          nranks, sub_bits, _stream(self.device, stream)), "hj_dev_build_routed_i64")
        self.key_bits = 64

    def probe_routed(self, tuples, counts, bin0, out_r, out_s, count=None, stream=None):
        """Probe routed tuples of bins [bin0, bin0 + counts.shape[1])."""
        _need_cuda(tuples, counts, out_r, out_s)
        count = self._count if count is None else count
        check(lib.hj_dev_probe_routed_i64(self._ctx, _ptr(tuples), tuples.shape[0], _ptr(counts), counts.shape[0],
                                          bin0, counts.shape[1], _ptr(out_r), _ptr(out_s), out_r.numel(), _ptr(count),
                                          _stream(self.device, stream)), "hj_dev_probe_routed_i64")
        return count

    def partition(self, key, pay=None, nparts=2, out=None, counts=None, stream=None):
        """Radix-route rows to nparts owners: packed (n, 2) tuples grouped by
        owner + per-owner counts (int64 device tensor)."""
        st = _stream(self.device, stream)
        n = key.shape[0]
        out = torch.empty((n, 2), dtype=torch.int64, device=self.device) if out is None else out
        counts = torch.empty(nparts, dtype=torch.int64, device=self.device) if counts is None else counts
        if pay is None:   # key is already packed tuples
            _need_cuda(key, out, counts)
            check(lib.hj_dev_partition_tuples_i64(self._ctx, _ptr(key), n, nparts, _ptr(out), _ptr(counts), st),
                  "hj_dev_partition_tuples_i64")
        else:
            _need_cuda(key, pay, out, counts)
            check(lib.hj_dev_partition_i64(self._ctx, _ptr(key), _ptr(pay), n, nparts, _ptr(out), _ptr(counts), st),
                  "hj_dev_partition_i64")
        return out, counts

    # -------------------------------------------------------------- whole join
    def join_rows(self, t1, t2, stream=None):
        """nested-loop.mlir (:29-192) on device: t1, t2 are 2-D int32 tensors
        (row-major, key in column 0); returns the (M, c1 + c2 - 1) int32 rows
        [X row, Y cols 1..] of every key match, X the larger table (ties: t1).
        Count first, then materialise exactly M rows.  Row strides may exceed
        the column count (column slices of wider tables)."""
        for t in (t1, t2):
            if not t.is_cuda:
                raise ValueError("hash join inputs must be device tensors")
            if t.dtype != torch.int32 or t.dim() != 2 or (t.numel() and t.stride(1) != 1):
                raise ValueError("tables must be 2-D int32 tensors with unit column stride")
        ld = [t.stride(0) if t.numel() else t.shape[1] for t in (t1, t2)]
        st = _stream(self.device, stream)
        args = (_ptr(t1), t1.shape[0], t1.shape[1], ld[0], _ptr(t2), t2.shape[0], t2.shape[1], ld[1])
        check(lib.hj_dev_count_rows_i32(self._ctx, *args, _ptr(self._count), st), "hj_dev_count_rows_i32")
        m = int(self._count.item())
        oc = t1.shape[1] + t2.shape[1] - 1
        out = torch.empty((max(m, 1), oc), dtype=torch.int32, device=t1.device)
        check(lib.hj_dev_join_rows_i32(self._ctx, *args, _ptr(out), oc, m, _ptr(self._count), st),
              "hj_dev_join_rows_i32")
        return out[:m]

    def join_host(self, rkey, rpay, skey, spay, device_budget=0, capacity=None):
        """Out-of-core join of host-resident int64 numpy columns (relations
        larger than HBM): routed into groups that fit `device_budget` bytes
        (0 = 80 % of free HBM), each built on the GPU with its probe side
        streamed through.  Returns host arrays (R.pay, S.pay)."""
        import numpy as np
        cols = [np.ascontiguousarray(a, np.int64) for a in (rkey, rpay, skey, spay)]
        if cols[0].shape != cols[1].shape or cols[2].shape != cols[3].shape:
            raise ValueError("key and payload columns must have equal lengths")
        cap = max(1, cols[2].size if capacity is None else int(capacity))
        for _ in range(2):
            out_r = np.empty(cap, np.int64); out_s = np.empty(cap, np.int64)
            m = lib.hj_host_join_ooc_i64(self._ctx, cols[0].ctypes.data, cols[1].ctypes.data, cols[0].size,
                                         cols[2].ctypes.data, cols[3].ctypes.data, cols[2].size,
                                         out_r.ctypes.data, out_s.ctypes.data, cap, int(device_budget))
            if m < 0:
                check(int(m), "hj_host_join_ooc_i64")
            if m <= cap:
                return out_r[:m], out_s[:m]
            cap = int(m)
        raise RuntimeError("out-of-core join output did not fit after resizing")

    CMP = {"lt": 0, "le": 1, "gt": 2, "ge": 3, "eq": 4, "ne": 5}

    def select(self, values, op, value, with_rows=False, stream=None):
        """Experiments/selection.mlir's query on device: the elements v of a
        float32 or int64 tensor with `v <op> value` ('lt' 'le' 'gt' 'ge' 'eq'
        'ne'), compacted in input order (and their indices if with_rows)."""
        _need_cuda(values)
        if values.dtype not in (torch.float32, torch.int64) or values.dim() != 1:
            raise ValueError("selection input must be a 1-D float32 or int64 tensor")
        n = values.numel()
        out = torch.empty(max(n, 1), dtype=values.dtype, device=values.device)
        rows = torch.empty(max(n, 1), dtype=torch.int64, device=values.device) if with_rows else None
        f = lib.hj_dev_select_f32 if values.dtype == torch.float32 else lib.hj_dev_select_i64
        v = float(value) if values.dtype == torch.float32 else int(value)
        check(f(self._ctx, _ptr(values), n, self.CMP[op], v, _ptr(out), _ptr(rows) if with_rows else None, n,
                _ptr(self._count), _stream(self.device, stream)), "hj_dev_select")
        m = int(self._count.item())
        return (out[:m], rows[:m]) if with_rows else out[:m]

    def join(self, rkey, rpay, skey, spay=None, capacity=None, stream=None):
        """The @main join (join_v2.mlir:646-696) on device tensors: build, then
        probe into an output sized optimistically (|S| rows, or `capacity`),
        re-probing once at the exact M if that was too small."""
        self._built(rkey, rpay, skey.numel(), stream)
        dt = torch.int64 if rkey.dtype == torch.int64 else torch.int32
        return self._pair_sized(dt, skey.numel() if capacity is None else int(capacity),
                                lambda o_r, o_s: self.probe_relation(skey, spay, o_r, o_s, stream=stream), "join")

    # ---- key filter (hj.h "Key filter"): opt-in, nothing here turns it on by itself
    FILTERED_JOIN_KINDS = ("inner", "semi", "anti")

    def key_filter(self, n_keys, bits_per_key=16):
        """A KeyFilter for n_keys build keys on this context's device (not yet cleared)."""
        return KeyFilter(n_keys, bits_per_key, device=self.device.index)

    def filtered_join(self, rkey, rpay, skey, spay=None, how="inner", bits_per_key=16, stream=None, **kw):
        """join / semi_join / anti_join behind a key filter built from rkey:
        the S rows whose key fails the filter never reach the build and probe.
        how = 'inner' -> join(R, PASS rows), 'semi' -> semi_join(R, PASS rows),
        'anti' -> the REJECT rows plus anti_join(R, PASS rows); the result
        multisets equal the unfiltered calls'.  int64 keys; spay None is the
        row index.  Takes the underlying method's keyword arguments (capacity,
        with_keys).  last_filtered = (S rows in, S rows kept)."""
        if how not in self.FILTERED_JOIN_KINDS:
            raise ValueError("how must be one of " + ", ".join(self.FILTERED_JOIN_KINDS))
        if rkey.dtype != torch.int64 or skey.dtype != torch.int64 or rkey.dim() != 1 or skey.dim() != 1:
            raise TypeError("filtered_join takes 1-D int64 key columns")
        _need_cuda(rkey, rpay, skey, spay)
        if spay is None:
            spay = torch.arange(skey.numel(), dtype=torch.int64, device=self.device)
        f = self.key_filter(rkey.numel(), bits_per_key)
        try:
            f.clear(stream=stream)
            f.insert(rkey, stream=stream)
            pk, pp = f.apply(skey, spay, "pass", stream=stream)
            self.last_filtered = (skey.numel(), pk.numel())
            if how == "inner":
                return self.join(rkey, rpay, pk, pp, stream=stream, **kw)
            if how == "semi":
                return self.semi_join(rkey, pk, pp, rpay, stream=stream, **kw)
            rk, rp = f.apply(skey, spay, "reject", stream=stream)
        finally:
            f.close()
        with_keys = kw.get("with_keys", False)
        a = self.anti_join(rkey, pk, pp, rpay, stream=stream, **kw)
        if with_keys:
            return torch.cat([rk, a[0]]), torch.cat([rp, a[1]])
        return torch.cat([rp, a])

    # ---- composite keys (hj.h "Composite keys"): up to four key columns, packed exactly into one int64 key
    JOIN_ON_KINDS = ("inner", "semi", "anti", "left", "right", "full")

    def _packed_keys(self, relations, stream=None):
        """(codec, [one packed int64 key column per relation]) for relations
        given as lists of key columns: a codec of the call's own (the caller
        closes it) observes all, seals, packs each, then the plan is read ONCE
        (the one synchronisation): HJError when the joint range needs more than
        64 bits (the packs wrote nothing then) or a row was packed out of range
        -- before the caller builds anything."""
        kc = KeyCodec(tuple(getattr(t, "dtype", None) for t in relations[0]), self.device.index)
        try:
            for cols in relations:
                kc.observe(cols, stream=stream)
            kc.seal(stream=stream)
            keys = [kc.pack(cols, stream=stream) for cols in relations]
            info = kc.info()
            if not info["fits"]:
                raise HJError(f"composite key: the columns' joint range needs {info['bits']} = {info['total_bits']} "
                              f"bits, more than 64 (HJ_ERR_RANGE {HJ_ERR_RANGE})")
            if info["rows_out_of_range"]:
                raise HJError(f"composite key: {info['rows_out_of_range']} rows packed outside the observed range")
        except BaseException:
            kc.close()
            raise
        return kc, keys

    def join_on(self, rcols, rpay, scols, spay=None, how="inner", stream=None, **kw):
        """The join ON r.c0 = s.c0 AND r.c1 = s.c1 ...: rcols / scols are lists
        of 1..4 key columns (1-D contiguous int32 / int64 device tensors, the
        same dtypes on both sides), rpay / spay int64 payload columns (None:
        the row index).  how = 'inner' (join), 'semi' / 'anti' (semi_join /
        anti_join: S rows with / without a partner), 'left' (outer_join: every
        S row), 'right' (full_join how="build": every R row), 'full'
        (full_join); returns what that method returns, and takes its keyword
        arguments (capacity, null, null_r, null_s, with_keys -- the keys of
        with_keys are the packed ones).  Both relations are observed, the plan
        sealed and read once: HJError when the joint range needs more than 64
        bits, before any build."""
        if how not in self.JOIN_ON_KINDS:
            raise ValueError("how must be one of " + ", ".join(self.JOIN_ON_KINDS))
        kc, (rk, sk) = self._packed_keys([rcols, scols], stream=stream)
        kc.close()   # the packed columns stand alone
        if rpay is None:
            rpay = torch.arange(rk.numel(), dtype=torch.int64, device=self.device)
        if spay is None:
            spay = torch.arange(sk.numel(), dtype=torch.int64, device=self.device)
        if how == "inner":
            return self.join(rk, rpay, sk, spay, stream=stream, **kw)
        if how in ("semi", "anti"):
            f = self.semi_join if how == "semi" else self.anti_join
            return f(rk, sk, spay, rpay, stream=stream, **kw)
        if how == "left":
            return self.outer_join(rk, rpay, sk, spay, stream=stream, **kw)
        return self.full_join(rk, rpay, sk, spay, how="build" if how == "right" else "full", stream=stream, **kw)

    def aggregate_on(self, cols, val=None, aggs=("count", "sum"), stream=None):
        """GROUP BY c0, c1, ...: {"keys": [one tensor per column, in the
        columns' dtypes], agg: tensor, ...} with one row per distinct tuple,
        for aggs among "count", "sum", "min", "max" over the int64 column val.
        Packs, calls aggregate, unpacks the key column."""
        kc, (key,) = self._packed_keys([cols], stream=stream)
        try:
            a = self.aggregate(key, val, aggs=aggs, stream=stream)
            out = {"keys": kc.unpack(a.pop("key").contiguous(), stream=stream)}
        finally:
            kc.close()
        out.update(a)
        return out

    def distinct_on(self, cols, stream=None):
        """SELECT DISTINCT c0, c1, ...: the distinct tuples' columns, in no particular order."""
        return self.aggregate_on(cols, aggs=(), stream=stream)["keys"]


# ------------------------------------------------------------------ datagen
@contextlib.contextmanager
def _star_built(dims, group_by, dev, stream, grouped=None):
    """The one-call star functions' setup: a StarProbe and, per dimension (rkey, rpay, skey, how[, null]), a
    HashJoin holding its build under the global strategy; grouped(rkey, rpay, how, null) is called behind the
    build of each dimension marked in group_by.  Yields (star, [(hj, skey, how, null), ...], extras) and behind
    the block closes the star, what the block appended to extras, and the contexts, in that order."""
    hjs, star, extras = [], StarProbe(dev), []
    try:
        probe_dims = []
        for d, g in zip(dims, group_by):
            if len(d) not in (4, 5):
                raise ValueError("a dimension is (rkey, rpay, skey, how[, null])")
            rkey, rpay, skey, how = d[:4]
            if g and how == "anti":
                raise ValueError("an anti dimension has no payload to group by")
            hj = HashJoin(dev)
            hjs.append(hj)
            hj.set_strategy("global")
            hj.build_table(rkey, rpay, stream=stream)
            null = d[4] if len(d) == 5 and d[4] is not None else -1
            probe_dims.append((hj, skey, how, null))
            if g:
                grouped(rkey, rpay, how, null)
        yield star, probe_dims, extras
    finally:
        star.close()   # (waits for the device before the contexts go)
        for x in extras + hjs:
            x.close()


def star_join(dims, device=None, stream=None):
    """A star join in one call: dims = [(rkey, rpay, skey, how[, null]), ...],
    one entry per dimension -- its build columns (rpay None for int32 keys:
    row ids), this dimension's key column of the fact rows, how in "inner" |
    "left" | "anti" and for "left" the payload of a row without a partner
    (default -1).  Builds one HashJoin per dimension under the global strategy,
    probes them with one StarProbe and returns (rows, [payload columns]): the
    qualifying fact rows' positions in input order and per dimension its
    payload column (None for "anti").  Synchronises to read M."""
    if not dims:
        raise ValueError("star_join needs at least one dimension")
    dev = dims[0][2].device.index if device is None else device
    with _star_built(dims, [False] * len(dims), dev, stream) as (star, probe_dims, _):
        return star.probe(probe_dims, stream=stream)


def star_aggregate(dims, val=None, group_by=None, aggs=("count", "sum"), max_groups=None, device=None, stream=None):
    """A star query in one call: dims = [(rkey, rpay, skey, how[, null]), ...]
    as star_join's, val the fact column to aggregate (the key columns' dtype;
    None with aggs of "count" alone), group_by one boolean per dimension: the
    qualifying fact rows are grouped by the payloads of the dimensions marked
    (a "left" dimension's null is a group value; an "anti" dimension has no
    payload and cannot be marked).  Builds the dimensions under the global
    strategy, packs the grouped payload columns' ranges with a KeyCodec, runs
    StarProbe.aggregate and returns {"keys": [per dimension its payload column
    of the groups, None where not grouped], agg: int64 tensor, ...}, one row
    per group in no particular order.  max_groups defaults to the product over
    the grouped dimensions of their build rows (+ 1 for "left"), at most the
    fact rows.  Raises HJError when the grouped ranges do not fit 64 bits
    together (HJ_ERR_RANGE).  Synchronises."""
    if not dims:
        raise ValueError("star_aggregate needs at least one dimension")
    group_by = [False] * len(dims) if group_by is None else [bool(g) for g in group_by]
    if len(group_by) != len(dims):
        raise ValueError("group_by needs one entry per dimension")
    dev = dims[0][2].device.index if device is None else device
    cols, rows = [], []

    def grouped_dim(rkey, rpay, how, null):   # its payload's values: the build's (i32: the row ids) and a LEFT null
        pay = rpay if rkey.dtype == torch.int64 else torch.arange(rkey.numel(), dtype=torch.int32, device=rkey.device)
        if how == "left":
            pay = torch.cat([pay, torch.tensor([null], dtype=pay.dtype, device=pay.device)])
        cols.append(pay.contiguous())
        rows.append(rkey.numel() + (how == "left"))

    with _star_built(dims, group_by, dev, stream, grouped_dim) as (star, probe_dims, extras):
        n = probe_dims[0][1].numel()
        grouped = [i for i, g in enumerate(group_by) if g]
        group = base = None
        if grouped:
            kc = KeyCodec([c.dtype for c in cols], dev)
            extras.append(kc)
            # one observe per column, the others held at a value of their own (an empty one at 0)
            rep = [c[:1] if c.numel() else torch.zeros(1, dtype=c.dtype, device=c.device) for c in cols]
            for i, c in enumerate(cols):
                if c.numel():
                    kc.observe([c if j == i else rep[j].expand(c.numel()).contiguous() for j in range(len(cols))],
                               stream=stream)
            kc.seal(stream=stream)
            plan = kc.info()
            if not plan["fits"]:
                raise HJError(f"star_aggregate failed with {HJ_ERR_RANGE}: the grouped payload ranges need "
                              f"{plan['total_bits']} bits together")
            group, base = [-1] * len(dims), [0] * len(dims)
            for c, i in enumerate(grouped):
                if plan["bits"][c] > 0:
                    group[i] = sum(plan["bits"][c + 1:])
                    base[i] = plan["lo"][c]
        if max_groups is None:
            max_groups = 1
            for r in rows:
                max_groups *= r
            max_groups = min(max_groups, n)
        a = star.aggregate(probe_dims, val, aggs=aggs, group=group, base=base, max_groups=max_groups, stream=stream)
        keys = [None] * len(dims)
        if grouped:
            for i, col in zip(grouped, kc.unpack(a["key"].contiguous(), stream=stream)):
                keys[i] = col
        out = {"keys": keys}
        out.update({k: v for k, v in a.items() if k != "key"})
        torch.cuda.synchronize(dev)
        return out


def star_query(dims, val=None, where=None, expr=None, group_by=None, fact_group_by=None, aggs=("count", "sum"),
               max_groups=None, device=None, stream=None):
    """star_aggregate with the fact row's own part of the query: dims (may be
    empty), val, group_by, aggs and max_groups as star_aggregate's; where and
    expr as StarProbe.query_into's; fact_group_by a list of fact columns to
    group by as well.  One key is laid out over the grouped dimensions' payload
    fields followed by the fact columns' fields -- a fact column's width from
    its observed minimum and maximum, a 0-bit field left out -- and unpacked
    again: returns {"keys": [per dimension its payload column of the groups,
    None where not grouped], "fact_keys": [per fact_group_by column its column
    of the groups, in the column's dtype], agg: int64 tensor, ...}.  Raises
    HJError (HJ_ERR_RANGE) when the fields need more than 64 bits together.
    Synchronises."""
    dims = list(dims)
    group_by = [False] * len(dims) if group_by is None else [bool(g) for g in group_by]
    fcols = [] if fact_group_by is None else list(fact_group_by)
    if len(group_by) != len(dims):
        raise ValueError("group_by needs one entry per dimension")
    if len(fcols) > HJ_STAR_MAX_FACT_GROUPS:
        raise ValueError(f"fact_group_by takes up to {HJ_STAR_MAX_FACT_GROUPS} columns")
    some = [d[2] for d in dims] + [w[0] for w in (where or [])] + fcols + [c for c in (val,) if c is not None]
    if not some:
        raise ValueError("star_query needs a dimension or a fact column")
    dev = some[0].device.index if device is None else device
    n = some[0].numel()
    fields = []   # (lo, hi) of every key field, the grouped dimensions' first

    def grouped_dim(rkey, rpay, how, null):   # its payload's values: the build's (i32: the row ids) and a LEFT null
        vals = []
        if rkey.numel():
            vals = [int(rpay.min()), int(rpay.max())] if rkey.dtype == torch.int64 else [0, rkey.numel() - 1]
        if how == "left":
            vals.append(int(null))
        fields.append((min(vals), max(vals)) if vals else (0, 0))

    with _star_built(dims, group_by, dev, stream, grouped_dim) as (star, probe_dims, _):
        for c in fcols:
            fields.append((int(c.min()), int(c.max())) if c.numel() else (0, 0))
        bits = [(hi - lo).bit_length() for lo, hi in fields]
        if sum(bits) > 64:
            raise HJError(f"star_query failed with {HJ_ERR_RANGE}: the grouped ranges need {sum(bits)} bits together")
        shifts = [sum(bits[i + 1:]) for i in range(len(bits))]
        grouped = [i for i, g in enumerate(group_by) if g]
        group, base = [-1] * len(dims), [0] * len(dims)
        for k, i in enumerate(grouped):
            if bits[k]:
                group[i], base[i] = shifts[k], fields[k][0]
        ng = len(grouped)
        fact_group = [(c, shifts[ng + k], fields[ng + k][0]) for k, c in enumerate(fcols) if bits[ng + k]]
        if max_groups is None:
            max_groups = 1
            for b in bits:
                max_groups <<= b
            max_groups = max(1, min(max_groups, n))
        a = star.query(probe_dims, val, aggs=aggs, where=where, expr=expr, fact_group=fact_group, group=group,
                       base=base, max_groups=max_groups, stream=stream)
        key = a.pop("key")

        def field(k, dtype):   # field k of every group key, back in its column's values
            f = (key >> shifts[k]) & ((1 << bits[k]) - 1) if 0 < bits[k] < 64 else key if bits[k] else torch.zeros_like(key)
            return (f + fields[k][0]).to(dtype)

        keys = [None] * len(dims)
        for k, i in enumerate(grouped):
            keys[i] = field(k, probe_dims[i][1].dtype)
        out = {"keys": keys, "fact_keys": [field(ng + k, c.dtype) for k, c in enumerate(fcols)]}
        out.update(a)
        torch.cuda.synchronize(dev)
        return out


U64_MAX = (1 << 64) - 1


def hit_threshold(frac: float) -> int:
    if frac >= 1.0:
        return U64_MAX
    return min(U64_MAX - 1, int(frac * float(1 << 64)))


def gen_pkfk(seed, NR, NS, frac=1.0, r0=0, nr=None, s0=0, ns=None, device=None, stream=None):
    """Slice [r0, r0+nr) of R and [s0, s0+ns) of S of the PK-FK pair
    (SURVEY 8(d) C1/C3), generated on the device."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    nr = NR if nr is None else nr
    ns = NS if ns is None else ns
    rk = torch.empty(nr, dtype=torch.int64, device=dev); rp = torch.empty_like(rk)
    sk = torch.empty(ns, dtype=torch.int64, device=dev); sp = torch.empty_like(sk)
    check(lib.hj_dev_gen_pkfk_i64(seed, NR, hit_threshold(frac), r0, nr, _ptr(rk), _ptr(rp), s0, ns, _ptr(sk),
                                  _ptr(sp), _stream(dev, stream)), "hj_dev_gen_pkfk_i64")
    return rk, rp, sk, sp


def zipf_params(NR, theta):
    a = (C.c_double * 4)()
    check(lib.hj_zipf_params(int(NR), float(theta), a), "hj_zipf_params")
    return list(a)


def gen_zipf(seed, NR, NS, theta=0.9, s0=0, ns=None, device=None, stream=None):
    """Slice [s0, s0+ns) of a Zipf(theta) probe side over the PK-FK build side
    of the same seed (gen_pkfk's R), generated on the device."""
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    ns = NS if ns is None else ns
    sk = torch.empty(ns, dtype=torch.int64, device=dev); sp = torch.empty_like(sk)
    check(lib.hj_dev_gen_zipf_i64(seed, NR, float(theta), s0, ns, _ptr(sk), _ptr(sp), _stream(dev, stream)),
          "hj_dev_gen_zipf_i64")
    return sk, sp


def gen_uniform_i64(seed, stream_id, lo, hi, n, i0=0, device=None, stream=None):
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    k = torch.empty(n, dtype=torch.int64, device=dev); p = torch.empty_like(k)
    check(lib.hj_dev_gen_uniform_i64(seed, stream_id, lo, hi, i0, n, _ptr(k), _ptr(p), _stream(dev, stream)),
          "hj_dev_gen_uniform_i64")
    return k, p


def gen_uniform_i32(seed, stream_id, lo, hi, n, i0=0, device=None, stream=None):
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    k = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.hj_dev_gen_uniform_i32(seed, stream_id, lo, hi, i0, n, _ptr(k), _stream(dev, stream)),
          "hj_dev_gen_uniform_i32")
    return k


def device_info(device=0):
    """hipDeviceProp facts the roofline quotes (hj_device_info)."""
    a = (C.c_int64 * 8)()
    check(lib.hj_device_info(int(device), a), "hj_device_info")
    keys = ("cus", "memory_clock_khz", "memory_bus_bits", "l2_bytes", "hbm_bytes", "shader_clock_khz",
            "lds_bytes_per_cu", "peak_mb_per_s")
    return dict(zip(keys, [int(x) for x in a]))


COPY_SHAPES = {"persistent": 0, "flat": 1}


def stream_copy(src, dst, shape="persistent", stream=None):
    """Copy 16-B rows src -> dst on the device in one of the two reference
    copy shapes of hj_dev_stream_copy (the bench's copy floor)."""
    _need_cuda(src, dst)
    if src.numel() * src.element_size() != dst.numel() * dst.element_size() or src.numel() * src.element_size() % 16:
        raise ValueError("stream_copy needs equal-sized buffers of whole 16-B rows")
    rows = src.numel() * src.element_size() // 16
    check(lib.hj_dev_stream_copy(_ptr(src), _ptr(dst), rows, COPY_SHAPES[shape], _stream(src.device, stream)),
          "hj_dev_stream_copy")


# Routed-tuple buffers (the EXACT routing pass's destination) are drawn like
# the bucket sets' row buffers in libhj.so (hj_capi.cpp ensure_rows): a
# buffer of >= 1 GiB is probed (hj_placement_check: the partition pass's write
# pattern against a flat write) and redrawn while pattern/flat > 1.12 (the
# library's hj_placement_set_good value), up to 24 draws while free memory is
# >= 3x the buffer, holding at most 2 rejected draws at once (a further reject
# releases the oldest); the best draw is kept.  A buffer that keeps a slow
# draw is a give-up, counted in placement_stats().  HJ_PLACEMENT_PROBE=0
# turns it off.
PLACE_MIN_BYTES = 1 << 30
PLACE_DRAWS = 24
PLACE_HELD = 2
PLACE_SPARE = 3
_py_place = {"probes": 0, "rejected": 0, "gave_up": 0, "gave_up_low_mem": 0, "held_max": 0,
             "last_kept_ratio": 0.0, "worst_kept_ratio": 0.0}


def placed_rows(rows, device):
    """A (rows, 2) int64 device tensor at a placement the partition passes'
    write pattern runs fast in (see PLACE_*).

    The probe writes the candidate on the device's default HIP stream, so the
    caller's streams are drained first (a block torch hands out may still be
    in use by work queued on another stream).  Rejected draws are released to
    the driver with torch.cuda.empty_cache(), which also releases every other
    unused block torch has cached in this process (outside every timed
    region; the allocation is once per exchange buffer)."""
    rows = max(int(rows), 1)
    nbytes = rows * 16
    if nbytes < PLACE_MIN_BYTES or os.environ.get("HJ_PLACEMENT_PROBE", "1") == "0":
        return torch.empty((rows, 2), dtype=torch.int64, device=device)
    good = float(lib.hj_placement_set_good(0.0))
    torch.cuda.synchronize(device)
    held, best, best_r, draws, rejected, held_max, low_mem = [], None, float("inf"), 0, 0, 0, False
    for k in range(PLACE_DRAWS):
        if k > 0 and torch.cuda.mem_get_info(device)[0] < PLACE_SPARE * nbytes:
            low_mem = True
            break
        t = torch.empty((rows, 2), dtype=torch.int64, device=device)
        r = C.c_double(0.0)
        with torch.cuda.device(device):
            check(lib.hj_placement_check(_ptr(t), nbytes, C.byref(r)), "hj_placement_check")
        draws += 1
        if r.value < best_r:
            rej, best, best_r = best, t, r.value
        else:
            rej = t
        if rej is not None:
            rejected += 1
            held.append(rej)
            if len(held) > PLACE_HELD:
                held.pop(0)
            held_max = max(held_max, len(held))
        if best_r <= good:
            break
    _py_place["probes"] += draws
    _py_place["rejected"] += rejected
    if best_r > good:
        _py_place["gave_up"] += 1
        _py_place["gave_up_low_mem"] += int(low_mem)
    _py_place["held_max"] = max(_py_place["held_max"], held_max)
    _py_place["last_kept_ratio"] = round(best_r, 3)
    _py_place["worst_kept_ratio"] = max(_py_place["worst_kept_ratio"], round(best_r, 3))
    if rejected:
        del held, rej
        torch.cuda.empty_cache()   # the rejects go back to the driver, not to torch's cache
    return best


def placement_stats():
    """Row-buffer placement probe counts of this process (hj_placement_stats_ex):
    draws probed / rejected, buffers that kept a slow draw (gave_up; of those,
    gave_up_low_mem: free memory below 3x the buffer stopped the draws), the
    most rejected draws held at once, and the pattern/flat write ratio of the
    last and the worst buffer kept (~1.0 good, 1.25-1.35 a slow placement);
    routed_tuples: the same for the Python-drawn routed-tuple buffers."""
    out = (C.c_longlong * 5)()
    last, worst = C.c_double(0.0), C.c_double(0.0)
    lib.hj_placement_stats_ex(out, C.byref(last), C.byref(worst))
    return {"probes": out[0], "rejected": out[1], "gave_up": out[2], "gave_up_low_mem": out[3],
            "held_max": out[4], "last_kept_ratio": round(last.value, 3), "worst_kept_ratio": round(worst.value, 3),
            "routed_tuples": dict(_py_place)}


def partition_of(key: int, nparts: int) -> int:
    """Owner of a key under the routing hash (host function of libhj.so)."""
    return int(lib.hj_partition_of(int(key), int(nparts)))
