"""Expectations of the expand probe tests (hj_dev_expand_*): pure numpy, never
the library.  R is stable-sorted by key, searchsorted left / right gives every
probe row's run of partners; the offsets are the exclusive scan of the segment
widths.  Offsets are compared exactly; the values after sorting WITHIN
segments on both sides (lexsort by (segment id, value)), and unsorted as well
when the build side repeats no key."""
import numpy as np

KINDS = ("inner", "outer")


class ExpandExpect:
    def __init__(self, rk, rp, sk, how, null):
        rp = np.asarray(rp, np.int64)
        o = np.argsort(rk, kind="stable")
        rs = rk[o]
        lo, hi = np.searchsorted(rs, sk, "left"), np.searchsorted(rs, sk, "right")
        self.cnt = (hi - lo).astype(np.int64)
        self.w = np.maximum(self.cnt, 1) if how == "outer" else self.cnt
        self.off = np.concatenate([[0], np.cumsum(self.w)]).astype(np.int64)
        self.m = int(self.off[-1])
        self.seg = np.repeat(np.arange(len(sk), dtype=np.int64), self.w)
        k = np.arange(self.m, dtype=np.int64) - self.off[self.seg]      # place inside the segment
        if len(rk):
            at = np.minimum(np.repeat(lo, self.w) + k, len(rk) - 1)
            self.r = np.where(np.repeat(self.cnt, self.w) > 0, rp[o][at], null).astype(np.int64)
        else:
            self.r = np.full(self.m, null, np.int64)
        self.unique = len(np.unique(rk)) == len(rk)

    def sorted_within(self, vals, upto=None):
        """vals[:upto] ordered by (segment, value)."""
        upto = self.m if upto is None else upto
        v, s = np.asarray(vals[:upto], np.int64), self.seg[:upto]
        return v[np.lexsort((v, s))]

    def same_values(self, got, upto=None):
        """Do the first `upto` values equal the expected ones segment by segment?
        A segment cut by `upto` holds SOME of its partners there: every value
        must be one of the segment's, none twice."""
        upto = self.m if upto is None else min(upto, self.m)
        got = np.asarray(got[:upto], np.int64)
        if self.unique and not np.array_equal(got, self.r[:upto]):
            return False
        if upto == 0:
            return True
        last = int(self.seg[upto - 1])
        whole = int(self.off[last]) if self.off[last + 1] > upto else upto   # the end of the last complete segment
        if not np.array_equal(self.sorted_within(got, whole), self.sorted_within(self.r, whole)):
            return False
        part = np.sort(got[whole:upto])
        full = np.sort(self.r[whole:int(self.off[last + 1])])
        if len(part) != len(np.unique(part)) and len(full) == len(np.unique(full)):
            return False
        # (multiset inclusion: each value at most as often as the segment holds it)
        uv, uc = np.unique(part, return_counts=True)
        fv, fc = np.unique(full, return_counts=True)
        pos = np.searchsorted(fv, uv)
        return bool(len(uv) == 0 or ((pos < len(fv)).all() and (fv[np.minimum(pos, len(fv) - 1)] == uv).all()
                                     and (uc <= fc[np.minimum(pos, len(fv) - 1)]).all()))
