"""Host model of the key filter (hj.h "Key filter"), restated in numpy from the
format's definition, and seeded input makers for the filter tests.

A split-block Bloom filter: nblocks blocks of eight uint32 words; a key owns
one bit in each word of one block.  For a key k (int32 sign-extended first):

    h     = fmix64(uint64(k) ^ 0x9E3779B97F4A7C15)
    block = ((h >> 32) * nblocks) >> 32
    mask[w] = 1 << ((uint32(h) * SALT[w] mod 2^32) >> 27)

Nothing here calls the library."""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
XOR = 0x9E3779B97F4A7C15
SALT = np.array([0x47b6137b, 0x44974d91, 0x8824ad5b, 0xa2b7289d, 0x705495c7, 0x2df1424b, 0x9efc4947, 0x5c6bfb31],
                np.uint32)

# key, nblocks, block, mask[0..7]: the known answers of the format's definition
KNOWN = [
    (5, 1, 0, [0x4000000, 0x400000, 0x800000, 0x200, 0x8000, 0x8, 0x400, 0x20000]),
    (0, 3, 1, [0x4, 0x40000, 0x10, 0x800, 0x2000, 0x200000, 0x4, 0x2]),
    (-1, 4099, 974, [0x1000000, 0x800, 0x1000, 0x80, 0x8000000, 0x2000, 0x10000, 0x400000]),
    (I64_MIN, (1 << 20) + 7, 72715, [0x80000, 0x400, 0x2000000, 0x800, 0x8000000, 0x8000, 0x20000000, 0x1]),
    (I64_MAX, (1 << 31) - 1, 2035610209, [0x100, 0x80, 0x40000000, 0x20, 0x2000, 0x2000, 0x200, 0x2000000]),
    (1234567890123, 1000, 50, [0x4000, 0x40, 0x400, 0x2, 0x4000, 0x200000, 0x4000000, 0x800000]),
]
PLACE_NBLOCKS = [1, 3, 1000, 4099, (1 << 20) + 7, (1 << 31) - 1]


def fmix64(k):
    k = np.asarray(k, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def place(keys, nblocks):
    """(block, mask): block int64 (n,), mask uint32 (n, 8) of int64 / int32 keys."""
    k = np.atleast_1d(np.asarray(keys)).astype(np.int64).view(np.uint64)
    h = fmix64(k ^ np.uint64(XOR))
    block = ((h >> np.uint64(32)) * np.uint64(nblocks)) >> np.uint64(32)
    lo = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(over="ignore"):
        sh = (lo[:, None] * SALT[None, :]) >> np.uint32(27)
    return block.astype(np.int64), (np.uint32(1) << sh).astype(np.uint32)


def build(keys, nblocks, dense=None):
    """The filter's words, uint32 (nblocks, 8), after inserting keys into a cleared
    filter.  dense: which of the two equivalent ways to OR the bits in (default: by size)."""
    block, mask = place(keys, nblocks)
    word = (block[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
    if len(block) * 8 > nblocks * 16 if dense is None else dense:
        # many keys per block: one bool per filter bit, then packed (bit b of a word is bit b of its value)
        bits = np.zeros(nblocks * 256, bool)
        bits[word * 32 + np.log2(mask.reshape(-1)).astype(np.int64)] = True
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(nblocks, 8)
    words = np.zeros((nblocks, 8), np.uint32)
    if len(block):
        np.bitwise_or.at(words.reshape(-1), word, mask.reshape(-1))
    return words


def test(words, keys):
    """bool (n,): which keys pass."""
    block, mask = place(keys, len(words))
    return ((words[block] & mask) == mask).all(axis=1)


test.__test__ = False   # (a model function, not a test)


def blocks_for(n_keys, bits_per_key):
    return max(1, -(-n_keys * bits_per_key // 256))


def as_i64(words):
    """The words as the int64 elements of KeyFilter.words (nblocks * 4)."""
    return np.ascontiguousarray(words).reshape(-1).view(np.int64)


# ------------------------------------------------------------------ inputs
def keys(seed, n, lo=I64_MIN, hi=I64_MAX):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.int64, endpoint=True)


def disjoint(seed, n_in, n_out):
    """(inserted, absent): random int64 keys, no key in both, none repeated."""
    rng = np.random.default_rng(seed)
    u = np.unique(rng.integers(I64_MIN, I64_MAX, n_in + n_out + 64, dtype=np.int64, endpoint=True))
    assert len(u) >= n_in + n_out
    u = rng.permutation(u)
    return u[:n_in], u[n_in:n_in + n_out]


def relation(seed, n, pool, hit=0.5):
    """n probe keys: about `hit` of them drawn from pool (a build side's keys), the rest random."""
    rng = np.random.default_rng(seed)
    k = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    if len(pool) and n:
        m = rng.random(n) < hit
        k[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
    return k
