"""Host restatement of the sampling contract of ``cmf_draw_batch`` (DESIGN.md "Device-resident split"), numpy only, written from
the contract and not from the kernel's code.

Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library).
  key of a draw   = words 0, 1 of philox(counter = (seed lo, seed hi, draw lo, draw hi), key = (0, 0))
  u32(slot, cloud, i) = word 0 of philox(counter = (slot, cloud, i, 0), key = key of the draw)
Selection for a frame of n points resampled to N (dataset._resample = the reference's sample_points):
  n <  N: 0 .. n-1 in order, then for j = 0 .. N-n-1 the point  (u32(slot, cloud, j) * n) >> 32
  n >= N: point i gets the 64-bit sort key (u32(slot, cloud, i) << 32) | i; the N smallest keys, ascending, are the draw.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four integer arrays (broadcast together), key: two integers -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & LO for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LO, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def draw_key(seed, draw):
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    w = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32, draw & 0xFFFFFFFF, draw >> 32), (0, 0))
    return int(w[0]), int(w[1])


def draw_one(n, N, key, slot, cloud):
    """The N indices of one (slot, cloud) for a frame of n points."""
    n, N = int(n), int(N)
    if n < N:
        u = philox4x32_10((slot, cloud, np.arange(N - n), 0), key)[0]
        return np.concatenate([np.arange(n, dtype=np.int64), ((u * np.uint64(n)) >> S32).astype(np.int64)]).astype(np.int32)
    i = np.arange(n, dtype=np.uint64)
    keys = (philox4x32_10((slot, cloud, i, 0), key)[0] << S32) | i
    return (np.sort(keys)[:N] & LO).astype(np.int32)


def draw_ref(n1, n2, N, seed, draw, slots=None):
    """n1, n2: per-slot point counts of the two clouds -> idx1, idx2 (B, N) int32.  ``slots``: the slot number of each row
    (default 0 .. B-1)."""
    key = draw_key(seed, draw)
    slots = range(len(n1)) if slots is None else slots
    idx1 = np.stack([draw_one(n, N, key, s, 0) for s, n in zip(slots, n1)])
    idx2 = np.stack([draw_one(n, N, key, s, 1) for s, n in zip(slots, n2)])
    return idx1, idx2
