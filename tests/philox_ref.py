"""Reference generator of the device random streams: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
and the three mappings include/mpdx.h documents - restated here from that contract in plain Python / numpy, importing nothing of the product.

  counter block  (ctr_lo, ctr_hi, 0x243F6A88, 0x85A308D3),  key (seed_lo, seed_hi)
  uniform        u = ((word >> 8) + 0.5) / 2^24                                            (never 0, never above 1)
  normal4        Box-Muller in float64: r0 = sqrt(-2 ln u0), z0 = r0 cos 2 pi u1, z1 = r0 sin 2 pi u1; z2, z3 likewise from u2, u3
  randn          element i of a stream at counter `offset` = component i & 3 of counter offset + (i >> 2)   (64-bit wrap-around)
  randint        (word0 * T) >> 32
  uniform4       the four uniforms of one counter

Every function takes Python ints (scalar form) or uint64 numpy arrays for the counter (vectorised form); both forms give the same words."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key bumps (golden ratio, sqrt(3) - 1)
C2, C3 = 0x243F6A88, 0x85A308D3          # the fixed upper half of the product's counter block (first digits of pi)
K_TIMESTEP = 0x74696D6573746570          # key domain of the training pass's timestep draws: seed ^ K_TIMESTEP
K_NOISE = 0x747261696E6E6F69             # key domain of the training pass's noise draws:    seed ^ K_NOISE
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def philox4x32(counter4, key2, rounds=10):
    """The textbook bijection: four 32-bit counter words, two 32-bit key words -> four 32-bit words.  Python ints in, ints out; if any
    input is a numpy array every word is computed as uint64 arrays (values < 2^32) of the broadcast shape."""
    vec = any(isinstance(v, np.ndarray) for v in (*counter4, *key2))
    if vec:
        k_ = np.uint64
        c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & k_(MASK32) for v in counter4)
        k0, k1 = (np.asarray(v, dtype=np.uint64) & k_(MASK32) for v in key2)
    else:
        k_ = int
        c0, c1, c2, c3 = (int(v) & MASK32 for v in counter4)
        k0, k1 = (int(v) & MASK32 for v in key2)
    m0, m1, w0, w1, mask, s32 = k_(M0), k_(M1), k_(W0), k_(W1), k_(MASK32), k_(32)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bit products (no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return c0, c1, c2, c3


def words(seed, ctr, rounds=10):
    """The product's block: 64-bit seed as the key, 64-bit counter in the lower two counter words."""
    seed = int(seed) & MASK64
    if isinstance(ctr, np.ndarray):
        ctr = ctr.astype(np.uint64)
        lo, hi = ctr & np.uint64(MASK32), ctr >> np.uint64(32)
    else:
        ctr = int(ctr) & MASK64
        lo, hi = ctr & MASK32, ctr >> 32
    return philox4x32((lo, hi, C2, C3), (seed & MASK32, seed >> 32), rounds)


def _uniform(w):
    if isinstance(w, np.ndarray):
        return ((w >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    return ((w >> 8) + 0.5) / 16777216.0


def uniform4(seed, ctr, rounds=10):
    """float64 array [..., 4]"""
    return np.stack([np.asarray(_uniform(w), dtype=np.float64) for w in words(seed, ctr, rounds)], axis=-1)


def normal4(seed, ctr):
    """float64 array [..., 4]"""
    u = uniform4(seed, ctr)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a0, a1 = 2.0 * math.pi * u[..., 1], 2.0 * math.pi * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def counters(offset, n_quads):
    """uint64 counters offset, offset + 1, ... with 64-bit wrap-around"""
    return np.uint64(int(offset) & MASK64) + np.arange(int(n_quads), dtype=np.uint64)


def randn(n, seed, offset=0):
    """float64 [n]: what mpdx_randn(out, n, seed, offset) is documented to write"""
    n = int(n)
    return normal4(seed, counters(offset, (n + 3) // 4)).reshape(-1)[:n]


def randint(seed, ctr, T):
    """uniform integer in [0, T) by multiply-shift of the counter's first word"""
    w0 = words(seed, ctr)[0]
    if isinstance(w0, np.ndarray):
        return ((w0 * np.uint64(T)) >> np.uint64(32)).astype(np.int64)
    return (w0 * int(T)) >> 32


NORMAL_MAX = math.sqrt(-2.0 * math.log(2.0 ** -25))   # |z| of the smallest uniform, 0.5 / 2^24: about 5.887
