"""The Gaussian noise of a DP-FedAvg round restated in numpy, float64, for the
noise tests and tools/bench_noise.py: Philox4x32-10 (Salmon et al. 2011) keyed by the seed, counted
by (absolute column // 4, sequence), 23-bit uniforms that are never 0 or 1, Box-Muller on two pairs
per counter, and the fp32 add.  Also the launch grid (plan_gauss_add of
flearn_amd/csrc/fa_geometry.hpp, checked against the C++ by tests/test_noise_host.py).  No torch, no
flearn_amd."""
import math
from collections import namedtuple

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the round's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the key's increments
MASK = 0xFFFFFFFF
ROUNDS = 10
Z_MAX = math.sqrt(48.0 * math.log(2.0))  # u_a = 2^-24: sqrt(-2 ln 2^-24) = 5.768...

# |z_gpu - z_ref| <= Z_ERROR: twice the largest difference measured on MI355X over the 2^20 columns of
# SAMPLE below (6.31e-7 at z = -4.21, profiles/noise/bench_noise.json "z_error"), rounded up to one
# significant digit; the issue caps it at 1e-5.  (fl32 of the reference itself is 2.3e-7 away.)
Z_ERROR = 2e-6
SAMPLE = dict(seed=0x0123456789ABCDEF, sequence=1, n=1 << 20)

BLOCK = 256  # gauss_add_kernel's lanes per block, one quad per lane and step
BLOCKS_PER_CU = 8

Plan = namedtuple("Plan", "quads blocks grid steps")


def philox4x32(counter, key, rounds=ROUNDS):
    """The four output words (uint64 arrays holding 32-bit values) for counter = (c0, c1, c2, c3),
    each an integer or an array, and key = (k0, k1), two integers."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in counter)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    lo, sh = np.uint64(MASK), np.uint64(32)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 bits: exact in 64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & lo
    return c0, c1, c2, c3


def words(seed, sequence, q):
    """uint64 [len(q), 4]: the words of the counters q (absolute column // 4) of one noised round."""
    q = np.asarray(q, dtype=np.uint64)
    seed, sequence = int(seed) & (2**64 - 1), int(sequence) & (2**64 - 1)
    out = philox4x32((q & np.uint64(MASK), q >> np.uint64(32), sequence & MASK, sequence >> 32), (seed & MASK, seed >> 32))
    return np.stack(out, axis=-1)


def uniform(word):
    """((word >> 9) + 0.5) * 2^-23, in [2^-24, 1 - 2^-24]: exact in fp32 and float64."""
    return ((np.asarray(word, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(seed, sequence, col_begin, n_cols):
    """float64 [n_cols]: the standard normals of the absolute columns col_begin .. col_begin + n_cols - 1."""
    col_begin, n_cols = int(col_begin), int(n_cols)
    q0, q1 = col_begin // 4, (col_begin + n_cols + 3) // 4
    u = uniform(words(seed, sequence, np.uint64(q0) + np.arange(q1 - q0, dtype=np.uint64)))  # [quads, 4]
    z = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):  # words a, a + 1 -> columns 4q + a, 4q + a + 1
        r = np.sqrt(-2.0 * np.log(u[:, a]))
        z[:, a] = r * np.cos(2.0 * np.pi * u[:, a + 1])
        z[:, a + 1] = r * np.sin(2.0 * np.pi * u[:, a + 1])
    off = col_begin - 4 * q0
    return z.reshape(-1)[off : off + n_cols]


def add(acc, sigma, z):
    """fl32(acc + fl32(sigma * z)) for fp32 acc, an fp32 sigma and z already rounded to fp32."""
    return (np.asarray(acc, np.float32) + (np.float32(sigma) * np.asarray(z, np.float32)).astype(np.float32)).astype(np.float32)


def ceil_div(a, b):
    return -(-a // b)


def plan(n_cols, cus, forced=0):
    """plan_gauss_add: quads of the window, 256-lane blocks that cover them once, the grid (the forced
    one, else at most 8 blocks per CU) and the grid-stride steps of the busiest lane."""
    quads = ceil_div(max(n_cols, 0), 4)
    blocks = max(1, ceil_div(quads, BLOCK))
    cap = forced if forced > 0 else cus * BLOCKS_PER_CU
    grid = max(1, min(blocks, cap))
    return Plan(quads, blocks, grid, ceil_div(blocks, grid))
