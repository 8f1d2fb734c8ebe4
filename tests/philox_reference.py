"""The device noise stream restated in plain numpy, from the published algorithm and the stream's
contract, for tests that compare the engine's draws element by element.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): a
round maps a four-word counter (c0, c1, c2, c3) under a two-word key (k0, k1) to

    (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))

with hi / lo the halves of the 64-bit product; ten rounds, the key bumped by the Weyl constants
(W0, W1) between rounds.  Pinned by the Random123 known-answer vectors (test_philox_reference_cpu).

The contract of the stream (the comments of device_common.hpp and sample_device.hpp): the key is
(seed lo, seed hi); the counter of rollout g, step k, update u, block blk is (draw lo, draw hi, u,
blk) with draw = g H + k; a block's words (x, y, z, w) give components 4 blk .. 4 blk + 3 by two
Box-Muller pairs, (x, y) then (z, w), cosine first.  A pair (a, b) is u1 = ((a >> 8) + 1) / 2^24 in
(0, 1], u2 = (b >> 8) / 2^24 in [0, 1) revolutions; both are exact in fp32, so the fp64 value
computed here is the exact value the device's fp32 Box-Muller approximates.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57   # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # the key's Weyl increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """uint32[..., 4] from counters [..., 4] and keys [..., 2] (broadcast against each other)."""
    ctr = np.asarray(ctr, dtype=np.uint64) & MASK
    key = np.asarray(key, dtype=np.uint64) & MASK
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape) for i in range(2))
    for _ in range(10):
        p0 = np.uint64(M0) * c0   # 32 x 32 bits: fits 64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(a, b):
    """(u1, u2) of a word pair, fp64 (exact): u1 in (0, 1], u2 in [0, 1)."""
    a = np.asarray(a, dtype=np.uint32).astype(np.float64)
    b = np.asarray(b, dtype=np.uint32).astype(np.float64)
    return (np.floor(a / 256.0) + 1.0) / 16777216.0, np.floor(b / 256.0) / 16777216.0


def box_muller_f64(a, b):
    """(z0, z1) = r (cos, sin)(2 pi u2), r = sqrt(-2 ln u1), in fp64."""
    u1, u2 = uniforms(a, b)
    r = np.sqrt(-2.0 * np.log(u1) + 0.0)   # (+ 0.0: u1 = 1 gives a radius of +0, not sqrt(-0))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def words(seed, update_index, g, k, H, blocks):
    """The stream's words uint32[..., blocks, 4] at rollouts g and steps k (broadcast)."""
    seed = int(seed)
    g, k = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(k, dtype=np.uint64))
    draw = g * np.uint64(H) + k
    ctr = np.zeros(g.shape + (blocks, 4), dtype=np.uint64)
    ctr[..., 0] = (draw & MASK)[..., None]
    ctr[..., 1] = (draw >> S32)[..., None]
    ctr[..., 2] = np.uint64(int(update_index) & 0xFFFFFFFF)
    ctr[..., 3] = np.arange(blocks, dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(ctr, key)


def normals(seed, update_index, g, k, H, C):
    """z[..., C]: the standard normals of rollouts g, steps k (broadcast) of an update, fp64."""
    blocks = (C + 3) // 4
    w = words(seed, update_index, g, k, H, blocks)
    z = np.empty(w.shape[:-2] + (4 * blocks,))
    z[..., 0::4], z[..., 1::4] = box_muller_f64(w[..., 0], w[..., 1])
    z[..., 2::4], z[..., 3::4] = box_muller_f64(w[..., 2], w[..., 3])
    return z[..., :C]


def stable_ranks(prev_costs):
    """rank[r] of every rollout r >= 2 in the stable ascending order of the previous costs, NaN
    last (helpers.replay_device_draws' order); rollouts 0 and 1 have none (-1)."""
    c = np.asarray(prev_costs, dtype=np.float64)[2:]
    order = np.argsort(np.where(np.isnan(c), np.inf, c), kind="stable")
    rank = np.full(c.size + 2, -1, dtype=np.int64)
    rank[2 + order] = np.arange(c.size)
    return rank


def philox_mask(prev_costs, H, keep, shift):
    """bool[R, H]: the (rollout, step) columns of an update that are fresh Philox draws."""
    rank = stable_ranks(prev_costs)
    fresh = np.ones((rank.size, H), dtype=bool)
    fresh[:2] = False
    kept = np.flatnonzero((rank >= 0) & (rank < keep))
    fresh[kept, :max(H - shift, 0) if shift > 0 else H] = False
    return fresh


def expected_noise(prev_costs, prev_noise, prev_optimal, keep, shift, seed, update_index, tdiag):
    """(eps[R, H, C], z[R, H, C], fresh[R, H]) of an update as Trajectory::sample leaves the noise
    (mppi.cpp:189-270) with the device stream: rollout 0 zero; rollout 1 minus the previous U*; the
    `keep` best rollouts of the previous costs carry their previous eps moved `shift` steps up, and
    their last `shift` columns are fresh (shift 0: they keep everything); the rest is fresh.
    Fresh columns are tdiag * z with z the stream's normals at (g, k) under `update_index`; z is
    returned for all columns, fresh or not."""
    prev_noise = np.asarray(prev_noise, dtype=np.float64)
    R, H, C = prev_noise.shape
    tdiag = np.asarray(tdiag, dtype=np.float64)
    z = normals(seed, update_index, np.arange(R)[:, None], np.arange(H)[None, :], H, C)
    eps = tdiag * z
    fresh = philox_mask(prev_costs, H, keep, shift)
    eps[0] = 0.0
    eps[1] = -np.asarray(prev_optimal, dtype=np.float64)
    rank = stable_ranks(prev_costs)
    for r in np.flatnonzero((rank >= 0) & (rank < keep)):
        if shift > 0:
            n = max(H - shift, 0)
            eps[r, :n] = prev_noise[r, shift:shift + n]
        else:
            eps[r] = prev_noise[r]
    return eps, z, fresh


# Seeds whose first update (index 0) holds a Box-Muller edge input at one small FrankaRidgeback
# shape: EDGE_SHAPE = (rollouts S, steps H, keep-best), R = S + 2 rows; found by an offline search
# with words() over seeds 0x9E3779B900000000 + i, i < 16000, among the fresh rollouts (g >= 2 +
# keep-best: the first update's kept rollouts keep their zeros) and the pairs whose components have
# a non-zero variance (0 .. 9).  An entry is kind: (seed, rollout g, step k, component c of the
# pair's cosine draw; the sine draw is c + 1).  The pair's words are (a, b) = words (c % 4, c % 4 + 1)
# of block c // 4.  test_philox_reference_cpu asserts each word is where this table says.
EDGE_SHAPE = (30, 8, 5)
EDGE_SEEDS = {
    "a_min": (0x9E3779B9000018E5, 20, 6, 4),       # a >> 8 == 0: u1 = 2^-24, the largest radius
    "a_max": (0x9E3779B9000010F4, 22, 4, 0),       # a >> 8 == 0xFFFFFF: u1 = 1, radius 0
    "b_zero": (0x9E3779B90000302B, 9, 3, 4),       # b >> 8 == 0: u2 = 0
    "b_quarter": (0x9E3779B900000E7F, 17, 1, 4),   # b >> 8 == 0x400000: u2 = 1/4
}
EDGE_WORDS = {"a_min": ("a", 0), "a_max": ("a", 0xFFFFFF), "b_zero": ("b", 0), "b_quarter": ("b", 0x400000)}
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))   # sqrt(-2 ln 2^-24) = 5.7681...: the stream's largest |z|
