"""The numpy restatement of the device noise stream (philox_reference.py) pinned by itself: the
published known-answer vectors, the key's two halves, the Box-Muller edges, the layout of an
update's noise, and the committed edge seeds the GPU test (test_gpu_philox_stream.py) relies on."""
import numpy as np
import pytest

import philox_reference as P

# Random123's kat_vectors for philox4x32-10: counter, key, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in P.philox4x32_10(ctr, key)) == want
    # vectorised: the three at once, and broadcast of one key over several counters
    got = P.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert got.dtype == np.uint32 and got.tolist() == [list(k[2]) for k in KAT]
    got = P.philox4x32_10(np.array([KAT[0][0], KAT[0][0]]), np.array(KAT[0][1]))
    assert got.tolist() == [list(KAT[0][2])] * 2


def test_counter_and_key_layout():
    """words(): the counter is (draw lo, draw hi, update, block), the key (seed lo, seed hi)."""
    H, seed = 8, 0x0123456789ABCDEF
    w = P.words(seed, 3, 5, 2, H, 3)
    for blk in range(3):
        want = P.philox4x32_10((5 * H + 2, 0, 3, blk), (0x89ABCDEF, 0x01234567))
        assert np.array_equal(w[blk], want)
    # a draw index past 32 bits lands in counter word 1 (no handle of test size reaches it)
    g = (1 << 33) // H + 7
    w = P.words(seed, 3, g, 1, H, 1)
    d = g * H + 1
    assert np.array_equal(w[0], P.philox4x32_10((d & 0xFFFFFFFF, d >> 32, 3, 0), (0x89ABCDEF, 0x01234567)))
    # the update index is taken modulo 2^32
    assert np.array_equal(P.words(seed, (1 << 32) + 3, 5, 2, H, 3), P.words(seed, 3, 5, 2, H, 3))


def test_every_seed_bit_keys_the_stream():
    """The high word of the seed is key word 1: clearing it, or swapping the halves, gives another
    stream, in nearly every draw."""
    seed = 0x9E3779B97F4A7C15
    low_only = seed & 0xFFFFFFFF
    swapped = ((seed & 0xFFFFFFFF) << 32) | (seed >> 32)
    g, k = np.arange(2, 34)[:, None], np.arange(8)[None, :]
    z = P.normals(seed, 0, g, k, 8, 12)
    for other in (low_only, swapped):
        zo = P.normals(other, 0, g, k, 8, 12)
        assert np.mean(np.abs(z - zo) > 1e-3) > 0.99
    # and the update index, the step, the rollout and the block each change it
    assert np.mean(np.abs(z - P.normals(seed, 1, g, k, 8, 12)) > 1e-3) > 0.99
    assert np.mean(np.abs(z[:, 1:] - z[:, :-1]) > 1e-3) > 0.99
    assert np.mean(np.abs(z[1:] - z[:-1]) > 1e-3) > 0.99
    assert np.mean(np.abs(z[..., 4:8] - z[..., 0:4]) > 1e-3) > 0.99


def test_box_muller_values_and_edges():
    top = np.uint32(0xFFFFFF00)
    z0, z1 = P.box_muller_f64(np.uint32(0), np.uint32(0))          # u1 = 2^-24, u2 = 0
    assert z0 == pytest.approx(P.R_MAX, abs=1e-15) and z1 == 0.0
    assert P.R_MAX == pytest.approx(5.768107546403532, abs=1e-15)
    z0, z1 = P.box_muller_f64(np.uint32(0xFF), np.uint32(0x400000FF))   # the low 8 bits are dropped
    assert abs(z0) < 1e-15 and z1 == pytest.approx(P.R_MAX, abs=1e-15)
    z0, z1 = P.box_muller_f64(top, np.uint32(0x12345678))           # u1 = 1: radius +0
    assert z0 == 0.0 and z1 == 0.0 and not np.signbit(z1)
    u1, u2 = P.uniforms(np.array([0, 0xFFFFFFFF], dtype=np.uint32), np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u1.tolist() == [2.0 ** -24, 1.0] and u2.tolist() == [0.0, 1.0 - 2.0 ** -24]
    # a generic pair against the formula written out
    a, b = 0x80000000, 0x20000000   # u1 = 1/2 + 2^-24, u2 = 1/8
    z0, z1 = P.box_muller_f64(np.uint32(a), np.uint32(b))
    r = np.sqrt(-2.0 * np.log(0.5 + 2.0 ** -24))
    assert z0 == pytest.approx(r * np.sqrt(0.5), rel=1e-15) and z1 == pytest.approx(r * np.sqrt(0.5), rel=1e-15)


def test_normals_word_to_component_mapping_and_moments():
    H, C, seed = 8, 12, 0x5EED
    g, k = np.arange(2, 2050)[:, None], np.arange(H)[None, :]
    z = P.normals(seed, 0, g, k, H, C)
    w = P.words(seed, 0, g, k, H, 3)
    for blk in range(3):
        c0, s0 = P.box_muller_f64(w[..., blk, 0], w[..., blk, 1])
        c1, s1 = P.box_muller_f64(w[..., blk, 2], w[..., blk, 3])
        for j, v in enumerate((c0, s0, c1, s1)):
            assert np.array_equal(z[..., 4 * blk + j], v)
    assert np.all(np.isfinite(z))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert np.max(np.abs(np.corrcoef(z.reshape(-1, C).T) - np.eye(C))) < 0.03
    # C = 3 (the point mass): block 0 alone, its first three components
    assert np.array_equal(P.normals(seed, 0, g, k, H, 3), z[..., :3])


def test_expected_noise_layout():
    """expected_noise against the rules written out per rollout, with NaN and tied costs."""
    S, H, C, K = 14, 6, 12, 4
    R = S + 2
    rng = np.random.default_rng(1)
    prev_costs = rng.uniform(1.0, 2.0, R)
    prev_costs[5] = np.nan
    prev_costs[9] = prev_costs[3] = 0.5   # a tie for the best: rollout 3 ranks before 9
    prev_costs[12] = 0.75
    prev_costs[7] = 0.8
    prev_noise = rng.standard_normal((R, H, C))
    U = rng.standard_normal((H, C))
    td = np.sqrt(np.array([0.1, 0.1, 0.2] + [7.5] * 7 + [0.0, 0.0]))
    rank = P.stable_ranks(prev_costs)
    assert rank[0] == rank[1] == -1 and rank[3] == 0 and rank[9] == 1 and rank[12] == 2 and rank[7] == 3
    assert rank[5] == S - 1 and sorted(rank[2:]) == list(range(S))
    for shift in (0, 2, H, H + 3):
        eps, z, fresh = P.expected_noise(prev_costs, prev_noise, U, K, shift, 0xABCDEF0123456789, 7, td)
        assert np.array_equal(z, P.normals(0xABCDEF0123456789, 7, np.arange(R)[:, None], np.arange(H)[None, :], H, C))
        assert np.all(eps[0] == 0.0) and np.array_equal(eps[1], -U)
        kept = H if shift == 0 else max(H - shift, 0)
        for r in range(2, R):
            n = kept if r in (3, 9, 12, 7) else 0
            assert np.array_equal(eps[r, :n], prev_noise[r, (shift if shift > 0 else 0):][:n])
            assert np.array_equal(eps[r, n:], td * z[r, n:])
            assert fresh[r].tolist() == [False] * n + [True] * (H - n)
        assert not fresh[:2].any() and np.all(eps[fresh][:, 10:] == 0.0)   # no variance: no noise
    # nothing kept: everything past rollout 1 is fresh whatever the shift
    eps, z, fresh = P.expected_noise(prev_costs, prev_noise, U, 0, 2, 1, 0, td)
    assert fresh[2:].all() and np.array_equal(eps[2:], td * z[2:])


@pytest.mark.parametrize("kind", sorted(P.EDGE_SEEDS))
def test_edge_seeds_hold_their_words(kind):
    """The committed edge seeds: the stated word at the stated (g, k, component), in a fresh
    rollout of the first update and a component with variance, and what the reference makes of it."""
    S, H, K = P.EDGE_SHAPE
    assert S <= 32 and H <= 8
    seed, g, k, c = P.EDGE_SEEDS[kind]
    which, value = P.EDGE_WORDS[kind]
    assert seed >> 32 != 0 and 2 + K <= g < S + 2 and 0 <= k < H and c % 2 == 0 and c + 1 < 10
    w = P.words(seed, 0, g, k, H, 3)[c // 4]
    a, b = int(w[c % 4]), int(w[c % 4 + 1])
    assert ({"a": a, "b": b}[which] >> 8) == value
    prev = np.zeros(S + 2)
    assert P.philox_mask(prev, H, K, 0)[g, k]   # fresh in the first update (costs all equal: index order)
    z = P.normals(seed, 0, g, k, H, 12)
    u1, u2 = P.uniforms(np.uint32(a), np.uint32(b))
    if kind == "a_min":
        assert u1 == 2.0 ** -24 and np.hypot(z[c], z[c + 1]) == pytest.approx(P.R_MAX, abs=1e-14)
    elif kind == "a_max":
        assert u1 == 1.0 and z[c] == 0.0 and z[c + 1] == 0.0
    elif kind == "b_zero":
        assert u2 == 0.0 and z[c] == np.sqrt(-2.0 * np.log(u1)) and z[c + 1] == 0.0
    else:
        assert u2 == 0.25 and abs(z[c]) < 1e-15 and z[c + 1] == pytest.approx(np.sqrt(-2.0 * np.log(u1)), rel=1e-15)
