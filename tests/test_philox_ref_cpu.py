"""tests/philox_ref.py checked on its own (no GPU, no product code): the published known-answer vectors of philox4x32-10, the scalar
against the vectorised form, and the properties the device mappings rely on (multiply-shift integers, key domains, normal range)."""
import math

import numpy as np
import pytest

import philox_ref as pr

# Random123 (kat_vectors, philox4x32 10): counter words, key words -> output words
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    assert tuple(pr.philox4x32(ctr, key)) == want
    got = pr.philox4x32(tuple(np.array([c, c], dtype=np.uint64) for c in ctr), key)
    assert [tuple(int(w[i]) for w in got) for i in (0, 1)] == [want, want]
    assert tuple(pr.philox4x32(ctr, key, rounds=9)) != want            # the round count is live


def test_vectorised_equals_scalar():
    seeds = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 0x0123456789ABCDEF)
    offs = (0, 2 ** 32 - 3, 2 ** 40 + 5, 2 ** 64 - 2)
    for seed in seeds:
        for off in offs:
            ctr = pr.counters(off, 6)
            assert [int(c) for c in ctr] == [(off + i) % 2 ** 64 for i in range(6)]            # carry into the high word, 64-bit wrap
            vec = pr.words(seed, ctr)
            for i in range(6):
                assert tuple(int(w[i]) for w in vec) == tuple(pr.words(seed, (off + i) % 2 ** 64))
            np.testing.assert_array_equal(pr.uniform4(seed, ctr)[2], pr.uniform4(seed, int(ctr[2])))
            np.testing.assert_array_equal(pr.normal4(seed, ctr)[5], pr.normal4(seed, int(ctr[5])))
            np.testing.assert_array_equal(pr.randint(seed, ctr, 25), [pr.randint(seed, int(c), 25) for c in ctr])
    # the block's layout: seed halves are the key, counter halves the two low counter words, the two constants the high ones
    assert tuple(pr.words(0x299F31D0A4093822, 0x85A308D3243F6A88)) == tuple(pr.philox4x32((0x243F6A88, 0x85A308D3, pr.C2, pr.C3), (0xA4093822, 0x299F31D0)))
    # every seed / counter bit reaches the words: the high halves are live
    assert tuple(pr.words(1, 5)) != tuple(pr.words(1 + 2 ** 32, 5)) and tuple(pr.words(1, 5)) != tuple(pr.words(1, 5 + 2 ** 32))


def test_randn_stream_layout():
    a = pr.randn(23, 7, 2 ** 32 - 3)
    assert a.shape == (23,) and a.dtype == np.float64
    for i in (0, 3, 4, 13, 22):
        assert a[i] == pr.normal4(7, 2 ** 32 - 3 + (i >> 2))[i & 3]
    np.testing.assert_array_equal(pr.randn(5, 7, 1), pr.randn(9, 7, 0)[4:9])     # offsets count quads
    assert pr.randn(0, 7, 0).shape == (0,)


def _chi2_critical(df, p):
    """upper critical value of chi-square(df) at tail probability p (Wilson-Hilferty; df >= 20: relative error below 1e-3)"""
    from statistics import NormalDist
    z = NormalDist().inv_cdf(1.0 - p)
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


@pytest.mark.parametrize("T", [25, 100])
def test_randint_is_uniform(T):
    """multiply-shift of 32 random bits: the bins of [0, T) differ by at most 1 in 2^32 / T preimages - 10^5 consecutive counters pass a
    chi-square test at the 1e-4 level"""
    n = 100_000
    v = pr.randint(12345 ^ pr.K_TIMESTEP, pr.counters(0, n), T)
    assert v.min() >= 0 and v.max() < T
    cnt = np.bincount(v, minlength=T)
    chi2 = float(((cnt - n / T) ** 2 / (n / T)).sum())
    crit = _chi2_critical(T - 1, 1e-4)
    print(f"T={T}: chi2 = {chi2:.1f}, critical value at 1e-4 = {crit:.1f}")
    assert len(cnt) == T and cnt.min() > 0 and chi2 < crit


def test_key_domains_differ():
    assert pr.K_TIMESTEP == int.from_bytes(b"timestep", "big") and pr.K_NOISE == int.from_bytes(b"trainnoi", "big")
    ctr = pr.counters(0, 4096)
    for seed in (0, 1234, 2 ** 64 - 1):
        w = [np.stack(pr.words(s, ctr)) for s in (seed, seed ^ pr.K_TIMESTEP, seed ^ pr.K_NOISE)]
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert float((w[a] == w[b]).mean()) < 1e-3      # equal counters, different words (chance of a 32-bit match: 2^-32 per word)


def test_normals_are_finite_and_bounded():
    assert abs(pr.NORMAL_MAX - 5.887) < 1e-3
    z = pr.randn(1 << 18, 99, 2 ** 63)
    assert np.isfinite(z).all() and np.abs(z).max() <= pr.NORMAL_MAX
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    # the extreme words: u = 0.5 / 2^24 (largest radius) and u = 1 - 0.5 / 2^24
    assert pr._uniform(0) == 0.5 / 2 ** 24 and pr._uniform(0xFFFFFFFF) == 1.0 - 0.5 / 2 ** 24
    assert math.sqrt(-2.0 * math.log(pr._uniform(0))) == pr.NORMAL_MAX


def test_float32_radius_near_u_equal_one():
    """Why philox_radius (csrc/conv_block.hpp) leaves the logf form for the last 1024 values of k: emulated in float32, (k + 0.5) / 2^24 rounds for
    k >= 2^23 and sqrt(-2 ln u) is then up to 2.4e-4 from the float64 radius (u = 1 at k = 2^24 - 1); the series 2 v + v^2 of -2 ln(1 - v),
    v = (2^24 - k - 0.5) / 2^24, stays within 1e-7, and the logf form below the switch within 3e-6."""
    f = np.float32
    k = np.arange(2 ** 24 - 4096, 2 ** 24, dtype=np.int64)
    exact = np.sqrt(-2.0 * np.log((k + 0.5) / 2.0 ** 24))
    u = (k.astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    naive = np.sqrt(f(-2.0) * np.log(u)).astype(np.float64)
    v = ((2 ** 24 - k).astype(f) - f(0.5)) * f(1.0 / 16777216.0)
    assert (v.astype(np.float64) == (2 ** 24 - k - 0.5) / 2.0 ** 24).all()          # exact in float32
    series = np.sqrt(f(2.0) * v + v * v).astype(np.float64)
    tail = k >= 2 ** 24 - 1024
    assert naive[-1] == 0.0 and 2.3e-4 < np.abs(naive - exact).max() < 2.5e-4
    assert np.abs(series - exact)[tail].max() < 1e-7
    assert np.abs(naive - exact)[~tail].max() < 3e-6
