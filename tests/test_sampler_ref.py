"""
CPU tests of tests/sampler_ref.py, the NumPy restatement of the device forward sampler: its Philox is the oracle's,
its draws have the model's law (the checks and tolerances of test_model_sample_gpu_statistics and of the shared
model's test_sample_gpu_statistics), and it is a pure function of the seed.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import sampler_ref as SR
from oracle import fcdiff_oracle as O


def test_philox_known_answers():
    """Random123 kat_vectors for philox4x32-10, as tests/test_oracle_golden.py has them."""
    def one(ctr, key):
        return tuple(int(x) for x in SR.philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]))
    assert one((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert one((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert one((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_philox_is_the_oracles_element_for_element():
    rs = np.random.RandomState(0)
    ctr = rs.randint(0, 2 ** 32, size=(4, 300), dtype=np.uint64)
    ctr[:, :4] = np.array([[0, 0xffffffff, 1, 0x80000000]] * 4, dtype=np.uint64).T
    for key in ((0, 0), (0xffffffff, 0xffffffff), (12345, 7)):
        got = SR.philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1])
        for j in range(ctr.shape[1]):
            assert tuple(int(g[j]) for g in got) == O.philox4x32_10([int(x) for x in ctr[:, j]], key)


@pytest.mark.parametrize("seed", SR.SEEDS + [2 ** 64 - 1])
def test_uniforms_are_the_oracles_site_uniforms(seed):
    idx = np.array([0, 1, 2, 255, 256, 65535, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    for kind in (SR.K_R, SR.K_F, SR.K_T, SR.K_FT):
        got = SR.uniform(seed, idx, kind)
        exp = [O.site_uniform(seed, int(i), 0, 0, kind, 0) for i in idx]
        assert np.array_equal(got, np.array(exp))
    # the high counter word: an index past 2^32 is the counter (lo, hi, 0, kind)
    big = np.array([2 ** 32 + 5, 3 * 2 ** 32 + 1], dtype=np.uint64)
    got = SR.uniform(seed, big, SR.K_T)
    exp = [O.site_uniform(seed, int(i) & 0xFFFFFFFF, int(i) >> 32, 0, SR.K_T, 0) for i in big]
    assert np.array_equal(got, np.array(exp))
    # the normal takes its two uniforms from the two halves of ONE block
    z = SR.normal(seed, idx, SR.K_BT)
    for (j, i) in enumerate(idx):
        u1 = 1.0 - O.site_uniform(seed, int(i), 0, 0, SR.K_BT, 0)
        u2 = O.site_uniform(seed, int(i), 0, 0, SR.K_BT, 1)
        assert z[j] == np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    assert 8.5 < SR.Z_MAX < 8.6


def law_checks(s, theta, N, H, U, shared):
    (pi, eta, eps) = theta[:3]
    (gamma, mu, sigma) = (theta[3:6], theta[6:9], theta[9:12])
    (r, t, fk, ftk, b, bt) = (s["r"], s["t"], s["f"], s["ft"], s["b"], s["bt"])
    C = N * (N - 1) // 2
    assert r.shape == ((N,) if shared else (N, U)) and r.dtype == bool and t.shape == (C, U) and t.dtype == bool
    assert fk.shape == (C,) and ftk.shape == (C, U) and b.shape == (C, H) and bt.shape == (C, U)
    assert set(np.unique(fk)) <= {0, 1, 2} and set(np.unique(ftk)) <= {0, 1, 2}
    assert np.abs(b).max() <= 1 and np.abs(bt).max() <= 1
    nptest.assert_allclose(r.mean(), pi, atol=5 * np.sqrt(0.21 / N) if shared else 0.03)
    nptest.assert_allclose(np.bincount(fk, minlength=3) / C, gamma, atol=0.02 if shared else 0.05)
    ends = O.edge_endpoints(N)
    (rn, rm) = (r[ends[:, 0]], r[ends[:, 1]])
    if shared:
        (rn, rm) = (np.broadcast_to(rn[:, None], t.shape), np.broadcast_to(rm[:, None], t.shape))
    assert t[rn & rm].all() and not t[~rn & ~rm].any()
    nptest.assert_allclose(t[rn ^ rm].mean(), eta, atol=0.02 if shared else 0.03)
    same = ftk == fk[:, None]
    nptest.assert_allclose(same[~t].mean(), 1 - eps, atol=0.02)
    nptest.assert_allclose(same[t].mean(), eps, atol=0.02 if shared else 0.03)
    for k in range(3):
        other = ftk[(fk == k)[:, None] & ~same]
        counts = np.bincount(other, minlength=3)
        assert counts[k] == 0 and abs(counts[(k + 1) % 3] / counts.sum() - 0.5) < 0.05       # the two others equally
        nptest.assert_allclose(b[fk == k].mean(), mu[k], atol=0.02)
        nptest.assert_allclose(b[fk == k].std(), sigma[k], atol=0.02)
        nptest.assert_allclose(bt[ftk == k].mean(), mu[k], atol=0.02)
        nptest.assert_allclose(bt[ftk == k].std(), sigma[k], atol=0.02)


def test_unshared_reference_has_the_models_law():
    (N, H, U) = (40, 6, 50)
    law_checks(SR.sample(SR.THETA_USUAL, N, H, U, 1), SR.THETA_USUAL, N, H, U, False)


def test_shared_reference_has_the_models_law():
    (N, H, U) = (300, 6, 50)
    law_checks(SR.sample(SR.THETA_USUAL, N, H, U, 1, shared=True), SR.THETA_USUAL, N, H, U, True)


@pytest.mark.parametrize("shared", [False, True])
def test_edge_parameters_reach_every_boundary(shared):
    """epsilon = 0, eta = 1, gamma = (1, 0, 0): f is 0 everywhere; a typical connection keeps it; an anomalous one never
    does and takes the two others equally; a discordant pair is always anomalous; b and b~ reach the clip."""
    (N, H, U) = (40, 6, 50)
    s = SR.sample(SR.THETA_EDGE, N, H, U, 1, shared=shared)
    ends = O.edge_endpoints(N)
    (rn, rm) = (s["r"][ends[:, 0]], s["r"][ends[:, 1]])
    if shared:
        (rn, rm) = (rn[:, None], rm[:, None])
    assert not s["f"].any()
    assert np.array_equal(s["t"], np.broadcast_to(rn | rm, s["t"].shape))
    assert not s["ft"][~s["t"]].any() and (s["ft"][s["t"]] > 0).all()
    nptest.assert_allclose((s["ft"][s["t"]] == 1).mean(), 0.5, atol=0.02)
    assert (s["b"] == -1.0).any() and (s["bt"] == -1.0).any() and (s["bt"] == 1.0).any()


@pytest.mark.parametrize("shared", [False, True])
def test_reference_is_a_pure_function_of_the_seed(shared):
    (N, H, U) = (23, 7, 11)
    a = SR.sample(SR.THETA_USUAL, N, H, U, SR.SEEDS[1], shared=shared)
    b = SR.sample(SR.THETA_USUAL, N, H, U, SR.SEEDS[1], shared=shared)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # the low and the high word of the seed both matter
    for other in (SR.SEEDS[1] + 1, SR.SEEDS[1] + (1 << 32)):
        c = SR.sample(SR.THETA_USUAL, N, H, U, other, shared=shared)
        assert not any(np.array_equal(a[k], c[k]) for k in ("t", "ft", "b", "bt"))
    # a smaller U is not a prefix in the unshared model (r is indexed n U + u), but f does not depend on U or H
    d = SR.sample(SR.THETA_USUAL, N, 2, 5, SR.SEEDS[1], shared=shared)
    assert np.array_equal(d["f"], a["f"])
