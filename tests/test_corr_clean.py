"""
The cleaning front-end without a GPU: the long-double oracle of tests/corr_clean_ref.py against two independent
statements of the same quantity (numpy.linalg.lstsq residuals; the partial-correlation identity), its drop rule, the
fp64 restatement of the kernels' pipeline against it on every input of tests/test_gpu_corr_clean.py and
tests/test_gpu_corr_clean_long.py (so that the bound used there, corr_ref.BOUND, is shown to be fair), that those inputs
sit on the seams they are meant for, and the host-side argument checks of fcdiff_amd.corr, which raise before any
context exists.
"""
import numpy as np
import numpy.testing as nptest
import pytest

import corr_clean_ref as CR
import corr_ref as R
from oracle import fcdiff_oracle as O

# what the oracle is held to against fp64 NumPy statements of the same quantity: their error, not its own
NUMPY = dict(rtol=1e-9, atol=1e-11)


def lstsq_corr(ts, cf, mask):
    """corrcoef of the numpy.linalg.lstsq residuals on [1 | confounds], kept frames only: (C, S)."""
    (S, Nreg, T) = ts.shape
    ends = O.edge_endpoints(Nreg)
    out = np.zeros((ends.shape[0], S))
    for s in range(S):
        k = np.ones(T, dtype=bool) if mask is None else mask[s]
        Y = ts[s][:, k].T
        X = np.ones((Y.shape[0], 1)) if cf is None else np.concatenate([np.ones((Y.shape[0], 1)), cf[s][:, k].T], axis=1)
        X = X / np.sqrt((X * X).sum(axis=0))[None, :]
        res = Y - X.dot(np.linalg.lstsq(X, Y, rcond=None)[0])
        out[:, s] = np.corrcoef(res.T)[ends[:, 0], ends[:, 1]]
    return out


@pytest.mark.parametrize("case", [(3, 7, 60, 0, 0.2), (2, 6, 60, 3, 0.0), (3, 9, 90, 17, 0.15), (2, 5, 131, 36, 0.1)])
def test_oracle_against_lstsq(case):
    (S, Nreg, T, Q, drop) = case
    (ts, cf, mask) = CR.make_input(11 + Q, S, Nreg, T, Q, drop=drop, level=5.0)
    (got, info) = CR.corr_clean_ld(ts, cf, mask)
    nptest.assert_allclose(got, lstsq_corr(ts, cf, mask), **NUMPY)
    nk = T if mask is None else mask.sum(axis=1)
    assert np.array_equal(info[:, 0], np.broadcast_to(nk, (S,)))
    assert (info[:, 1] == Q).all() and np.array_equal(info[:, 2], info[:, 0] - 1 - Q)


def test_oracle_against_partial_correlation():
    """rho_ij|X = -P_ij / sqrt(P_ii P_jj), P the inverse covariance of (y_i, y_j, X): no projection anywhere."""
    (S, Nreg, T, Q) = (2, 5, 80, 4)
    (ts, cf, mask) = CR.make_input(5, S, Nreg, T, Q, drop=0.2)
    (got, _info) = CR.corr_clean_ld(ts, cf, mask)
    ends = O.edge_endpoints(Nreg)
    for s in range(S):
        k = mask[s]
        for (c, (n, m)) in enumerate(ends):
            Z = np.concatenate([ts[s][[n, m]][:, k], cf[s][:, k]], axis=0)
            P = np.linalg.inv(np.cov(Z))
            assert abs(got[c, s] - (-P[0, 1] / np.sqrt(P[0, 0] * P[1, 1]))) < 1e-10


def test_dropped_columns_change_nothing_but_rank():
    (S, Nreg, T, Q) = (2, 6, 70, 5)
    (ts, cf, mask) = CR.make_input(8, S, Nreg, T, Q, drop=0.2, level=3.0)
    (base, info0) = CR.corr_clean_ld(ts, cf, mask)
    assert (info0[:, 1] == Q).all()
    dup = np.concatenate([cf, -2.5 * cf[:, 1:2]], axis=1)
    zero = np.concatenate([cf[:, :2], np.zeros((S, 1, T)), cf[:, 2:]], axis=1)
    const = np.concatenate([np.full((S, 1, T), 7.25), cf], axis=1)
    const[:, 0][~mask] = -1.0              # constant over the kept frames only
    comb = np.concatenate([cf, cf[:, 0:1] + 3.0 * cf[:, 3:4]], axis=1)
    for (name, other) in (("duplicate", dup), ("zero", zero), ("constant", const), ("combination", comb)):
        (got, info) = CR.corr_clean_ld(ts, other, mask)
        assert (info[:, 1] == Q).all() and np.array_equal(info[:, 2], info0[:, 2]), name
        nptest.assert_allclose(got, base, err_msg=name, **R.BOUND)
    # which member of a collinear pair comes first does not matter
    (swapped, _i) = CR.corr_clean_ld(ts, dup[:, ::-1], mask)
    nptest.assert_allclose(swapped, base, **R.BOUND)


def test_no_residual_rule():
    (S, Nreg, T, Q) = (4, 5, 40, 3)
    (ts, cf, mask) = CR.make_input(9, S, Nreg, T, Q, drop=0.2)
    ts[0, 1] = 2.0 * cf[0, 0] - 0.5 * cf[0, 2] + 4.0          # in the span (with the intercept)
    ts[0, 2][mask[0]] = 3.0                                    # constant over the kept frames only
    mask[1] = False
    mask[1, :Q + 2] = True                                     # dof 1
    mask[2] = False
    mask[2, :Q + 3] = True                                     # dof 2
    mask[3] = False                                            # nothing kept
    (got, info) = CR.corr_clean_ld(ts, cf, mask)
    ends = O.edge_endpoints(Nreg)
    touched = (ends == 1).any(axis=1) | (ends == 2).any(axis=1)
    assert np.isnan(got[touched, 0]).all() and np.isfinite(got[~touched, 0]).all()
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, 2]).all() and np.isnan(got[:, 3]).all()
    assert info.tolist()[1:] == [[Q + 2, Q, 1], [Q + 3, Q, 2], [0, 0, -1]]


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement of the kernels' pipeline stays inside the bound on the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CR.GPU_INPUTS + CR.GPU_LONG_INPUTS, ids=CR.input_id)
def test_fp64_restatement_within_bound(kw):
    (ts, cf, mask, cleaned) = CR.gpu_case(kw)
    (exp, info) = CR.corr_clean_ld(ts, cf, mask, cleaned=cleaned)
    (got, info64) = CR.corr_fp64(ts, cf, mask)
    assert np.array_equal(info, info64)
    assert np.isfinite(exp).all()
    (_d, excess) = R.worst_excess(got, exp, **R.BOUND)
    assert excess < 1.0, "fp64 restatement at %.3g of the bound" % excess


def test_gpu_inputs_reach_every_resid_instantiation():
    """clean_resid_kernel<QP> has nine instantiations, QP = 8 ceil(Q / 8) for Q = 0 .. 64: each is launched by some input."""
    qs = set(kw["Q"] for kw in CR.GPU_INPUTS + CR.GPU_LONG_INPUTS)
    assert set((Q + 7) // 8 for Q in qs) == set(range(9))


def test_chunk_masks_sit_on_the_seams():
    """n_kept exactly on a block of 256 positions, below it with two blocks of nothing but zero fill behind, and one past it;
    the masks' dropped and kept runs where clean_index_kernel's 256-frame chunks meet."""
    assert len(CR.CHUNK_INPUTS) == 3 and all(kw in CR.GPU_LONG_INPUTS for kw in CR.CHUNK_INPUTS)
    seen = set()
    for kw in CR.CHUNK_INPUTS:
        (S, T) = (kw["S"], kw["T"])
        m = CR.chunk_masks(S, T, kw["Nreg"] + T)
        assert m.shape == (S, T) and m.dtype == bool and np.array_equal(m, CR.make_input(**kw)[2])
        nk = m.sum(axis=1)
        assert nk[:4].tolist() == [200, 256, T - 256, T - 5] and 0 < nk[4] < T
        assert not m[0, :256].any() and not m[1, 256:].any() and not m[2, 256:512].any() and m[2, 255] and m[2, 512]
        assert not m[3, 254:258].any() and m[3, 253] and m[3, 258] and not m[3, 0]
        assert T > 512
        seen.update(nk.tolist())
    assert {200, 256, 257} <= seen


def test_fp64_restatement_residuals():
    (ts, cf, mask) = CR.make_input(77, 2, 9, 90, 17, drop=0.2, level=100.0, scales=True)
    cleaned = CR.clean_ld(ts, cf, mask)
    (resid, info) = CR.clean_fp64(ts, cf, mask)
    assert np.array_equal(info, cleaned["info"])
    nptest.assert_allclose(resid, cleaned["resid"].astype(np.float64), rtol=0, atol=1e-10)
    for s in range(2):
        assert (resid[s, :, info[s, 0]:] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# host-side argument checks: they raise before a context is made (there is no GPU here to make one on)
# ---------------------------------------------------------------------------------------------------------------------
class NoContext(object):
    """Stands where a context would: anything asked of it is an error of the test."""

    def __getattr__(self, name):
        raise AssertionError("the context was used (%s) before the arguments were checked" % name)


BAD_ARGS = [
    (dict(ts=(2, 5), frame_mask=(2, 5)), ValueError),
    (dict(ts=(2, 5, 30), confounds=(2, 30)), ValueError),
    (dict(ts=(2, 5, 30), confounds=(3, 2, 30)), ValueError),
    (dict(ts=(2, 5, 30), confounds=(2, 2, 31)), ValueError),
    (dict(ts=(2, 5, 30), frame_mask=(2, 5, 30)), ValueError),
    (dict(ts=(2, 5, 30), frame_mask=(3, 30)), ValueError),
    (dict(ts=(2, 5, 30), frame_mask=(2, 29)), ValueError),
    (dict(ts=(2, 5, 30), confounds=(2, 65, 30)), NotImplementedError),
]


@pytest.mark.parametrize("shapes,exc", BAD_ARGS)
def test_host_argument_checks(shapes, exc):
    from fcdiff_amd import corr
    args = {k: np.ones(v) for (k, v) in shapes.items()}
    ts = args.pop("ts")
    with pytest.raises(exc):
        corr.correlations(ts, ctx=NoContext(), **args)
    with pytest.raises(exc):
        corr.clean(ts, ctx=NoContext(), **args)


def test_host_argument_checks_accept_torch_shapes():
    import torch
    from fcdiff_amd import corr
    with pytest.raises(ValueError):
        corr.correlations(torch.ones(2, 5, 30), ctx=NoContext(), frame_mask=torch.ones(2, 31, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        corr.clean(torch.ones(2, 5, 30), ctx=NoContext(), confounds=torch.ones(2, 65, 30))
