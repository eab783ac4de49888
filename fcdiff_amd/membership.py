"""
Patient or control?  The host side of UnsharedRegionFit.membership / SharedRegionFit.membership.

For a new subject x_u (C,) and each chain g of a sampler fit, with (f_g, r_g) the chain's end state:
  control side   lc[g, u] = sum_c log N(x_cu; mu_k, sigma_k), k = f_gc: the law of a healthy subject given the template;
  patient side   shared model: lp[g, u] = sum_c log M_{k, l}(x_cu), l the mixture case of the population's (r_gn, r_gm) -- the
                 new patient inherits the population's r, so nothing is annealed;
                 unshared model: lp[g, u] = the annealed-importance-sampling log-weight over the patient's own r_u
                 (score.ais_weights: E exp(lp[g, u]) = p(x_u | f_g)).
Both sides are pooled the same way: log mean_g exp(l[g, u]) over every chain of every rank (score.pool_ais on the sums of
fcd_score_ais_finish), an estimate of p(x_u | data, group) with theta plugged in.  lc and the shared lp come from one kernel
(fcd_member_loglik) that works straight from x and theta: no (C, U', 3, 3) table.  The cohort is walked in chunks of CHUNK
subjects, so apart from a chunk's own buffers nothing on the device grows with it.
"""
import numpy as np

from . import _lib
from .score import ais_weights, chain_parts, pool_ais

CHUNK = 256         # subjects per device pass: (G, CHUNK) outputs per side, and the unshared side's (C, CHUNK, 3, 3) tables


def member_loglik(ctx, x_dev, theta, f_state, r_bits, Nreg, G, r_cols, missing_data, patient=True):
    """(lc, lp) (G, U) float64 device tensors of fcd_member_loglik for x_dev (C, U); lp is None without `patient`."""
    import torch
    U = int(x_dev.shape[1])
    lc = torch.empty((int(G), U), dtype=torch.float64, device=x_dev.device)
    lp = torch.empty((int(G), U), dtype=torch.float64, device=x_dev.device) if patient else None
    (th, _th) = _lib.dbl_array(theta)
    ctx.call("fcd_member_loglik", _lib.dptr(x_dev), th, _lib.dptr(f_state), _lib.dptr(r_bits if patient else None), int(Nreg), U,
             int(G), int(r_cols), _lib.FCD_DATA_NAN_MISSING if missing_data else 0, _lib.dptr(lc), _lib.dptr(lp),
             _lib.stream_ptr())
    return lc, lp


def pool(parts_patient, parts_control):
    """(R, U, 4) sums of each side (fcd_score_ais_finish per rank) -> the result dict of membership()."""
    parts_patient = np.asarray(parts_patient, dtype=np.float64)
    (lp, se_p, ess_p) = pool_ais(parts_patient)
    (lc, se_c, ess_c) = pool_ais(parts_control)
    with np.errstate(invalid="ignore"):
        log_bf = lp - lc
    return {"log_patient": lp, "log_patient_se": se_p, "ess_patient": ess_p, "log_control": lc, "log_control_se": se_c,
            "ess_control": ess_c, "log_bf": log_bf, "log_bf_se": np.sqrt(se_p * se_p + se_c * se_c),
            "n_chains": int(np.sum(parts_patient[..., 3], axis=0)[0])}


def chunks(U, size=None):
    """[(u0, u1), ...] covering range(U) in steps of `size` (default CHUNK, read at call time)."""
    size = CHUNK if size is None else int(size)
    return [(u0, min(U, u0 + size)) for u0 in range(0, int(U), size)]


def membership(ctx, up, x_new, Nreg, sampler, model, missing_data, shared, b_dev=None, pi2=None, n_anneal=None, key=None):
    """
    The chunk loop of membership(): x_new (C, U') NumPy, `up` the fit's host-to-device copy, `sampler` the fit's engine (read
    only).  shared: r is the sampler's one column; else b_dev, pi2, n_anneal and key drive score.ais_weights per chunk.
    """
    theta = model.theta()
    (pp, pc) = ([], [])
    for (u0, u1) in chunks(x_new.shape[1]):
        x_dev = up(x_new[:, u0:u1])
        if shared:
            (lc, lp) = member_loglik(ctx, x_dev, theta, sampler.f_state, sampler.r_bits, Nreg, sampler.G, 1, missing_data)
        else:
            (lc, _none) = member_loglik(ctx, x_dev, theta, sampler.f_state, None, Nreg, sampler.G, 1, missing_data, patient=False)
            lp = ais_weights(ctx, b_dev, x_dev, Nreg, sampler, model, pi2, missing_data, n_anneal, key)[3]
        pp.append(chain_parts(ctx, lp))
        pc.append(chain_parts(ctx, lc))
    ctx.check_device()
    return pool(np.concatenate(pp, axis=1), np.concatenate(pc, axis=1))
