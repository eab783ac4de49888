"""
Scoring new patients against a fitted model (UnsharedRegionFit.score): the host side.

Given the template F and theta, patients are independent in the IAR model (doc/methods.rst, the generative model), so a
patient who was not in the fit is scored with the fit held fixed:
  vb     q_F and theta fixed; the new patients' q_R iterated to its fixed point (fcd_vb_update_qR), then the per-patient
         lower bound elbo[u] <= E_{q_F} log p(bt_u | F) (fcd_vb_patient_elbo).
  gibbs  each chain's template draw f_g fixed (the end state of the fit's sampler); annealed importance sampling over r
         from the prior to p(r | f_g, bt) (fcd_score_ais_step between r passes on the tempered table) gives
         log_pred[u] = log mean_g p(bt_u | f_g); r-only sweeps at beta = 1 then sample p(r | f_g, bt) and feed the tallies
         behind p_R, the count law and the connection posteriors.
Every device step is a kernel of libfcdiff_hip.so; what is here is orchestration and the few host formulas on per-patient
numbers (the AIS schedule, the pooling of the AIS sums over ranks) that the CPU tests check directly.
"""
import numpy as np

from . import _lib
from . import tables
from . import util
from .gibbs import GibbsEngine, allreduce_counts, pool_u32, PAIR_COUNT_MAX

# Random numbers of the scoring sampler.  Its Philox counter is (site, chain id, sweep, kind) like the fit's, and its sites
# reuse the training patients' site indices, so with the fit's key and sweep numbers the r draws would reuse the uniforms
# that made f_g.  Both are kept apart: the key is score_key(seed) (a 64-bit mix, never the seed itself in practice), and the
# sweeps are numbered from SCORE_SWEEP0 = 2^31 on, past any fit of fewer than 2^31 sweeps -- so even a key that happened to
# equal the fit's would not reuse the fit's r-pass uniforms.  (The prior draw of r at beta = 0 is fcd_gibbs_init's sweep 0:
# kept apart by the key.)
SCORE_SWEEP0 = 1 << 31
_MASK64 = (1 << 64) - 1


def score_key(seed):
    """Philox key of the scoring sampler for a seed: the splitmix64 output function of seed + 0x9E3779B97F4A7C15."""
    z = (int(seed) + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def ais_schedule(n_anneal, beta_lin=1e-3, frac_lin=0.2):
    """
    0 = beta_0 < beta_1 < ... < beta_T = 1 (T = n_anneal >= 1): the first max(1, round(frac_lin T)) steps linear from 0 to
    beta_lin, the rest geometric from beta_lin to 1 (T = 1: the one step 0 -> 1).  beta_T is exactly 1.0, so the last
    tempered table is the beta = 1 table bit for bit.
    """
    T = int(n_anneal)
    if T < 1:
        raise ValueError("n_anneal must be >= 1")
    if T == 1:
        return np.array([0.0, 1.0])
    n_lin = min(max(1, int(round(frac_lin * T))), T - 1)
    lin = beta_lin * np.arange(0, n_lin + 1) / n_lin
    n_geo = T - n_lin
    geo = beta_lin ** (1.0 - np.arange(1, n_geo + 1) / n_geo)
    out = np.concatenate([lin, geo])
    out[-1] = 1.0
    return out


def pool_ais(parts):
    """
    parts (R, U, 4): per rank and patient {m = max_g w, s1 = sum_g exp(w - m), s2 = sum_g exp(2 (w - m)), n chains}
    (fcd_score_ais_finish) -> (log_pred, log_pred_se, ess), each (U,):
        log_pred = log( sum_all exp(w) / n_all )               (logsumexp over every rank's chains - log G)
        ess      = (sum exp w)^2 / sum exp(2 w)
        se       = sqrt((n S2 / S1^2 - 1) / (n - 1))            (delta method: se of the mean weight over the mean)
    A patient with every weight zero (m = -inf on every rank) gets log_pred = -inf, ess = 0 and se = nan.
    """
    parts = np.asarray(parts, dtype=np.float64)
    if parts.ndim == 2:
        parts = parts[None]
    (mx, s1, s2, n) = (parts[..., 0], parts[..., 1], parts[..., 2], parts[..., 3])
    M = np.max(mx, axis=0)
    dead = ~np.isfinite(M) & (M < 0)
    Ms = np.where(dead, 0.0, M)
    with np.errstate(invalid="ignore", over="ignore"):
        scale = np.where(np.isneginf(mx), 0.0, np.exp(mx - Ms[None, :]))
        S1 = np.sum(s1 * scale, axis=0)
        S2 = np.sum(s2 * scale * scale, axis=0)
    nn = np.sum(n, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_pred = np.where(dead, -np.inf, Ms + np.log(S1) - np.log(nn))
        ess = np.where(dead, 0.0, S1 * S1 / S2)
        v = np.maximum(nn * S2 / (S1 * S1) - 1.0, 0.0)
        se = np.where(dead | (nn < 2), np.nan, np.sqrt(v / np.maximum(nn - 1.0, 1.0)))
    return log_pred, se, ess


def _world():
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def gather_rows(t):
    """(R, ...) NumPy stack of every rank's copy of t (one rank: t alone)."""
    import torch
    import torch.distributed as dist
    if _world() == 1:
        return t.cpu().numpy()[None]
    x = t if dist.get_backend() == "nccl" else t.cpu()
    lst = [torch.zeros_like(x) for _ in range(dist.get_world_size())]
    dist.all_gather(lst, x)
    return np.stack([y.cpu().numpy() for y in lst])


def lik_tables(ctx, b_dev, bt_dev, theta, missing_data, noise=None):
    """(S_B (C, 3), lM (C, U', 3, 3)) of new patients bt_dev (C, U') or (C, U', K') into fresh tensors (the table kernel needs
    H >= 1: b is the fit's).  noise: tables.build's (the controls' variances of the fit, the new patients' own), or None."""
    kw = {} if noise is None else {"noise": noise}
    return tables.build(ctx, b_dev, bt_dev, theta, _lib.FCD_DATA_NAN_MISSING if missing_data else 0, **kw)


def hyper_block(ctx, gamma, pi2, device):
    import torch
    return tables.write_hyper(ctx, torch.zeros(8, dtype=torch.float64, device=device), gamma, pi2)


def chain_parts(ctx, w):
    """(R, U, 4) NumPy: fcd_score_ais_finish of this rank's log-weights w (G, U), stacked over ranks (for pool_ais)."""
    import torch
    (G, U) = (int(w.shape[0]), int(w.shape[1]))
    fin = torch.empty((U, 4), dtype=torch.float64, device=w.device)
    ctx.call("fcd_score_ais_finish", _lib.dptr(w), U, G, _lib.dptr(fin), _lib.stream_ptr())
    return gather_rows(fin)


def patient_elbo(ctx, lq_F, lq_R, lM, hyper, Nreg, U):
    """(U, 4) NumPy {E_lM, E_lp_R, E_lq_R, elbo} per patient through fcd_vb_patient_elbo."""
    import torch
    C = util.N_to_C(int(Nreg))
    if (tuple(lq_F.shape) != (C, 1, 3) or tuple(lq_R.shape) != (Nreg, U, 2) or tuple(lM.shape) != (C, U, 3, 3)):
        raise ValueError("lq_F (C, 1, 3), lq_R (Nreg, U, 2) and lM (C, U, 3, 3) disagree")
    out = torch.empty((U, 4), dtype=torch.float64, device=lM.device)
    ctx.call("fcd_vb_patient_elbo", _lib.dptr(lq_F.contiguous()), _lib.dptr(lq_R.contiguous()), _lib.dptr(lM.contiguous()),
             _lib.dptr(hyper), int(Nreg), int(U), _lib.dptr(out), _lib.stream_ptr())
    return out.cpu().numpy()


def score_vb(ctx, b_dev, bt_dev, Nreg, lq_F, model, pi2, edge_mode, missing_data, connections, max_iters, tol, noise=None):
    """The variational path of UnsharedRegionFit.score (see there); lq_F is the fit's, read only."""
    import torch
    from .fit import count_posterior, conn_posterior
    U = int(bt_dev.shape[1])
    theta = model.theta()
    (_S_B, lM) = lik_tables(ctx, b_dev, bt_dev, theta, missing_data, noise)
    hyper = hyper_block(ctx, model.gamma, pi2, bt_dev.device)
    lq_R = torch.full((Nreg, U, 2), -np.log(2), dtype=torch.float64, device=bt_dev.device)      # uniform, as _init_lps
    # Each patient stops on its own: its q_R is taken at the first iteration where its own max_n |delta q| < tol.  The update
    # treats patients independently (one workgroup each), so a patient's trajectory -- and with this rule its result -- does
    # not depend on the other patients of the call.  The others keep iterating until all have stopped or max_iters.
    final = np.full((Nreg, U, 2), -np.log(2))
    q_prev = np.full((Nreg, U), 0.5)
    iters = np.zeros(U, dtype=np.int64)             # 0 while a patient is still iterating
    converged = np.zeros(U, dtype=bool)
    last = int(max_iters)
    for i in range(1, last + 1):
        ctx.call("fcd_vb_update_qR", _lib.dptr(lq_F), _lib.dptr(lM), _lib.dptr(hyper), int(Nreg), U, _lib.EDGE_MODES[edge_mode],
                 _lib.dptr(lq_R), _lib.stream_ptr())
        cur = lq_R.cpu().numpy()
        q = np.exp(cur[:, :, 1])
        ok = np.max(np.abs(q - q_prev), axis=0) < tol
        q_prev = q
        stop = (iters == 0) & (ok | (i == last))
        final[:, stop, :] = cur[:, stop, :]
        iters[stop] = i
        converged |= stop & ok
        if np.all(iters > 0):
            break
    lq_R = torch.as_tensor(final, device=bt_dev.device)
    terms = patient_elbo(ctx, lq_F, lq_R, lM, hyper, Nreg, U)
    (p_patient, _p_region) = count_posterior(ctx, lq_R, Nreg, U)
    out = {"p_R": np.exp(lq_R[:, :, 1].cpu().numpy()), "p_patient_count": p_patient, "p_patient_any": 1.0 - p_patient[:, 0],
           "elbo": terms[:, 3].copy(), "iters": iters, "converged": converged}
    if connections:
        out.update(conn_posterior(ctx, bt_dev, Nreg, U, theta, lq_F=lq_F, lq_R=lq_R, missing_data=missing_data,
                                  noise_var=None if noise is None else noise[1]))
    return out


def ais_weights(ctx, b_dev, bt_dev, Nreg, sampler, model, pi2, missing_data, n_anneal, key, noise=None):
    """
    The annealing ladder over r with each chain's template f_g (the end state of `sampler`, read only) held: r from the prior,
    then per rung one fcd_score_ais_step and one r pass on the tempered table.  Returns (eng, lM, region_tables, w, sweep):
    the scoring engine with r ~ p(r | f_g, bt) on the beta = 1 working table, the untempered table, the function that
    rebuilds the engine's region-major table from a table, the log-weights w (G, U) with E exp(w[g, u]) = p(bt_u | f_g), and
    the next free sweep number.
    """
    import torch
    U = int(bt_dev.shape[1])
    G = sampler.G
    theta = model.theta()
    (S_B, lM) = lik_tables(ctx, b_dev, bt_dev, theta, missing_data, noise)
    lMw = lM.clone()                         # the working (tempered) table the r pass reads
    # (built without its tables: no f pass runs while scoring, so the f pass's edge tables are never made; the r pass's
    # region-major table is made here when the fit's sampler had one, and after every rung of the ladder below)
    eng = GibbsEngine(S_B, lMw, Nreg, U, G, chain0=sampler.chain0, seed=key, edge_index="symmetric", ctx=ctx,
                      region_major=False)
    sym = _lib.EDGE_MODES["symmetric"]

    def region_tables(table):
        if eng.lMd is not None:
            ctx.call("fcd_gibbs_region_tables", _lib.dptr(table), int(Nreg), U, sym, _lib.dptr(eng.lMd), _lib.stream_ptr())
    if sampler.lMd is not None:
        eng.lMd = torch.empty((U, Nreg, Nreg, 3, 2), dtype=torch.float64, device=bt_dev.device)
    eng.set_hyper(np.asarray(model.gamma, dtype=np.float64), pi2)
    eng.init(float(pi2[1]))                  # r from the prior: beta = 0 exactly ...
    eng.f_state.copy_(sampler.f_state)       # ... with the fit's template draws in place of the drawn f
    w = torch.zeros((G, U), dtype=torch.float64, device=bt_dev.device)
    betas = ais_schedule(n_anneal)
    sweep = SCORE_SWEEP0
    for t in range(1, len(betas)):
        ctx.call("fcd_score_ais_step", _lib.dptr(lM), _lib.dptr(eng.f_state), _lib.dptr(eng.r_bits), int(Nreg), U, G,
                 float(betas[t - 1]), float(betas[t]), _lib.dptr(w), _lib.dptr(lMw), _lib.stream_ptr())
        region_tables(lMw)
        eng.r_step(sweep)
        sweep += 1
    return eng, lM, region_tables, w, sweep


def score_gibbs(ctx, b_dev, bt_dev, Nreg, sampler, model, pi2, missing_data, connections, n_anneal, n_sweeps, key,
                noise=None):
    """The sampler path of UnsharedRegionFit.score (see there); `sampler` is the fit's engine, read only (its f_state)."""
    import torch
    from .fit import conn_posterior
    U = int(bt_dev.shape[1])
    C = util.N_to_C(int(Nreg))
    G = sampler.G
    theta = model.theta()
    (eng, lM, region_tables, w, sweep) = ais_weights(ctx, b_dev, bt_dev, Nreg, sampler, model, pi2, missing_data, n_anneal, key,
                                                       noise)
    # beta = 1: the untempered table (bit for bit what the last AIS step wrote) and its region-major difference table
    eng.lM = lM
    region_tables(lM)
    hp = torch.zeros((U, Nreg + 1), dtype=torch.int32, device=bt_dev.device)
    hr = torch.zeros((Nreg, U + 1), dtype=torch.int32, device=bt_dev.device)
    acc = torch.zeros((C, U, 3, 3), dtype=torch.int32, device=bt_dev.device) if connections else None
    for _ in range(int(n_sweeps)):
        eng.r_step(sweep)
        sweep += 1
        eng.tally(want_counts=False, accumulate=True)
        eng.count_tally(hp, hr)
        if connections:
            eng.pair_tally(acc)
    # pooled over this rank's chains and, when the fit was sharded, over every rank's
    n_chains = allreduce_counts(torch.tensor([G], dtype=torch.int64, device=bt_dev.device)).cpu().numpy()
    cnt_r = pool_u32(eng.cnt_r)
    hp = pool_u32(hp).cpu().numpy().astype(np.float64)
    parts = chain_parts(ctx, w)
    p_R = cnt_r.cpu().numpy().astype(np.float64) / (float(n_chains[0]) * int(n_sweeps))
    ctx.check_device()
    p_patient = hp / hp.sum(axis=1, keepdims=True)
    (log_pred, se, ess) = pool_ais(parts)
    out = {"p_R": p_R, "p_patient_count": p_patient, "p_patient_any": 1.0 - p_patient[:, 0], "log_pred": log_pred,
           "log_pred_se": se, "ess": ess}
    if connections:
        pc = pool_u32(acc).cpu().numpy()
        if int(pc.max()) > PAIR_COUNT_MAX:
            raise ValueError("pooled connection counts exceed uint32: fewer sweeps or chains")
        out["connection_counts"] = pc
        counts = torch.as_tensor(np.ascontiguousarray(pc.astype(np.uint32).view(np.int32)), device=bt_dev.device)
        out.update(conn_posterior(ctx, bt_dev, Nreg, U, theta, counts=counts, missing_data=missing_data,
                                  noise_var=None if noise is None else noise[1]))
    return out
