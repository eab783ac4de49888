"""
NumPy reference of baseline.network_test(..., statistic="intensity") and baseline.graph_components(mask, weights): the graph
by network_ref.components (union-find), every component's sum by math.fsum, on the loop-level t of network_ref.group_t,
baseline_missing_ref.all_t or baseline_glm_ref.all_t.

The excess of a suprathreshold connection is e = max(|t| - threshold, 0); a NaN t (dead, undefined) is never suprathreshold
and adds nothing; t = +/-inf gives e = +inf, and inf >= inf counts in a p-value.
"""
import functools
import math

import numpy as np

import network_ref as NR
from fcdiff_amd import util


def excess(t, threshold, tail):
    """(mask (C,) bool, e (C,)): e = max(|t| - threshold, 0) where the connection is suprathreshold, 0.0 elsewhere."""
    with np.errstate(invalid="ignore"):
        mask = NR.suprathreshold(np.asarray(t, dtype=np.float64), threshold, tail)
        e = np.where(mask, np.maximum(np.abs(t) - threshold, 0.0), 0.0)
    return mask, e


def weighted_components(mask, weights, N):
    """
    network_ref.components(mask, N) with component_weight (K,), the fsum of the weights over each listed component's
    connections, max_weight (0.0 for an empty graph) and arg_extent, the extent of the first component that reaches it.
    A weight is read only where the mask is set.
    """
    mask = np.asarray(mask).astype(bool)
    out = NR.components(mask, N)
    terms = dict((int(lab), []) for lab in out["component_label"])
    for c in np.flatnonzero(mask):
        (n, _m) = util.c_to_nm(int(c))
        terms[int(out["component"][n])].append(float(weights[c]))
    sums = [math.fsum(terms[int(lab)]) if not any(math.isinf(v) for v in terms[int(lab)]) else math.inf
            for lab in out["component_label"]]
    out["component_weight"] = np.array(sums, dtype=np.float64)
    out["max_weight"] = max(sums) if sums else 0.0
    out["arg_extent"] = int(out["component_edges"][int(np.argmax(sums))]) if sums else 0
    return out


def from_t(t, tp, threshold, tail="both"):
    """
    Every key of baseline.network_test(..., statistic="intensity") but labels / permutations, from the observed t (C,) and the
    permuted t (P, C); also null_t, null_arg_extent (P,) = the extent of each labelling's largest-intensity component (for the
    tolerance) and null_extent_of_max (P,) bool = that component is one of the labelling's largest by extent.
    """
    (t, tp) = (np.asarray(t, dtype=np.float64), np.asarray(tp, dtype=np.float64))
    tp = np.where(np.isnan(t)[None, :], np.nan, tp)            # a dead connection is dead under every labelling
    N = int(round(util.C_to_N(t.shape[0])))
    P = tp.shape[0]
    with np.errstate(invalid="ignore"):
        out = _extent(t, tp, threshold, tail)
    (mask, e) = excess(t, threshold, tail)
    obs = weighted_components(mask, e, N)
    null = [weighted_components(*excess(tp[p], threshold, tail), N) for p in range(P)]
    null_max = np.array([r["max_weight"] for r in null], dtype=np.float64)
    ci = obs["component_weight"]
    p_int = np.array([(1.0 + sum(1 for v in null_max if v >= x)) / (1.0 + P) for x in ci])
    p_of = dict(zip(obs["component_label"].tolist(), p_int.tolist()))
    out.update({"component_intensity": ci, "null_max_intensity": null_max, "p_fwe_extent": out["p_fwe"], "p_fwe": p_int,
                "p_fwe_region": np.array([p_of.get(int(lab), math.nan) for lab in obs["component"]]),
                "statistic": "intensity",
                "null_arg_extent": np.array([r["arg_extent"] for r in null], dtype=np.int64),
                "null_extent_of_max": np.array([r["arg_extent"] == r["max_extent"] for r in null], dtype=bool)})
    return out


def _extent(t, tp, threshold, tail):
    """network_ref.network_test on a given pair of t (its b is only asked for the number of connections)."""
    return NR.network_test(np.empty((t.shape[0], 0)), None, None, threshold, tail, t_pair=(t, tp))


def intensity_gap(ref):
    """Smallest relative distance |a - b| / max(a, b) between an observed intensity and a null maximum (inf if there is no pair;
    a pair of equal infinities is no distance at all: inf >= inf is decided exactly)."""
    gap = math.inf
    for a in ref["component_intensity"]:
        for b in ref["null_max_intensity"]:
            if math.isinf(a) or math.isinf(b):               # (decided exactly: inf >= inf counts, inf > every finite sum)
                continue
            gap = min(gap, abs(a - b) / max(a, b) if max(a, b) > 0.0 else math.inf)
    return gap


def tolerance(ref_value, extent, threshold, rtol=1e-10):
    """rtol on every |t| of the sum, carried through the subtraction: sum |t| = intensity + extent * threshold."""
    return rtol * (ref_value + extent * threshold)


@functools.lru_cache(maxsize=None)
def case(shape, threshold, tail="both"):
    """(b, bt, labels, ref) of a network_ref shape: network_ref's data and t, made once."""
    (b, bt, labels, (t, tp)) = NR.data_case(shape)
    return b, bt, labels, from_t(t, tp, threshold, tail)
