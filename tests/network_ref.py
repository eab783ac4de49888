"""
NumPy reference of baseline.network_test and baseline.graph_components: a plain union-find over the loop-level t of
baseline_ref.py.  The t of a data set do not depend on the threshold, so they are made once (group_t) and thresholded often.
"""
import functools
import math

import numpy as np

import baseline_ref as BR
from fcdiff_amd import util


def components(mask, N):
    """
    Components of the graph on N regions whose edges are the set entries of mask (C,), connections in util.c_to_nm order.
    Returns a dict: component (N,) int64 = smallest region of the region's component, -1 for a region without an edge;
    component_label, component_edges, component_regions (K,) int64 by decreasing extent, then by label; n_edges, max_extent,
    max_regions (ints; 0 where no connection is set).
    """
    mask = np.asarray(mask).astype(bool)
    assert mask.shape == (util.N_to_C(N),)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    touched = [False] * N
    set_edges = []
    for c in range(mask.shape[0]):
        if mask[c]:
            (n, m) = util.c_to_nm(c)
            set_edges.append((n, m))
            touched[n] = touched[m] = True
            (a, b) = (find(n), find(m))
            if a != b:
                parent[max(a, b)] = min(a, b)           # the root of a set is its smallest member
    component = np.array([find(x) if touched[x] else -1 for x in range(N)], dtype=np.int64)
    extent = {}
    for (n, _m) in set_edges:
        extent[int(component[n])] = extent.get(int(component[n]), 0) + 1
    order = sorted(extent, key=lambda lab: (-extent[lab], lab))
    regions = [int((component == lab).sum()) for lab in order]
    return {"component": component, "component_label": np.array(order, dtype=np.int64),
            "component_edges": np.array([extent[lab] for lab in order], dtype=np.int64),
            "component_regions": np.array(regions, dtype=np.int64), "n_edges": len(set_edges),
            "max_extent": max(extent.values()) if extent else 0, "max_regions": max(regions) if regions else 0}


def group_t(b, bt, labels):
    """(t (C,), null_t (P, C)): baseline_ref's loop-level pooled-variance t of the observed labelling and of every row."""
    (C, H) = b.shape
    U = bt.shape[1]
    S = H + U
    X = np.concatenate([b, bt], axis=1)
    (xc, q) = BR.centre(X)
    observed = [0] * H + [1] * U
    t = np.array([BR._t_of(xc[c], q[c], observed, S, U, H) for c in range(C)])
    tp = np.array([[BR._t_of(xc[c], q[c], lab, S, U, H) for c in range(C)] for lab in labels]).reshape(len(labels), C)
    return t, tp


def suprathreshold(t, threshold, tail):
    if tail == "both":
        return np.abs(t) > threshold
    if tail == "greater":
        return t > threshold
    if tail == "less":
        return t < -threshold
    raise ValueError(tail)


def network_test(b, bt, labels, threshold, tail="both", t_pair=None):
    """Every key of baseline.network_test(b, bt, threshold, labels=labels, tail=tail) but `labels`; also null_t (P, C)."""
    (t, tp) = t_pair if t_pair is not None else group_t(b, bt, labels)
    N = int(round(util.C_to_N(b.shape[0])))
    P = tp.shape[0]
    obs = components(suprathreshold(t, threshold, tail), N)
    null = [components(suprathreshold(tp[p], threshold, tail), N) for p in range(P)]
    null_max_extent = np.array([r["max_extent"] for r in null], dtype=np.int64)
    p_fwe = np.array([(1.0 + sum(1 for v in null_max_extent if v >= e)) / (1.0 + P) for e in obs["component_edges"]])
    p_of = dict(zip(obs["component_label"].tolist(), p_fwe.tolist()))
    return {"t": t, "edge_mask": suprathreshold(t, threshold, tail), "component": obs["component"],
            "component_label": obs["component_label"], "component_edges": obs["component_edges"],
            "component_regions": obs["component_regions"], "null_max_extent": null_max_extent,
            "null_max_regions": np.array([r["max_regions"] for r in null], dtype=np.int64),
            "null_n_edges": np.array([r["n_edges"] for r in null], dtype=np.int64), "p_fwe": p_fwe,
            "p_fwe_region": np.array([p_of.get(int(lab), math.nan) for lab in obs["component"]]),
            "threshold": float(threshold), "tail": tail, "null_t": tp,
            "null_components": np.array([len(r["component_label"]) for r in null], dtype=np.int64)}


def threshold_gap(t, tp, threshold):
    """Smallest relative distance | |t| - threshold | / threshold over the observed and the permuted t."""
    a = np.abs(np.concatenate([np.asarray(t).reshape(-1), np.asarray(tp).reshape(-1)]))
    return float((np.abs(a - threshold) / threshold).min())


# the cases of the device test: baseline_ref.SHAPES, the three extra group_test shapes, and one with more than 32 regions
# (780 connections over 25 words)
SHAPES = BR.SHAPES + [(4, 100, 45, 20, 5), (3, 1000, 24, 3, 6), (4, 10, 9, 150, 7), (40, 12, 10, 40, 8)]


@functools.lru_cache(maxsize=None)
def data_case(shape):
    """(b, bt, labels, (t, null_t)) of a shape, made once."""
    (b, bt, labels) = BR.make_data(*shape)
    return b, bt, labels, group_t(b, bt, labels)


@functools.lru_cache(maxsize=None)
def case(shape, threshold, tail="both"):
    (b, bt, labels, t_pair) = data_case(shape)
    return b, bt, labels, network_test(b, bt, labels, threshold, tail, t_pair=t_pair)
