"""
The walk of the sparse r pass (gibbs_r_sparse_kernel) cuts a wave's visit list into segments of RS_SEG listed sites: per
segment one phase without dependencies (loads, Philox blocks, the sums over the regions outside the segment) and one serial
chain over the segment's own bits.  These cases are the smallest shapes at which that structure can go wrong; each is checked
the way tests/test_gpu_r_decided.py checks its own (run_case of that file): chains, marginal counters and pooled counts equal
to the C oracle's bit for bit, the four r_sure_* counters equal to the CPU prediction, dev_err == 0.

  list length around the segment   every site listed in the full chain word (r_sure = 2, r_sure_x = 0.25: a decided site stays
                                   off the list only where every chain's uniform lies in [0.25, 0.75]), about half of them in
                                   the one-chain word: Nreg = S - 1, S, S + 1, 2 S, 2 S + 1
  open count straddling S          a scaled table whose patients have fewer and more than S open sites (asserted on the CPU)
  Nreg = 270                       regions past the first four 64-region words
  G = 1, G = 130, chain0 != 0      a single chain, a partial last word, one patient
  slow sites among fast ones       an edge without a mode (its two rows are walked per chain) and -inf entries (NaN base), with
                                   r_sure_x = 0.25 so that decided sites of the other rows join the same segments
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import r_sure_ref as RS  # noqa: E402
from test_gpu_r_decided import N_SWEEPS, Call, env, run_case, scaled, tables_for  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def segment_size():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fcdiff_amd", "csrc", "fcd_gibbs_r.hip")
    with open(src) as fh:
        return int(re.search(r"constexpr int RS_SEG = (\d+);", fh.read()).group(1))


S = segment_size()


def sparse_in_every_pass(rise, forms):
    assert rise["r_sure_passes"] == N_SWEEPS - 2 and forms == [4]


def open_per_patient(m, N, U, S_B, lM):
    (_km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, S_B, lM, np.log(m.gamma))
    (d0, d1) = RS.decided(hi, lo, float(np.log(m.pi) - np.log(1.0 - m.pi)), rowflag)
    return (~(d0 | d1)).sum(axis=0)


@pytest.mark.parametrize("N", (S - 1, S, S + 1, 2 * S, 2 * S + 1))
def test_list_length_around_the_segment(env, N):
    (U, G) = (3, 65)
    (m, S_B, lM) = tables_for(env, N, 16, U, seed=3)
    (rise, forms) = run_case(env, "seg-len-%d" % N, m, N, U, G, 300 + N, 2, [Call(S_B, lM, N_SWEEPS)], knob=2, x=0.25)
    sparse_in_every_pass(rise, forms)


def test_open_count_straddles_the_segment(env):
    (N, U, G, factor) = (80, 4, 130, 0.8)
    (m, S_B, lM) = scaled(env, N, U, factor)
    n_open = open_per_patient(m, N, U, S_B, lM)
    assert n_open.min() < S < n_open.max(), n_open
    (rise, forms) = run_case(env, "straddle", m, N, U, G, 511, 6, [Call(S_B, lM, N_SWEEPS)], knob=2)
    sparse_in_every_pass(rise, forms)
    assert rise["r_sure_sites"] > 0


def test_regions_past_four_words(env):
    (N, U, G) = (270, 2, 65)
    (m, S_B, lM) = tables_for(env, N, 16, U, seed=9)
    (rise, forms) = run_case(env, "nreg-270", m, N, U, G, 270, 1, [Call(S_B, lM, N_SWEEPS)], knob=2)
    sparse_in_every_pass(rise, forms)


@pytest.mark.parametrize("G", (1, 130))
def test_one_patient_one_chain_partial_word(env, G):
    (N, U) = (S + 8, 1)
    (m, S_B, lM) = tables_for(env, N, 16, U, seed=4)
    (rise, forms) = run_case(env, "one-patient-%d" % G, m, N, U, G, 77 + G, 9, [Call(S_B, lM, N_SWEEPS)], knob=2, x=0.25)
    sparse_in_every_pass(rise, forms)


def test_an_open_edge_among_fast_sites(env):
    """masked tables (f_pass_table_cases.missing), scaled as in tests/test_gpu_r_decided.py: rows 4 and 3 are slow, and with
    r_sure_x = 0.25 the decided sites of the other rows are listed beside them -- Nreg 13: one segment holds both kinds"""
    import f_pass_table_cases as FC
    (S_B, lM, N, U, p) = FC.build("missing-13")
    m = FC.model()
    S8 = 8.0 * S_B
    S8[p["zero_lM"]] = S_B[p["zero_lM"]]
    (_km, _lMd, hi, lo, _base, rowflag) = RS.tables_for_call(N, U, S8, 8.0 * lM, np.log(m.gamma))
    assert rowflag[4] and rowflag[3] and not rowflag.all()
    assert RS.share(hi, lo, float(np.log(m.pi) - np.log(1.0 - m.pi)), rowflag) > 0.0
    (rise, forms) = run_case(env, "missing-13-x", m, N, U, 65, 43, 2, [Call(S8, 8.0 * lM, N_SWEEPS)], knob=2, x=0.25)
    sparse_in_every_pass(rise, forms)
    assert rise["r_sure_exceptions"] > 0


def test_minus_infinity_among_fast_sites(env):
    """the `firm` set of tests/nonfinite_tables.py (Nreg 33: two segments at S = 32, three at 16): sites with a NaN base are
    slow, r_sure_x = 0.25 lists decided sites of finite rows around them"""
    import nonfinite_tables as NF
    T = NF.build_set("firm-33-7", 130)
    m = env.pkg.UnsharedRegionModel()
    (m.gamma, m.pi) = (T.gamma.copy(), float(T.pi2[1]))
    with np.errstate(invalid="ignore"):
        (_km, _lMd, hi, _lo, base, rowflag) = RS.tables_for_call(T.Nreg, T.U, T.S_B, T.lM, T.lng)
    assert np.isnan(hi).any() and not rowflag.all()
    assert np.isnan(base).any() and np.isfinite(base).any()
    (rise, forms) = run_case(env, "firm-33-7-x", m, T.Nreg, T.U, 130, T.seed, 0, [Call(T.S_B, T.lM, N_SWEEPS)], knob=2, x=0.25,
                             hyper0=(T.gamma, T.pi2))
    sparse_in_every_pass(rise, forms)
