"""
bench.py --dump-outputs without a GPU: the writer stays within 64 MB, writes only float32 / float64, and cuts the chain
states of a large run to the same rows of f and r every time.
"""
import os

import numpy as np

import bench


def fake_outputs(G, Nreg, U, seed=0):
    rng = np.random.RandomState(seed)
    C = Nreg * (Nreg - 1) // 2
    return {"q_F": rng.rand(C, 3), "q_R": rng.rand(Nreg, U), "pi": np.array([0.1]), "gamma": rng.rand(3),
            "f": rng.randint(0, 3, (G, C)).astype(np.uint8), "r": rng.randint(0, 2, (G, Nreg, U)).astype(np.uint8)}


def read_dir(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_small_run_is_written_whole(tmp_path):
    o = fake_outputs(64, 12, 6)
    bench.write_outputs(np, str(tmp_path), o)
    got = read_dir(str(tmp_path))
    assert set(got) == {"q_F", "q_R", "pi", "gamma", "f", "r"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for k in o:
        np.testing.assert_array_equal(got[k], o[k])


def test_cfg3_run_keeps_a_fixed_sample_of_whole_chains_within_64_MB(tmp_path):
    o = fake_outputs(1024, 200, 50)
    (a, b) = (str(tmp_path / "a"), str(tmp_path / "b"))
    bench.write_outputs(np, a, o)
    bench.write_outputs(np, b, o)
    assert sum(os.path.getsize(os.path.join(a, n)) for n in os.listdir(a)) <= 64 << 20
    (ga, gb) = (read_dir(a), read_dir(b))
    n = ga["f"].shape[0]
    assert 1 <= n < 1024 and ga["r"].shape == (n, 200, 50)
    keep = np.sort(np.random.RandomState(0).choice(1024, n, replace=False))
    np.testing.assert_array_equal(ga["f"], o["f"][keep])
    np.testing.assert_array_equal(ga["r"], o["r"][keep])
    for k in ga:
        np.testing.assert_array_equal(ga[k], gb[k])
    np.testing.assert_array_equal(ga["q_F"], o["q_F"])
