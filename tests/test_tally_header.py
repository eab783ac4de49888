"""
The plain-C++ part of fcdiff_amd/csrc/fcd_tally.h (shared by the count, region-set, patient-group and patient-trait
tallies) on the host: the header compiles under g++, so its bit-sliced counters are driven here with 64 independent chains
against per-chain integer counts -- all-zero input, every chain at 1 / 511 / 512 / 1022 / 1023 at once, a few thousand
random words; any() against count > 0, store16 against the layout "chain c at row[c]" -- and the CSR checks of the region
sets and patient groups against one accepted input and every refusal's message text, without a GPU.  The kernels that use
the header are checked against NumPy in test_gpu_count_posterior.py, test_gpu_region_sets.py, test_gpu_patient_groups.py,
test_gpu_patient_traits.py and test_gpu_post_wraps.py.
"""
import os
import subprocess

from conftest import ROOT


def test_tally_header_on_the_host(tmp_path):
    exe = str(tmp_path / "tally_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "tally_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0, out
    (word, checks) = out.split()
    assert word == "ok" and int(checks) > 60000, out        # (530 comparisons of 64 chains, two checks each)
