"""
The knob table of a context (fcdiff_amd/csrc/fcd_knobs.h) on the host: the header needs nothing from HIP, so
tests/ctx_check.cpp includes it alone under g++ and checks, against expectations written out by hand, that each of the 24
knobs is set by its ABI name and lands in its own member (ints truncated, doubles kept), that an unknown name is refused,
that exactly the fourteen documented environment variables change a default -- read through a fake getenv -- with
FCD_R_COOP=2 giving 0 and =1 giving 1, that "0" and "" mean the default, and that no two rows share a name, an
environment name or a member.  The knobs' effects are the business of the GPU tests, which reach them through
fcd_ctx_set_knob.
"""
import os
import subprocess

from conftest import ROOT


def test_knob_table_on_the_host(tmp_path):
    exe = str(tmp_path / "ctx_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "ctx_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0, out
    (word, checks) = out.split()
    # 24 knobs x (6 values at the most x 25 checks, then five fake environments x 24 checks): the program ran all of it
    assert word == "ok" and int(checks) > 5000, out
