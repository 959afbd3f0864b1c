"""FastGicpRegistration of the C++ host mirror (lis-slam_amd/host/lis_slam_registration.hpp): lis-slam_amd/host/fgicp_smoke.cpp
builds with plain g++ and, on a GPU box, aligns a small synthetic scene as select_registration_method("FAST_GICP") would, checking the
recovered pose, the pcl::Registration surface and the setters inside the program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")


def test_fgicp_smoke_compiles_and_fails_loudly_without_a_device():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists (builds it if the tree is fresh)
    subprocess.check_call(["make", "-s", "-C", HOST, "fgicp_smoke"])
    assert os.path.exists(os.path.join(HOST, "fgicp_smoke"))
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    body = hdr[hdr.index("class FastGicpRegistration"):hdr.index("// OptimizedICPGN")]
    for name in ("setMaxCorrespondenceDistance", "setCorrespondenceRandomness", "setTransformationEpsilon", "setMaximumIterations",
                 "setInputTarget", "setInputSource", "align", "hasConverged", "getFitnessScore", "getFinalTransformation"):
        assert name in body, name


@pytest.mark.gpu
def test_fgicp_smoke_runs():
    exe = os.path.join(HOST, "fgicp_smoke")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "fgicp_smoke ok" in r.stdout, r.stdout + r.stderr
