"""CPU: the sampler headers of include/mlmcpi each compile as the only include of an otherwise empty translation unit, and
cluster_improved.hh reaches no ABI or device header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("header", ["sampler.hh", "cluster_sampler.hh", "cluster_improved.hh"])
def test_header_compiles_on_its_own(header, tmp_path):
    unit = tmp_path / "unit.cc"
    unit.write_text('#include "mlmcpi/%s"\n' % header)
    cxx = os.environ.get("CXX", "g++")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(unit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if header == "cluster_improved.hh":
        r = subprocess.run([cxx, "-std=c++17", "-MM", "-I" + os.path.join(ROOT, "include"), str(unit)], capture_output=True, text=True)
        deps = {os.path.basename(w) for w in r.stdout.replace("\\\n", " ").split()[2:]}
        assert deps == {"cluster_improved.hh", "chain_estimate.hh", "correlator.hh"}, deps
