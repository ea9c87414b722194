"""CPU: the layering of the device headers in mlmcpathintegral_amd/csrc.  Every header compiles on its own (make
check-headers), and the units that draw from no heat-bath sampler do not include one: read from the dependency files the
compiler wrote beside the objects of a built tree."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")
SAMPLER_HEADERS = {"vonmises.hpp", "step_envelope.hpp", "site_update.hpp", "fillin.hpp"}
UNITS_WITHOUT_SAMPLER = ("path1d", "path_hmc", "ho_exact", "lattice_reduce", "lattice_hmc", "gff_exact", "gff_levels", "cluster",
                         "sigma_cluster", "sigma_sw", "sigma_levels", "sigma_twolevel", "schwinger_or_block")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    return None


def test_every_header_compiles_on_its_own():
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "check-headers", "HIPCC=" + hipcc], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_units_without_a_sampler_include_no_sampler_header():
    build = os.path.join(CSRC, "build")
    if not os.path.isdir(build):
        pytest.skip("no built tree")
    for unit in UNITS_WITHOUT_SAMPLER:
        with open(os.path.join(build, unit + ".d")) as f:
            deps = {os.path.basename(w.rstrip(":")) for w in re.split(r"[\s\\]+", f.read()) if w}
        assert unit + ".hip" in deps and "device_common.hpp" in deps, (unit, sorted(deps))   # the file is what it should be
        assert not deps & SAMPLER_HEADERS, (unit, sorted(deps & SAMPLER_HEADERS))
