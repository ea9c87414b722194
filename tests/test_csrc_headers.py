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
                         "sigma_cluster", "sigma_sw", "sigma_sw_tiled", "sigma_sw_chain", "sigma_sw_correlator", "sigma_levels",
                         "sigma_twolevel", "schwinger_or_block", "runtime", "options", "schwinger_analytic", "index_maps", "sigma_field",
                         "sigma_smooth")
SW_UNITS = ("sigma_sw", "sigma_sw_tiled", "sigma_sw_chain", "sigma_sw_correlator")


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


def _deps(build, unit):
    with open(os.path.join(build, unit + ".d")) as f:
        deps = {os.path.basename(w.rstrip(":")) for w in re.split(r"[\s\\]+", f.read()) if w}
    assert unit + ".hip" in deps and "device_common.hpp" in deps, (unit, sorted(deps))   # the file is what it should be
    return deps


def test_units_without_a_sampler_include_no_sampler_header():
    build = os.path.join(CSRC, "build")
    if not os.path.isdir(build):
        pytest.skip("no built tree")
    for unit in UNITS_WITHOUT_SAMPLER:
        deps = _deps(build, unit)
        assert not deps & SAMPLER_HEADERS, (unit, sorted(deps & SAMPLER_HEADERS))


def test_the_cluster_samplers_share_the_embedding_and_nothing_of_each_other():
    """Wolff (sigma_cluster) and Swendsen-Wang (sigma_sw*) meet in sigma_cluster_device.hpp only: the Wolff unit does not see
    the Swendsen-Wang device library or its host header, and the Wolff-only device code is in sigma_cluster.hip itself, which no
    unit includes."""
    build = os.path.join(CSRC, "build")
    if not os.path.isdir(build):
        pytest.skip("no built tree")
    wolff = _deps(build, "sigma_cluster")
    assert "sigma_cluster_device.hpp" in wolff
    assert not wolff & {"sigma_sw_device.hpp", "sigma_sw_host.hpp"}, sorted(wolff)
    with open(os.path.join(CSRC, "sigma_cluster_device.hpp")) as f:
        shared = f.read()
    assert "wolff_" not in shared and "WolffImproved" not in shared and "uf_union" not in shared
    for unit in SW_UNITS:
        deps = _deps(build, unit)
        assert {"sigma_cluster_device.hpp", "sigma_sw_host.hpp"} <= deps, (unit, sorted(deps))
        assert "sigma_cluster.hip" not in deps, (unit, sorted(deps))


def test_the_smoothers_share_the_field_and_the_driver_and_nothing_of_each_other():
    """Cooling (sigma_cooling) and the gradient flow (sigma_flow) meet in the field of unit vectors (sigma_field_device.hpp, whose
    kernels and launches sigma_field.hip owns) and in the smoothing driver (sigma_smooth_host.hpp, sigma_smooth.hip): neither sees
    the other, and neither the field nor the driver sees a smoother."""
    build = os.path.join(CSRC, "build")
    if not os.path.isdir(build):
        pytest.skip("no built tree")
    smoothers = {"sigma_cooling.hip", "sigma_flow.hip"}
    for unit in ("sigma_cooling", "sigma_flow"):
        deps = _deps(build, unit)
        assert {"sigma_field_device.hpp", "sigma_smooth_host.hpp"} <= deps, (unit, sorted(deps))
        assert deps & smoothers == {unit + ".hip"}, (unit, sorted(deps))
    for unit in ("sigma_field", "sigma_smooth"):
        deps = _deps(build, unit)
        assert "sigma_field_device.hpp" in deps and not deps & smoothers, (unit, sorted(deps))
    with open(os.path.join(CSRC, "sigma_field_device.hpp")) as f:
        shared = f.read()
    assert "cool_" not in shared and "flow_" not in shared


def test_fillin_and_sigma_device_meet_in_test_math_only():
    """sigma_device.hpp switches fp contraction off for the rest of the file that includes it, fillin.hpp's callers are compiled
    with it on: the one unit that needs the primitives of both is test_math, whose kernel only calls functions compiled where
    they are defined.  Every unit the Makefile compiles is looked at."""
    build = os.path.join(CSRC, "build")
    if not os.path.isdir(build):
        pytest.skip("no built tree")
    with open(os.path.join(CSRC, "Makefile")) as f:
        units = [w[:-4] for w in re.search(r"^SRCS := (.*)$", f.read(), re.M).group(1).split()]
    assert len(units) >= 35 and "test_math" in units and "runtime" in units
    both = [u for u in units if {"fillin.hpp", "sigma_device.hpp"} <= _deps(build, u)]
    assert both == ["test_math"], both
