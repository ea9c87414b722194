"""The C++ host samplers (include/mlmcpi/*.hh) pinned to the raw ABI calls they stand for, draw by draw: host/test_replay
drives each class through its public interface and, beside it, issues the documented sequence of mlmcpi_* calls on buffers
of its own; after every draw the two states must agree bit for bit, and a sample handed out must never change afterwards
("the host layer's counter contract").  One process per case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_replay")

CASES = ["samplestate", "heatbath_sweeps", "heatbath_random", "hmc", "exact_and_cluster", "twolevel", "hierarchical", "mlmc_table"]


def build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mlmcpathintegral_amd", "csrc")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host")])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_host_sampler_replays_its_abi_calls(case):
    if not os.path.exists(EXE):
        build()
    r = subprocess.run([EXE, case], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.rstrip().endswith("all checks passed")


def test_replay_program_names_its_cases():
    """Without a GPU: an unknown case is refused with the list of cases, which is the list this file runs."""
    if not os.path.exists(EXE):
        build()
    r = subprocess.run([EXE, "no_such_case"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert r.stderr.split("one of")[1].split() == CASES
