"""CPU: the once-per-device guard of the LDS-heavy units (mlmcpathintegral_amd/csrc/device_once.hpp) through the stand-alone
host/test_device_once, which includes that header alone and links nothing of the library: 16 threads x 4 device indices run an
init exactly once per device, an init that fails is not latched, and the indices -1 and 64 are refused without a call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "test_device_once")


def test_device_once():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), EXE])   # (its own target: the library is not needed)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "test_device_once OK", r.stdout
