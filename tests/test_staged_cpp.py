"""The staged call of the handle forms (nautilus_amd/csrc/nhip_host.h, Staged) on its first-failure path: a stand-alone host
program (nautilus_amd/adapters/staged_test.cc) built from the library's runtime unit with the host sanitizers, run with no
HIP device visible, so that its first allocation fails.  No GPU needed, none touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTERS = os.path.join(ROOT, "nautilus_amd", "adapters")


def test_first_failure_is_sticky_and_destruction_clean():
    subprocess.check_call(["make", "-C", ADAPTERS, "staged_test"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    p = subprocess.run([os.path.join(ADAPTERS, "staged_test")], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0 and "STAGED_OK" in p.stdout, p.stdout + p.stderr
