"""The C++ drop-in for normal_computation.h (nautilus_amd/adapters/normal_computation_hip.h): what GetNormals (one scan per
call) and GetNormalsBatch return on clouds this test wrote equals the Python binding's output, byte for byte.  The binary
is built by __graft_entry__.build() (g++, links libnautilus_hip.so) and needs a GPU to run."""
import os
import subprocess

import numpy as np
import pytest

from tests import normals_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nautilus_amd", "adapters", "normals_test")


def test_adapter_header_mirrors_the_reference_signature():
    h = open(os.path.join(ROOT, "nautilus_amd", "adapters", "normal_computation_hip.h")).read()
    for s in ("namespace nautilus {", "namespace NormalComputation {", "std::vector<Vector2f> GetNormals(const std::vector<Vector2f> &points)",
              "GetNormalsBatch(const std::vector<std::vector<Vector2f>> &clouds)"):
        assert s in h


@pytest.mark.gpu
def test_adapter_binary_equals_the_python_binding(gpu, tmp_path):
    from nautilus_amd import csm, normals
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN), "normals_test"])
    rng = np.random.default_rng(3)
    clouds = [R.wall_scan(n, rng) for n in (300, 0, 1, 65, 1100)]  # (both forms of the kernel, an empty cloud, a lone point)
    with open(os.path.join(tmp_path, "clouds.bin"), "wb") as f:
        f.write(np.array([len(clouds)] + [len(c) for c in clouds], np.int32).tobytes())
        for c in clouds:
            f.write(c.astype(np.float32).tobytes())
    p = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "NORMALS_OK 5 clouds" in p.stdout, p.stdout + p.stderr
    xy, off = csm.pack_scans(clouds)
    want = normals.estimate(xy, off)
    assert np.abs(want[:300]).max() > 0.5 and not want[300].any()  # (normals; the lone point has none)
    for name in ("single.f32", "batch.f32"):
        got = np.fromfile(os.path.join(tmp_path, name), dtype=np.float32).reshape(-1, 2)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
