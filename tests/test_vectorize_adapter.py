"""The C++ header for the vector map (nautilus_amd/adapters/vectorize_hip.h): what VectorizeMap returns on clouds and poses
this test wrote equals the Python binding's output byte for byte, and the file io::WriteMapLines makes of it reads back as
hostside.write_map_lines' does.  The binary is built by __graft_entry__.build() (g++, links libnautilus_hip.so) and needs a
GPU to run."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "nautilus_amd", "adapters", "vectorize_test")


def test_adapter_header_declares_the_call():
    h = open(os.path.join(ROOT, "nautilus_amd", "adapters", "vectorize_hip.h")).read()
    for s in ("namespace nautilus_hip {", "inline std::vector<LineSegment> VectorizeMap(const std::vector<std::vector<Vec2f>> &scans,",
              "inline nhip_vectorize_spec_t VectorizeSpec(", "nhip_vectorize(handle.h"):
        assert s in h


@pytest.mark.gpu
def test_adapter_binary_equals_the_python_binding(gpu, tmp_path):
    from nautilus_amd import csm, hostside, synth, vectorize
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-C", os.path.dirname(BIN), "vectorize_test"])
    bag = synth.SynthBag(24)
    clouds, poses = list(bag.scans) + [np.zeros((0, 2), np.float32)], np.concatenate([bag.odom, [[1.0, 2.0, 0.5]]])
    with open(os.path.join(tmp_path, "clouds.bin"), "wb") as f:
        f.write(np.array([len(clouds)] + [len(c) for c in clouds], np.int32).tobytes())
        for c in clouds:
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
    poses.astype(np.float64).tofile(os.path.join(tmp_path, "poses.f64"))
    p = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "VECTORIZE_OK 25 scans" in p.stdout, p.stdout + p.stderr
    xy, off = csm.pack_scans(clouds)
    spec = vectorize.window_spec(poses, 30.0)  # (VectorizeSpec states the same window)
    want, _, stats = vectorize.vectorize(xy, off, poses, spec)
    got = np.fromfile(os.path.join(tmp_path, "lines.f32"), dtype=np.float32).reshape(-1, 4)
    assert len(want) > 5 and got.tobytes() == want.tobytes()
    assert np.fromfile(os.path.join(tmp_path, "stats.i32"), dtype=np.int32).tolist() == stats.tolist()
    mine = os.path.join(tmp_path, "python.txt")
    hostside.write_map_lines(mine, want)
    assert np.array_equal(hostside.read_map_lines(os.path.join(tmp_path, "map.txt")), hostside.read_map_lines(mine))
