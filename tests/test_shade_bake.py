"""The baked hemisphere basis of the FT_NONE kernels (csrc/jt_bsdf.h basis_baked), enumerated on the CPU.

tests/shade_bake_check.cpp is a stand-alone program (its own main, nothing loaded into Python): over
the axis normals with every zero sign, normals with z = +-0, the zero vectors, denormal components and
1.2 million random normals it compares, bit for bit, basis_fromz(-n) with the sign changes of
basis_fromz(n) that the kernels apply, the nine entries rebuilt from the six stored ones in both
orientations, and the XOR of eval_shading's and up_normal's predicates with up_normal called on the
oriented normal. It is built here with the host compiler under the address and undefined-behaviour
sanitizers, without floating-point contraction, and run once.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_baked_basis_matches_basis_fromz(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "shade_bake_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "shade_bake_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout


def test_frame_with_negative_zero_is_not_a_matte_kernel_scene(abi, lib):
    """The baking kernels overwrite the LDS copy of enrm, which element_normal reads for an instance
    that is not rot_identity. A frame with a -0 entry has an identity inverse under == and is not
    bitwise the identity rotation: the layout counts it under FT_XFORM (128), so such a scene never
    runs a kernel without that bit. The same scene with +0 has no feature at all."""
    import ctypes as C

    import numpy as np

    from conftest import make_params
    from jtrace import trace
    from jtrace.scene import CameraData, InstanceData, MaterialData, SceneData, ShapeData

    def feat(zero):
        sc = SceneData()
        sc.cameras.append(CameraData(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 5], np.float32), aspect=np.float32(1.0)))
        sc.materials.append(MaterialData(emission=np.ones(3, np.float32), color=np.full(3, 0.5, np.float32)))
        sc.shapes.append(ShapeData(positions=np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float32),
                                   triangles=np.array([[0, 1, 2]], np.int32)))
        frame = np.array([1, zero, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
        sc.instances.append(InstanceData(frame=frame, shape=0, material=0))
        sa = abi.SceneABI(sc)
        bvh, lights = trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib)
        params = make_params(abi, resolution=16, samples=1)
        buf = C.create_string_buffer(1 << 14)
        abi.check(lib, lib.jt_debug_layout_digest(sa.ref, bvh.ref, lights.ref, C.byref(params), buf, len(buf)))
        line = next(l for l in buf.value.decode().splitlines() if l.startswith("scalars"))
        return int(dict(t.split("=") for t in line.split()[1:])["feat"])

    assert feat(0.0) == 0
    assert feat(-0.0) == 128
