"""jt_probe_sh, jt_sphere_rays (include/jtrace.h), jtrace/sh.py and the grid of `python -m
jtrace.probes`, the part that needs no GPU: csrc/jt_sh.h's basis against jtrace.sh.sh_basis bit for
bit through the stand-alone program tests/sh_check.cpp (built with the host compiler under the
address and undefined-behaviour sanitizers), the basis' orthonormality and the irradiance formula by
quadrature, the four exports and their prototypes, the argument errors in the header's order before
the context is looked at, the probe grid, and the seed of the analytic scene of
tests/test_gpu_probe_sh.py, whose means the oracle's draws predict on the CPU."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import irradiance_ref as IR
import sh_ref as SH
from conftest import CORNELL, ROOT

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_probe_sh", "jt_probe_sh_device", "jt_sphere_rays", "jt_sphere_rays_device")
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def unit_vectors():
    """A few thousand float32 unit vectors: random ones, the axes, and directions with one or two
    zero components (of either sign of zero)."""
    rng = np.random.default_rng(9)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    planar = d[:300].copy()
    planar[np.arange(300), np.arange(300) % 3] = 0.0
    planar /= np.linalg.norm(planar, axis=1, keepdims=True)
    negz = planar[:60].copy()
    negz[negz == 0] = -0.0
    return np.concatenate([d, axes, planar, negz]).astype(F32)


def test_the_headers_basis_is_the_python_basis_bit_for_bit(tmp_path):
    from jtrace.sh import sh_basis
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sh_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "sh_check.cpp")], check=True)
    d = unit_vectors()
    assert len(d) >= 4000 and (d == 0).any(1).sum() >= 300
    (tmp_path / "in.bin").write_bytes(d.tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout and f"{len(d)} directions" in run.stdout
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), F32).reshape(len(d), 9)
    want = sh_basis(d)
    assert want.dtype == F32 and want.shape == (len(d), 9)
    diff = (bits(got) != bits(want)).any(1)
    assert not diff.any(), (int(diff.sum()), d[diff][:4], got[diff][:4], want[diff][:4])
    # one direction, and a leading shape, give the same values
    assert np.array_equal(bits(sh_basis(d[7])), bits(want[7])) and np.array_equal(bits(sh_basis(d.reshape(2, -1, 3))), bits(want).reshape(2, -1, 9))


def _latlong(nt=256, nphi=512):
    """Midpoint lat-long quadrature: directions (nt * nphi, 3) and solid-angle weights."""
    t = (np.arange(nt) + 0.5) / nt * np.pi
    p = (np.arange(nphi) + 0.5) / nphi * 2 * np.pi
    tt, pp = np.meshgrid(t, p, indexing="ij")
    d = np.stack([np.sin(tt) * np.cos(pp), np.sin(tt) * np.sin(pp), np.cos(tt)], -1).reshape(-1, 3)
    w = (np.sin(tt) * (np.pi / nt) * (2 * np.pi / nphi)).ravel()
    return d, w


def test_the_basis_is_orthonormal_over_the_sphere():
    from jtrace.sh import sh_basis
    d, w = _latlong()
    assert abs(w.sum() - 4 * np.pi) <= 1e-4
    Y = sh_basis(d).astype(np.float64)
    # the float64 mean of Y_j Y_k under the uniform measure, times 4 pi
    gram = (Y[:, :, None] * Y[:, None, :] * w[:, None, None]).sum(0) / w.sum() * 4 * np.pi
    print(np.abs(gram - np.eye(9)).max())
    assert np.abs(gram - np.eye(9)).max() <= 1e-4, gram


def test_sh_irradiance_of_a_constant_and_of_a_linear_field():
    from jtrace.sh import C0, sh_basis, sh_irradiance, sh_radiance
    rng = np.random.default_rng(4)
    normals = rng.normal(size=(50, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    # constant radiance L: what jt_probe_sh returns is the mean of L Y_k, so sh_0 = L c0, the rest 0
    L = np.array([2.0, 1.0, 0.5])
    sh = np.zeros((9, 4), F32)
    sh[0, :3], sh[0, 3] = L * float(C0), C0
    assert sh_radiance(sh).shape == (9, 3) and sh_radiance(sh).dtype == F32
    assert np.allclose(sh_radiance(sh)[0], 4 * np.pi * L * float(C0), rtol=1e-6)
    E = sh_irradiance(sh, normals)
    assert E.shape == (50, 3)
    assert np.abs(E / (np.pi * L) - 1).max() <= 1e-4, E[:3]
    # L(omega) = a . omega projected by quadrature (the mean over the uniform measure): E(n) = 2 pi / 3 a . n
    a = np.array([0.3, -1.1, 0.7])
    d, w = _latlong()
    Y = sh_basis(d).astype(np.float64)
    field = d @ a
    sh = np.zeros((9, 4), F32)
    sh[:, :3] = ((Y * (field * w)[:, None]).sum(0) / w.sum())[:, None]
    E = sh_irradiance(sh, normals)
    want = 2 * np.pi / 3 * (normals @ a)
    assert np.abs(E - want[:, None]).max() <= 1e-4 * np.abs(want).max(), (E[:3], want[:3])
    # probes (n, 9, 4) with one normal each
    many = np.broadcast_to(sh, (50, 9, 4))
    assert np.allclose(sh_irradiance(many, normals), E)


def test_the_four_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5 and "#define JT_ABI_VERSION 5" in HEADER.read_text()
    host, dev = [C.c_void_p, C.c_int64, abi.f32p, C.c_int64], [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    assert lib.jt_probe_sh.argtypes == host + [C.c_int32, C.c_int32, abi.f32p]
    assert lib.jt_probe_sh_device.argtypes == dev + [C.c_int32, C.c_int32, C.c_void_p]
    assert lib.jt_sphere_rays.argtypes == host + [C.c_int32, abi.f32p]
    assert lib.jt_sphere_rays_device.argtypes == dev + [C.c_int32, C.c_void_p]
    for name in NAMES:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
        kinds = [re.sub(r"\s+\w+$", "", a.strip()).replace("const ", "") for a in decl.split(",")]
        p = "void*" if name.endswith("_device") else "float*"
        samples = ["int32_t", "int32_t"] if "probe" in name else ["int32_t"]
        assert kinds == ["jt_ctx*", "int64_t", p, "int64_t"] + samples + [p], (name, kinds)
    # the header states the -0 rule and the contract
    doc = HEADER.read_text()
    assert "product of -0" in doc and "jt_radiance(jt_sphere_rays(points, base, s), base, s, s + 1)" in doc
    # the test-only chunk option is a known option
    assert lib.jt_set_option(b"test_probe_chunk", b"1000") == 0 and lib.jt_set_option(b"test_probe_chunk", None) == 0


def test_argument_errors_in_order_need_no_device(abi, lib):
    """Every JT_ERR_INVALID of the header's list names its argument and is reported before the
    context is looked at: the handle below is no context and is never read. Each call breaks one
    rule and, to show the order, every later rule of the list too. n == 0 with valid arguments is
    JT_OK, and nothing is written."""
    pts = np.zeros((4, 3), F32)
    out = np.full((4, 36), 7.0, F32)
    pp, op = pts.ctypes.data_as(abi.f32p), out.ctypes.data_as(abi.f32p)
    fake, dev = C.c_void_p(0x10), C.c_void_p(0x1000)
    odd16, odd8 = C.c_void_p(0x1008), C.c_void_p(0x1004)  # off 16 bytes (though on 8), off 8 bytes

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    def probe(ctx=fake, n=4, p=pp, base=0, s0=0, s1=1, o=op):
        return err(lib.jt_probe_sh(ctx, n, p, base, s0, s1, o))

    def probe_dev(ctx=fake, n=4, p=dev, base=0, s0=0, s1=1, o=dev):
        return err(lib.jt_probe_sh_device(ctx, n, p, base, s0, s1, o))

    def sphere(ctx=fake, n=4, p=pp, base=0, s=0, o=op):
        return err(lib.jt_sphere_rays(ctx, n, p, base, s, o))

    def sphere_dev(ctx=fake, n=4, p=dev, base=0, s=0, o=dev):
        return err(lib.jt_sphere_rays_device(ctx, n, p, base, s, o))

    late = dict(n=-1, base=-1, s0=-1, s1=-1)  # every later rule broken too
    late1 = dict(n=-1, base=-1, s=-1)
    assert "ctx" in probe(ctx=None, p=None, o=None, **late) and "ctx" in probe_dev(ctx=None, p=None, o=odd16, **late)
    assert "ctx" in sphere(ctx=None, p=None, o=None, **late1) and "ctx" in sphere_dev(ctx=None, p=None, o=odd8, **late1)
    assert re.match(r"points\b", probe(p=None, o=None, **late)) and re.match(r"d_points\b", probe_dev(p=None, o=None, **late))
    assert re.match(r"points\b", sphere(p=None, o=None, **late1)) and re.match(r"d_points\b", sphere_dev(p=None, o=None, **late1))
    assert re.match(r"sh\b", probe(o=None, **late)) and re.match(r"d_sh\b", probe_dev(o=None, **late))
    assert re.match(r"rays\b", sphere(o=None, **late1)) and re.match(r"d_rays\b", sphere_dev(o=None, **late1))
    for call, o in ((probe, op), (probe_dev, odd16)):
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", call(n=n, base=-1, s0=-1, s1=-1, o=o)), n
        assert re.match(r"stream_base must\b", call(base=-1, s0=-1, s1=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(base=2**31 - 3, s0=-1, s1=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(n=2**30, base=2**30 + 1, s0=-1, s1=-1, o=o))
        assert re.match(r"sample_begin\b", call(s0=-1, s1=-5, o=o))
        assert re.match(r"sample_end must\b", call(s0=3, s1=3, o=o)) and re.match(r"sample_end must\b", call(s0=3, s1=2, o=o))
        assert "2^24" in call(s0=5, s1=5 + 2**24 + 1, o=o)
    for call, o in ((sphere, op), (sphere_dev, odd8)):
        for n in (-1, -2**40, 2**30 + 1):
            assert re.match(r"n must\b", call(n=n, base=-1, s=-1, o=o)), n
        assert re.match(r"stream_base must\b", call(base=-1, s=-1, o=o))
        assert re.match(r"stream_base \+ n\b", call(base=2**31 - 3, s=-1, o=o))
        assert re.match(r"sample must\b", call(s=-1, o=o)) and re.match(r"sample must\b", call(s=-2**31, o=o))
    assert re.match(r"d_sh\b.*aligned to 16", probe_dev(o=odd16)) and re.match(r"d_sh\b.*aligned", probe_dev(n=0, o=odd8))
    assert re.match(r"d_rays\b.*aligned to 8", sphere_dev(o=odd8)) and re.match(r"d_rays\b.*aligned", sphere_dev(n=0, o=odd8))
    # a ray record needs 8 bytes only: what is off 16 but on 8 passes the checks (n == 0: no device work)
    assert lib.jt_sphere_rays_device(fake, 0, dev, 0, 0, odd16) == 0
    # the largest arguments that break no rule reach the n == 0 return: JT_OK, no device work
    assert lib.jt_probe_sh(fake, 0, pp, 2**31, 2**31 - 2, 2**31 - 1, op) == 0
    assert lib.jt_probe_sh(fake, 0, pp, 0, 0, 2**24, op) == 0
    assert lib.jt_probe_sh_device(fake, 0, dev, 0, 0, 1, dev) == 0
    assert lib.jt_sphere_rays(fake, 0, pp, 2**31, 2**31 - 1, op) == 0
    assert lib.jt_sphere_rays_device(fake, 0, dev, 0, 0, dev) == 0
    assert (out == 7.0).all() and (pts == 0).all()


def test_python_wrappers_turn_away_other_shapes():
    from jtrace.trace import _host_points
    assert _host_points(np.zeros((5, 3))).dtype == F32
    for shape in ((5, 6), (3,), (5, 3, 1)):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            _host_points(np.zeros(shape, F32))


# ------------------------------------------------------------------------------ the probes CLI's grid
def test_the_probe_grid_has_cell_centres_x_fastest():
    from jtrace.probes import _bounds, _grid, grid_points
    bounds = np.array([[-1.0, 0.0, 2.0], [1.0, 3.0, 6.0]])
    p = grid_points((4, 3, 2), bounds)
    assert p.shape == (24, 3) and p.dtype == F32
    xs, ys, zs = [-0.75, -0.25, 0.25, 0.75], [0.5, 1.5, 2.5], [3.0, 5.0]
    k = 0
    for z in zs:
        for y in ys:
            for x in xs:  # x fastest
                assert np.allclose(p[k], (x, y, z)), (k, p[k])
                k += 1
    assert np.allclose(grid_points((1, 1, 1), bounds)[0], bounds.mean(0))
    assert _grid("3x2x3") == (3, 2, 3) and _grid("3X2x1") == (3, 2, 1)
    assert np.array_equal(_bounds("0,1,2,3,4,5.5"), [[0, 1, 2], [3, 4, 5.5]])
    import argparse
    for bad in ("3x2", "3x2x0", "axbxc", "1x2x3x4"):
        with pytest.raises(argparse.ArgumentTypeError):
            _grid(bad)
    for bad in ("0,1,2", "a,b,c,d,e,f"):
        with pytest.raises(argparse.ArgumentTypeError):
            _bounds(bad)


def test_the_default_bounds_are_the_instances_transformed_positions(cornell):
    from jtrace.probes import grid_points, scene_bounds
    # the square scene: one quad at y = 1, identity frame
    b = scene_bounds(IR.square_scene())
    assert np.array_equal(b, [[-1, 1, -1], [1, 1, 1]])
    p = grid_points((2, 1, 2), b)
    assert np.array_equal(p, np.array([[-0.5, 1, -0.5], [0.5, 1, -0.5], [-0.5, 1, 0.5], [0.5, 1, 0.5]], F32))
    # a frame moves the box: twice as wide along x, turned a quarter about y (x -> -z, z -> x), lifted by 3
    sc = IR.square_scene()
    sc.instances[0].frame = np.array([0, 0, -2, 0, 1, 0, 1, 0, 0, 0, 3, 0], F32)
    assert np.allclose(scene_bounds(sc), [[-1, 4, -2], [1, 4, 2]])
    # cornellbox: every instance has the identity frame, so the box is that of all positions
    pos = np.concatenate([np.asarray(s.positions, np.float64) for s in cornell.shapes])
    assert all(np.allclose(i.frame, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]) for i in cornell.instances)
    assert np.array_equal(scene_bounds(cornell), [pos.min(0), pos.max(0)])


def test_the_probes_cli_rejects_before_a_context_is_made(tmp_path):
    """The rejections that need no device, through the module's own entry (no child process)."""
    from jtrace import probes
    bad = tmp_path / "bad.npy"
    np.save(bad, np.zeros((5, 6), F32))
    out = tmp_path / "p.npz"
    for args, msg in ((["--points", str(bad)], r"expected shape \(n, 3\)"),
                      (["--points", str(bad), "--grid", "2x2x2"], "not both"),
                      ([], "--points or --grid"),
                      (["--points", str(bad), "--bounds", "0,0,0,1,1,1"], "--bounds needs --grid"),
                      (["--grid", "2x2x2", "--samples", "0"], "--samples")):
        with pytest.raises(SystemExit, match=msg):
            probes.main(["--scene", CORNELL, "--output", str(out), *args])
    with pytest.raises(SystemExit, match="expected .npz"):
        probes.main(["--scene", CORNELL, "--grid", "2x2x2", "--output", str(tmp_path / "p.npy")])
    assert not out.exists()


# ------------------------------------------------------------------------------ the analytic scene's seed
def test_the_square_scenes_closed_forms():
    keep, cover = SH.square_expected()
    print("sh_k.rgb / L", keep, "sh_k.a under envhidden", cover)
    assert abs(keep[0] - SH.C0 * 5 / 6) <= 1e-6 and abs(cover[0] - SH.C0 / 6) <= 1e-6
    assert abs(keep[1] + SH.C1 * IR.SQUARE_F / 4) <= 1e-6
    assert np.abs(keep[[2, 3, 4, 5, 7]]).max() <= 1e-12
    # the figures the feature's issue states: 0.23508, -0.06769, +0.028981, +0.050196
    assert abs(keep[0] - 0.23508) <= 1e-5 and abs(keep[1] + 0.06769) <= 1e-5
    assert abs(keep[6] - 0.028981) <= 1e-6 and abs(keep[8] - 0.050196) <= 1e-6


def test_the_square_scenes_seed_lies_inside_the_bounds(oracle):
    """tests/test_gpu_probe_sh.py number 5, decided before any GPU runs: the oracle's first pairs of
    the 64 x 1024 samples, the float64 sphere draw and a float64 ray-square test give the means the
    kernel should find; every one is within 5 standard errors of its closed form."""
    keep, cover = SH.square_expected()
    seen, covered = SH.square_prediction(oracle, IR.SQUARE_SEED)
    print("visible: predicted", seen, "expected", keep, "in standard errors", (seen - keep) / SH.SQUARE_SH_SE)
    print("envhidden alpha: predicted", covered, "expected", cover, "in standard errors", (covered - cover) / SH.SQUARE_SH_SE)
    assert np.abs(seen - keep).max() <= 5 * SH.SQUARE_SH_SE
    assert np.abs(covered - cover).max() <= 5 * SH.SQUARE_SH_SE
