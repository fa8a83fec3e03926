"""sincos_unit and the baked matte sample's local draw (csrc/jt_device.h, csrc/jt_bsdf.h matte_local)
on the device, over their whole input set, and the baking kernels against the kernels that keep
sample_hemisphere_cos.

tests/probe/jt_unit_probe.hip compiles the product's headers with the product's flags
(libjt_unit_probe.so, built by tests/probe/unit_probe.mk). rn.x and rn.y are rand1f values, k * 2^-24:
  * sincos_unit(u) over all 2^24 u is float32(sin / cos(float64 phi)), phi = (2 pif) u, and is
    jl_sincos(phi) from the existing probe, bit for bit, no exception;
  * the local sample (r cos phi, r sin phi, z) in the new form (sincos_unit, sqrt_fast without its
    domain test) is bit-identical to sample_hemisphere_cos's lines: every rn.y at four rn.x, every
    rn.x at four rn.y (compared on the device), and a strided subset brought back and also checked
    against numpy's correctly rounded float32 square roots;
  * cornellbox at 44 x 36, 16 spp, both samplers: the baking kernel against HBM mode (lds_scene=0)
    and the general kernel (features=all), which keep sample_hemisphere_cos and sample_disk — image,
    AOVs, hits and counters equal. Once with the scene's pinhole camera and once with an aperture,
    where the lens sample's sine and cosine are used (sample_disk_unit).
"""
import copy
import ctypes as C

import numpy as np
import pytest

import primitives_ref as R
from conftest import make_params
from primitives_ref import F32

pytestmark = pytest.mark.gpu

UNIT_LIB = R.ROOT / "julia-raytracer_amd" / "build" / "libjt_unit_probe.so"
EDGES = (0.0, 2.0 ** -24, None, float(R.ONE_MINUS))  # None: 0.5 on the azimuth axis, 0.25 on the other
W, H, SPP = 44, 36, 16
COUNTERS = ("paths", "shades", "nodes", "instances", "prims", "rays", "light_queries")


class UnitProbe:
    def __init__(self):
        if not UNIT_LIB.exists():  # an error, not a skip
            raise FileNotFoundError(f"{UNIT_LIB} is missing: build it with make -C tests/probe -f unit_probe.mk unit (build() does)")
        self.lib = C.CDLL(str(UNIT_LIB))
        f32p = C.POINTER(C.c_float)
        self.lib.ju_sincos.argtypes = [C.c_int64, f32p, f32p]
        self.lib.ju_local.argtypes = [C.c_int64, f32p, f32p]
        self.lib.ju_local_sweep.argtypes = [C.c_int, C.c_float, C.POINTER(C.c_uint32)]

    def _run(self, fn, x, nin, nout):
        x = np.ascontiguousarray(x, F32).reshape(-1, nin)
        out = np.empty((len(x), nout), F32)
        f32p = C.POINTER(C.c_float)
        st = fn(len(x), x.ctypes.data_as(f32p), out.ctypes.data_as(f32p))
        if st != 0:
            raise RuntimeError(f"unit probe: HIP status {st}")
        return out

    def sincos(self, u):
        return self._run(self.lib.ju_sincos, u, 1, 2)

    def local(self, rn):
        return self._run(self.lib.ju_local, rn, 2, 6)

    def sweep(self, axis, fixed):
        res = np.zeros(10, np.uint32)
        st = self.lib.ju_local_sweep(axis, fixed, res.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st != 0:
            raise RuntimeError(f"unit probe sweep: HIP status {st}")
        return int(res[0]), int(res[1]), res[2:2 + min(int(res[1]), 8)].tolist()


@pytest.fixture(scope="module")
def unit(gpu):
    return UnitProbe()


def test_product_ships_the_new_form(unit):
    """The library under test was compiled with sincos_unit in the matte sample (JT_SINCOS_UNIT >= 1)."""
    assert unit.lib.ju_sincos_unit_level() >= 1


def test_sincos_unit_every_azimuth(unit, gpu):
    out = unit.sincos(R.rand_u())
    phi = R.phi_all().astype(np.float64)
    ref = np.stack([np.sin(phi).astype(F32), np.cos(phi).astype(F32)], 1)
    bad = R.mismatches(out, ref)
    print(f"sincos_unit against float64: n={len(out)} mismatches={len(bad)}")
    assert len(bad) == 0, (R.rand_u()[bad[:4]], out[bad[:4]], ref[bad[:4]])
    old = R.Probe().run("sincos", R.phi_all())[:, :2]
    bad = R.mismatches(out, old)
    print(f"sincos_unit against jl_sincos: mismatches={len(bad)}")
    assert len(bad) == 0, (R.rand_u()[bad[:4]], out[bad[:4]], old[bad[:4]])


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("edge", range(4))
def test_local_sample_new_form_is_the_old(unit, axis, edge):
    """axis 0: every rn.x at one rn.y; axis 1: every rn.y at one rn.x."""
    fixed = EDGES[edge] if EDGES[edge] is not None else (0.25 if axis == 0 else 0.5)
    n, bad, first = unit.sweep(axis, fixed)
    print(f"local sample, axis {axis}, fixed {fixed!r}: lanes={n} differing={bad}")
    assert n == 1 << 24
    assert bad == 0, first


def test_local_sample_values(unit):
    """A subset of the sweeps' inputs brought back to the host: the two forms' floats, equal, z and r
    numpy's correctly rounded float32 roots and the azimuth terms r times the float64 references."""
    k = np.concatenate([np.arange(0, 1 << 24, 257), [1, 2, (1 << 24) - 1, 1 << 23, 1 << 22, 3 << 22]])
    u = (k.astype(np.float64) * 2.0 ** -24).astype(F32)
    rows = [np.stack([u, np.full_like(u, f)], 1) for f in (0.0, 2.0 ** -24, 0.25, float(R.ONE_MINUS))]
    rows += [np.stack([np.full_like(u, f), u], 1) for f in (0.0, 2.0 ** -24, 0.5, float(R.ONE_MINUS))]
    rn = np.concatenate(rows).astype(F32)
    out = unit.local(rn)
    assert len(R.mismatches(out[:, :3], out[:, 3:])) == 0
    z = np.sqrt(rn[:, 1])
    r = np.sqrt(F32(1) - z * z)
    phi = (R.TWO_PIF * rn[:, 0]).astype(np.float64)
    ref = np.stack([r * np.cos(phi).astype(F32), r * np.sin(phi).astype(F32), z], 1)
    bad = R.mismatches(out[:, 3:], ref)
    print(f"local sample values: n={len(rn)} mismatches={len(bad)}")
    assert len(bad) == 0, (rn[bad[:4]], out[bad[:4]], ref[bad[:4]])


_scenes = {}


def _scene(abi, cornell, aperture):
    if aperture not in _scenes:
        sc = copy.deepcopy(cornell)
        sc.cameras[0].aspect = F32(W / H)
        sc.cameras[0].aperture = F32(aperture)
        _scenes[aperture] = abi.SceneABI(sc)
    return _scenes[aperture]


@pytest.mark.parametrize("aperture", [0.0, 0.05])
@pytest.mark.parametrize("sampler", [1, 2])
def test_baking_kernel_equals_the_kernels_that_keep_the_old_sample(gpu, abi, lib, options, cornell, sampler, aperture):
    from jtrace import trace
    sa = _scene(abi, cornell, aperture)
    params = make_params(abi, resolution=W, samples=SPP, batch=4, sampler=sampler)
    bvh, lights = trace.make_scene_bvh(sa, False, lib), trace.make_trace_lights(sa, lib)
    out = {}
    for mode, opt in (("lds", None), ("hbm", ("lds_scene", "0")), ("all", ("features", "all"))):
        for key in ("lds_scene", "features"):
            options(key, None)
        if opt:
            options(*opt)
        st = trace.make_trace_state(sa, bvh, lights, params, lib)
        st.trace_range(0, SPP)
        out[mode] = (st.get_image(),) + st.get_aovs() + (st.counters(), st.describe())
        st.close()
    lds = out["lds"]
    assert lds[0].shape[:2] == (H, W)
    assert f"kernel=trace_kernel_lds<{sampler},16,false,1,8192,false> mode=lds " in lds[5], lds[5]
    assert " mode=hbm " in out["hbm"][5], out["hbm"][5]
    assert f"<{sampler},16,false,1,255,false> mode=" in out["all"][5], out["all"][5]  # the general kernel, either mode
    assert lds[0][..., :3].mean() > 0 and lds[4]["shades"] > lds[3].sum() > 0
    for mode in ("hbm", "all"):
        g = out[mode]
        for k, what in enumerate(("image", "albedo", "normal", "hits")):
            assert np.array_equal(lds[k], g[k]), (mode, what)
        for key in COUNTERS:
            assert g[4][key] == lds[4][key], (mode, key, g[4][key], lds[4][key])
