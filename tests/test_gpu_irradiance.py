"""jt_irradiance and jt_hemisphere_rays on the GPU (csrc/jt_radiance.hip): cosine-weighted gathers at
the caller's points against the oracle's sample_hemisphere_cos bit for bit, against jt_radiance on
the same rays bit for bit, against themselves, and against a scene whose answer is known in closed
form.

Images are 67 x 45 (tests/surface_ref.py: the last wave of a launch is partial). A case's points are
the position and normal of gbuffer(-1) at the pixels that hit, misses dropped; every case leaves at
least 1000. The deep scene (tests/scenes_ref.py, lit as tests/test_gpu_radiance.py lights it) covers
199 pixels from its own camera, so `deep_lit` looks at its dense end from (0.15, 0.12, 0.5) through a
0.1 lens instead (about 1950 pixels by the oracle's queries): the scene, and the overflow stack it is
there for, are unchanged.

1. hemisphere_rays: origins have the positions' bits, directions are slots 13..15 of the oracle's
   "parts" probe (sample_hemisphere_cos of the normal and the sample's first two draws) in every bit.
2. irradiance(points, s, s + 1) is radiance(hemisphere_rays(points, s), s, s + 1) in every bit.
3. A range is the float32 fold of its one-sample calls.
4. Partition and grid independence, once across refills.
5. The physics: under a constant environment of radiance L a black square of half-width 1 at height
   1 hides the share F = 4 / (pi sqrt 2) atan(1 / sqrt 2) of the cosine-weighted hemisphere at the
   origin, so rgb = L (1 - F) and, with the environment hidden, alpha = F, within 5 standard errors
   of 65536 samples that are each 0 or L. tests/test_irradiance_host.py shows on the CPU, from the
   oracle's directions, that the seed used lies inside both bounds.
6. The context is untouched. 7. The device variants give the host variants' bits."""
import copy
import ctypes as C

import numpy as np
import pytest

import irradiance_ref as IR
import scenes_ref as SR
import surface_ref as R
from conftest import make_params

pytestmark = pytest.mark.gpu

W, H, N = R.W, R.H, R.W * R.H
F32 = np.float32
SEED = 0x5EED
ALL = ("reference", "near", "wide")
CASES = [("cornell", ALL, {}), ("naive", ("near",), {}), ("features1", ("near",), {}), ("materials4", ("near",), {}),
         ("deep_lit", ("wide",), {}), ("cornell", ("near",), {"test_lds_ring": 2})]
RUNS = [pytest.param(name, order, opts, id=f"{name}-{order}" + ("-ring2" if opts else ""))
        for name, orders, opts in CASES for order in orders]
SAMPLES = (0, 7)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def scene_of(name):
    if name == "deep_lit":
        sc = copy.deepcopy(SR.deep_scene())
        sc.materials[0].emission = np.array([2.0, 1.5, 1.0], F32)
        sc.cameras[0].frame = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.15, 0.12, 0.5], F32)
        sc.cameras[0].lens = F32(0.1)
        return sc, {}, {}
    return R.case(name)


class Run:
    """One (case, order, options): its points, and per (sample, stream_base) the rays and the
    one-sample results, computed once on one context and shared read-only."""

    def __init__(self, name, order, opts, abi, lib, oracle):
        self.abi, self.lib, self.oracle = abi, lib, oracle
        self.scene, self.kw, o = scene_of(name)
        self.opts = {**o, **opts}
        self.sa = abi.SceneABI(self.scene)
        self.bvh, self.lights = oracle.build_bvh(self.sa), oracle.make_lights(self.sa)
        self.params = make_params(abi, width=W, height=H, traversal=order, batch=1, seed=SEED, **self.kw)
        self.cache = {}
        st = self.state()
        _, _, surf = st.gbuffer(-1)
        self.describe = st.describe()
        st.close()
        surf = surf[surf["hit"] != 0]
        self.points = np.concatenate([surf["position"], surf["normal"]], 1).astype(F32)
        self.points.setflags(write=False)

    def state(self):
        from jtrace import trace
        try:
            for k, v in self.opts.items():
                self.abi.set_option(self.lib, k, v)
            st = trace.TraceState(self.sa, self.bvh, self.lights, self.params, self.lib)
        finally:
            self.abi.set_option(self.lib, None, None)
        assert (st.width, st.height) == (W, H)
        return st

    def triple(self, s, base=0):
        """(hemisphere_rays(points, s), radiance of those rays, irradiance(points, s, s + 1))"""
        if (s, base) not in self.cache:
            st = self.state()
            rays = st.hemisphere_rays(self.points, s, stream_base=base)
            rad = st.radiance(rays, s, s + 1, stream_base=base)
            irr = st.irradiance(self.points, s, s + 1, stream_base=base)
            st.close()
            for a in (rays, rad, irr):
                a.setflags(write=False)
            self.cache[(s, base)] = (rays, rad, irr)
        return self.cache[(s, base)]


class Runs(dict):
    def __init__(self, *a):
        super().__init__()
        self.args = a

    def get_run(self, name, order, opts):
        key = (name, order, tuple(sorted(opts.items())))
        if key not in self:
            self[key] = Run(name, order, opts, *self.args)
        return self[key]


@pytest.fixture(scope="module")
def runs(gpu, abi, lib, oracle):
    return Runs(abi, lib, oracle)


def bases_of(name, order, opts):
    return (0, 5) if (name, order) == ("cornell", "near") and not opts else (0,)


# ------------------------------------------------------------------------------ 1: the rays, the oracle
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_hemisphere_rays_are_the_oracles_directions_bit_for_bit(name, order, opts, runs, oracle):
    r = runs.get_run(name, order, opts)
    n = len(r.points)
    assert n >= 1000, (name, n)
    if opts:
        assert "ring_used=2" in r.describe, r.describe
    if name == "deep_lit":
        assert "hbm_overflow=1" in r.describe and "traversal=wide" in r.describe, r.describe
    unit = r.points[:, 3:].astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    for base in bases_of(name, order, opts):
        for s in SAMPLES:
            rays, _, _ = r.triple(s, base)
            assert rays.shape == (n, 6) and rays.dtype == F32
            assert np.array_equal(bits(rays[:, :3]), bits(r.points[:, :3]))
            want = IR.oracle_directions(oracle, SEED, r.points[:, 3:], s, base)
            diff = (bits(rays[:, 3:]) != bits(want)).any(1)
            assert not diff.any(), (name, order, s, base, int(diff.sum()), rays[diff][:4], want[diff][:4])
            d = rays[:, 3:].astype(np.float64)
            length = np.linalg.norm(d, axis=1)
            print(name, order, "sample", s, "base", base, "points", n, "max |len - 1|", np.abs(length - 1).max(),
                  "min cos", (d * unit).sum(1).min())
            assert np.abs(length - 1).max() <= 2.0 ** -22
            assert ((d * unit).sum(1) >= 0).all()


# ------------------------------------------------------------------------------ 2: the kernel, jt_radiance
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_irradiance_is_radiance_of_the_hemisphere_rays_bit_for_bit(name, order, opts, runs):
    r = runs.get_run(name, order, opts)
    n = len(r.points)
    for base in bases_of(name, order, opts):
        for s in SAMPLES:
            _, rad, irr = r.triple(s, base)
            assert irr.shape == rad.shape == (n, 4) and irr.dtype == F32
            diff = (bits(irr) != bits(rad)).any(1)
            print(name, order, "sample", s, "base", base, "alpha 1 points", int((irr[:, 3] == 1).sum()), "differing", int(diff.sum()))
            assert (irr[:, 3] == 1).sum() > 100, "the gather rays see the scene"
            assert not diff.any(), (name, order, s, base, np.flatnonzero(diff)[:8], irr[diff][:4], rad[diff][:4])
    if len(bases_of(name, order, opts)) == 2:  # another stream, other draws
        assert not np.array_equal(bits(r.triple(0, 0)[0]), bits(r.triple(0, 5)[0]))


# ------------------------------------------------------------------------------ 3: the mean
@pytest.mark.parametrize("name", ["cornell", "features1"])
def test_the_mean_over_samples_is_the_float32_fold_of_one_sample_calls(name, runs):
    r = runs.get_run(name, "near", {})
    st = r.state()
    got = st.irradiance(r.points, 3, 8)
    acc = np.zeros((len(r.points), 4), F32)
    for c, s in enumerate(range(3, 8)):
        x = st.irradiance(r.points, s, s + 1)
        w = F32(1) / F32(c + 1)
        acc = acc * (F32(1) - w) + x * w
    st.close()
    assert acc.dtype == F32 and (got[:, 3] > 0).sum() > len(r.points) // 10
    diff = (bits(got) != bits(acc)).any(1)
    assert not diff.any(), (name, int(diff.sum()), got[diff][:4], acc[diff][:4])


# ------------------------------------------------------------------------------ 4: partition, grid
def test_partition_and_grid_independence(runs):
    r = runs.get_run("cornell", "near", {})
    st = r.state()
    pts = r.points
    whole = st.irradiance(pts, 0, 2)
    all_rays = st.hemisphere_rays(pts, 1)
    for n in (1, 63, 64, 65, len(pts)):
        one = st.irradiance(pts[:n], 0, 2)
        h = n // 2
        two = np.concatenate([st.irradiance(pts[:h], 0, 2), st.irradiance(pts[h:n], 0, 2, stream_base=h)])
        assert one.shape == two.shape == (n, 4)
        assert np.array_equal(bits(one), bits(two)), n
        assert np.array_equal(bits(one), bits(whole[:n])), n
        assert np.array_equal(bits(st.hemisphere_rays(pts[:n], 1)), bits(all_rays[:n])), n
    # the stream is the point's index plus stream_base, not the point's place in the call
    shifted = st.irradiance(pts[100:200], 0, 2, stream_base=100)
    assert np.array_equal(bits(shifted), bits(whole[100:200]))
    assert not np.array_equal(bits(st.irradiance(pts[100:200], 0, 2)), bits(whole[100:200]))
    st.close()


def test_partition_across_refills(runs):
    """The refill past a wave's first claim: 700 copies of the points are more than 4 x 256 x 8 x
    256 (four points for every lane of a 256-unit device's persistent grid), so lanes finish a
    point and take another and the hand-out (csrc/jt_feed.h) runs to its drain. Copy k of the
    result is the small call with stream_base k * n, in every bit."""
    COPIES = 700
    r = runs.get_run("cornell", "near", {})
    st = r.state()
    n = len(r.points)
    tiled = np.tile(r.points, (COPIES, 1))
    assert tiled.shape == (COPIES * n, 6) and COPIES * n > 4 * 256 * 8 * 256
    got = st.irradiance(tiled, 0, 1)
    assert got.shape == (COPIES * n, 4)
    for k in (0, 1, 349, 699):
        want = st.irradiance(r.points, 0, 1, stream_base=k * n)
        assert (want[:, 3] == 1).sum() > 100
        assert np.array_equal(bits(got[k * n:(k + 1) * n]), bits(want)), k
    st.close()


# ------------------------------------------------------------------------------ 5: the physics
@pytest.mark.parametrize("envhidden", [False, True], ids=["visible", "envhidden"])
def test_a_square_under_a_constant_sky(envhidden, gpu, abi, lib, oracle):
    from jtrace import trace
    sc = IR.square_scene()
    sa = abi.SceneABI(sc)
    params = make_params(abi, width=W, height=H, traversal="near", batch=1, seed=IR.SQUARE_SEED, sampler=1, envhidden=envhidden)
    st = trace.TraceState(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, lib)
    got = st.irradiance(IR.square_points(), 0, IR.SQUARE_SAMPLES).astype(np.float64)
    st.close()
    L, F, se = IR.SQUARE_L.astype(np.float64), IR.SQUARE_F, IR.SQUARE_SE
    rgb, alpha = got[:, :3].mean(0), got[:, 3].mean()
    print("envhidden", envhidden, "rgb / L", rgb / L, "1 - F", 1 - F, "alpha", alpha, "F", F, "5 se", 5 * se)
    if not envhidden:
        assert (got[:, 3] == 1).all()
        assert (np.abs(rgb - L * (1 - F)) <= 5 * se * L + 1e-5 * L * (1 - F)).all(), (rgb, L * (1 - F))
    else:
        assert (got[:, :3] == 0).all()
        assert abs(alpha - F) <= 5 * se, (alpha, F)


# ------------------------------------------------------------------------------ 6: the context
def test_the_context_is_untouched(runs):
    r = runs.get_run("cornell", "near", {})
    a, b = r.state(), r.state()
    out = []
    for st in (a, b):
        st.trace_range(0, 4)
        st.get_image()  # flushes: four samples traced
        st.trace_range(4, 5)  # queued
        assert st.samples == 5
        if st is a:
            irr = st.irradiance(r.points, 0, 3)
            rays = st.hemisphere_rays(r.points, 2)
            assert (irr[:, 3] > 0).any() and rays.shape == (len(r.points), 6) and st.samples == 5
        image = st.get_image()
        albedo, normal, hits = st.get_aovs()
        cnt = st.counters()
        cnt.pop("kernel_ms")
        out.append((image, albedo, normal, hits, cnt))
        st.close()
    for x, y in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(out[0][3], out[1][3]) and out[0][4] == out[1][4] and out[0][4]["paths"] == 5 * N, out[0][4]


# ------------------------------------------------------------------------------ 7: the device variants
def test_device_variants_give_the_host_bits_and_reject_misaligned_outputs(runs, abi, lib):
    import torch
    r = runs.get_run("features1", "near", {})
    st = r.state()
    n = len(r.points)
    want = st.irradiance(r.points, 1, 3, stream_base=5)
    want_rays = st.hemisphere_rays(r.points, 1, stream_base=5)
    dev = torch.device("cuda", int(r.params.device))
    d_points = torch.from_numpy(np.array(r.points)).to(dev)
    got = st.irradiance(d_points, 1, 3, stream_base=5)
    got_rays = st.hemisphere_rays(d_points, 1, stream_base=5)
    for t, shape in ((got, (n, 4)), (got_rays, (n, 6))):
        assert isinstance(t, torch.Tensor) and t.device == d_points.device and tuple(t.shape) == shape
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(bits(got_rays.cpu().numpy()), bits(want_rays))
    buf = torch.zeros(n * 6 + 4, dtype=torch.float32, device=dev)
    status = lib.jt_irradiance_device(st.handle, n, d_points.data_ptr(), 0, 0, 1, buf.data_ptr() + 4)
    assert status == -1 and "d_rgba" in lib.jt_last_error().decode() and "aligned" in lib.jt_last_error().decode()
    status = lib.jt_hemisphere_rays_device(st.handle, n, d_points.data_ptr(), 0, 0, buf.data_ptr() + 4)
    assert status == -1 and "d_rays" in lib.jt_last_error().decode() and "aligned" in lib.jt_last_error().decode()
    assert not buf.any().item()
    st.close()
