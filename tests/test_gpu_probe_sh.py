"""jt_probe_sh and jt_sphere_rays on the GPU (csrc/jt_radiance.hip, csrc/jt_sh.h): spherical-harmonic
radiance probes against a float64 restatement of the sphere draw, against jt_radiance on the same
rays and jtrace.sh's basis bit for bit, against themselves, and against a scene whose answer is known
in closed form.

Images are 67 x 45 (tests/surface_ref.py: the last wave of a launch is partial). A case's points are
the positions of gbuffer(-1) at the pixels that hit, misses dropped; every case leaves at least 1000.
The cases are those of tests/test_gpu_irradiance.py (the deep scene lit and looked at from its dense
end, as there). A probe on a surface sees the scene on one side and, on the other, the inside of the
surface or nothing: rays that find nothing in a scene without an environment have the target
(0, 0, 0, 0), which is what exercises the -0 rule.

1. sphere_rays: origins have the positions' bits; directions equal the float64 restatement
   (tests/sh_ref.py) on the oracle's first pairs within 4e-6 per component: phi <= 2 pi has the
   float32 spacing 4.8e-7, the sine and cosine of it inherit that, and the products with r, the
   three roundings of z and r and the normalisation add a handful of 6e-8 each. Unit within 2^-22;
   over all points the mean of d is 0 and the mean of d.z^2 is 1/3 within 5 standard errors.
2. probe_sh(p, s, s + 1) is the fold step 0 * 0 + (radiance(sphere_rays(p, s), s, s + 1) * Y) * 1
   with Y = jtrace.sh.sh_basis of those directions, in every bit of all 36 floats.
3. A range is the float32 fold of its one-sample results.
4. Partition and grid independence, once across refills.
5. The physics: at the origin under a constant environment L, below the black square that is the
   face y = 1 of the cube about it (tests/sh_ref.py states the closed forms), within 5 standard
   errors. tests/test_sh_host.py shows on the CPU that the seed used lies inside the bounds.
6. The context is untouched. 7. The device variants give the host variants' bits; the host variant
   over a chunk boundary (option test_probe_chunk) gives the bits of one device call."""
import copy

import numpy as np
import pytest

import irradiance_ref as IR
import scenes_ref as SR
import sh_ref as SH
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
    if name == "deep_lit":  # as tests/test_gpu_irradiance.py lights and frames it
        sc = copy.deepcopy(SR.deep_scene())
        sc.materials[0].emission = np.array([2.0, 1.5, 1.0], F32)
        sc.cameras[0].frame = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.15, 0.12, 0.5], F32)
        sc.cameras[0].lens = F32(0.1)
        return sc, {}, {}
    return R.case(name)


def fold_step(acc, rad, rays, count):
    from jtrace.sh import sh_basis, sh_fold
    return sh_fold(acc, rad, sh_basis(rays[:, 3:]), count)


class Run:
    """One (case, order, options): its points, and per (sample, stream_base) the rays, their radiance
    and the one-sample probes, computed once on one context and shared read-only."""

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
        self.points = np.ascontiguousarray(surf[surf["hit"] != 0]["position"], F32)
        self.points.setflags(write=False)

    def state(self, **more):
        from jtrace import trace
        try:
            for k, v in {**self.opts, **more}.items():
                self.abi.set_option(self.lib, k, v)
            st = trace.TraceState(self.sa, self.bvh, self.lights, self.params, self.lib)
        finally:
            self.abi.set_option(self.lib, None, None)
        assert (st.width, st.height) == (W, H)
        return st

    def triple(self, s, base=0):
        """(sphere_rays(points, s), radiance of those rays, probe_sh(points, s, s + 1))"""
        if (s, base) not in self.cache:
            st = self.state()
            rays = st.sphere_rays(self.points, s, stream_base=base)
            rad = st.radiance(rays, s, s + 1, stream_base=base)
            sh = st.probe_sh(self.points, s, s + 1, stream_base=base)
            st.close()
            for a in (rays, rad, sh):
                a.setflags(write=False)
            self.cache[(s, base)] = (rays, rad, sh)
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


# ------------------------------------------------------------------------------ 1: the rays
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_sphere_rays_are_the_float64_draw_on_the_oracles_pairs(name, order, opts, runs, oracle):
    r = runs.get_run(name, order, opts)
    n = len(r.points)
    assert n >= 1000, (name, n)
    if opts:
        assert "ring_used=2" in r.describe, r.describe
    if name == "deep_lit":
        assert "hbm_overflow=1" in r.describe and "traversal=wide" in r.describe, r.describe
    for base in bases_of(name, order, opts):
        for s in SAMPLES:
            rays, _, _ = r.triple(s, base)
            assert rays.shape == (n, 6) and rays.dtype == F32
            assert np.array_equal(bits(rays[:, :3]), bits(r.points))
            want = SH.sphere_directions64(IR.first_pairs(oracle, SEED, np.arange(n) + base, s))
            d = rays[:, 3:].astype(np.float64)
            length = np.linalg.norm(d, axis=1)
            se = 1 / np.sqrt(3 * n)  # a component of a uniform direction has the variance 1/3
            se_z2 = np.sqrt(4 / 45 / n)  # z^2: mean 1/3, second moment 1/5
            print(name, order, "sample", s, "base", base, "points", n, "worst difference", np.abs(d - want).max(),
                  "max |len - 1|", np.abs(length - 1).max(), "mean d / se", d.mean(0) / se, "mean z^2", (d[:, 2] ** 2).mean())
            assert np.abs(d - want).max() <= 4e-6
            assert np.abs(length - 1).max() <= 2.0 ** -22
            assert np.abs(d.mean(0)).max() <= 5 * se
            assert abs((d[:, 2] ** 2).mean() - 1 / 3) <= 5 * se_z2


# ------------------------------------------------------------------------------ 2: one sample
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_one_sample_is_the_fold_step_of_radiance_times_the_basis_bit_for_bit(name, order, opts, runs):
    from jtrace.sh import sh_basis
    r = runs.get_run(name, order, opts)
    n = len(r.points)
    for base in bases_of(name, order, opts):
        for s in SAMPLES:
            rays, rad, sh = r.triple(s, base)
            assert sh.shape == (n, 9, 4) and sh.dtype == F32 and rad.shape == (n, 4)
            want = fold_step(np.zeros((n, 9, 4), F32), rad, rays, 0)
            assert want.dtype == F32
            diff = (bits(sh) != bits(want)).reshape(n, -1).any(1)
            Y = sh_basis(rays[:, 3:])
            # a channel of zero radiance times a negative Y_k: the bare product is -0
            minus = (rad == 0).any(1) & (Y < 0).any(1)
            print(name, order, "sample", s, "base", base, "alpha 1 points", int((rad[:, 3] == 1).sum()), "zero-target points with a negative Y",
                  int(minus.sum()), "differing", int(diff.sum()))
            assert (rad[:, 3] == 1).sum() > 100, "the rays see the scene"
            assert minus.sum() >= 1, "the -0 rule is exercised"
            bare = rad[:, None, :] * Y[:, :, None]
            assert (bits(bare[minus]) == 0x80000000).any() and not (bits(sh) == 0x80000000).any()
            assert not diff.any(), (name, order, s, base, np.flatnonzero(diff)[:8], sh[diff][:2], want[diff][:2])
    if len(bases_of(name, order, opts)) == 2:  # another stream, other draws
        assert not np.array_equal(bits(r.triple(0, 0)[0]), bits(r.triple(0, 5)[0]))


# ------------------------------------------------------------------------------ 3: the mean
@pytest.mark.parametrize("name", ["cornell", "features1"])
def test_a_range_is_the_float32_fold_of_its_one_sample_results(name, runs):
    r = runs.get_run(name, "near", {})
    st = r.state()
    got = st.probe_sh(r.points, 3, 8)
    acc = np.zeros((len(r.points), 9, 4), F32)
    for c, s in enumerate(range(3, 8)):
        x = st.probe_sh(r.points, s, s + 1)
        w = F32(1) / F32(c + 1)
        acc = acc * (F32(1) - w) + x * w
    st.close()
    assert acc.dtype == F32 and (got[:, 0, 3] > 0).sum() > len(r.points) // 10
    diff = (bits(got) != bits(acc)).reshape(len(got), -1).any(1)
    assert not diff.any(), (name, int(diff.sum()), got[diff][:2], acc[diff][:2])


# ------------------------------------------------------------------------------ 4: partition, grid
def test_partition_and_grid_independence(runs):
    r = runs.get_run("cornell", "near", {})
    st = r.state()
    pts = r.points
    whole = st.probe_sh(pts, 0, 2)
    all_rays = st.sphere_rays(pts, 1)
    for n in (1, 63, 64, 65, len(pts)):
        one = st.probe_sh(pts[:n], 0, 2)
        h = n // 2
        two = np.concatenate([st.probe_sh(pts[:h], 0, 2), st.probe_sh(pts[h:n], 0, 2, stream_base=h)])
        assert one.shape == two.shape == (n, 9, 4)
        assert np.array_equal(bits(one), bits(two)), n
        assert np.array_equal(bits(one), bits(whole[:n])), n
        assert np.array_equal(bits(st.sphere_rays(pts[:n], 1)), bits(all_rays[:n])), n
    # the stream is the point's index plus stream_base, not the point's place in the call
    shifted = st.probe_sh(pts[100:200], 0, 2, stream_base=100)
    assert np.array_equal(bits(shifted), bits(whole[100:200]))
    assert not np.array_equal(bits(st.probe_sh(pts[100:200], 0, 2)), bits(whole[100:200]))
    st.close()


def test_partition_across_refills(runs):
    """The refill past a wave's first claim, as tests/test_gpu_irradiance.py runs it: 700 copies of
    the points are more than 4 x 256 x 8 x 256 (four points for every lane of a 256-unit device's
    persistent grid), so lanes finish a probe, with its record written, and take another. Copy k
    of the result is the small call with stream_base k * n, in every bit. Two samples, so a lane
    reads its own record back once."""
    COPIES = 700
    r = runs.get_run("cornell", "near", {})
    st = r.state()
    n = len(r.points)
    tiled = np.tile(r.points, (COPIES, 1))
    assert tiled.shape == (COPIES * n, 3) and COPIES * n > 4 * 256 * 8 * 256
    got = st.probe_sh(tiled, 0, 2)
    assert got.shape == (COPIES * n, 9, 4)
    for k in (0, 1, 349, 699):
        want = st.probe_sh(r.points, 0, 2, stream_base=k * n)
        assert (want[:, 0, 3] > 0).sum() > 100
        assert np.array_equal(bits(got[k * n:(k + 1) * n]), bits(want)), k
    st.close()


# ------------------------------------------------------------------------------ 5: the physics
@pytest.fixture(scope="module")
def square_face():
    return SH.square_face_integrals()  # the 2000 x 2000 quadrature, once


@pytest.mark.parametrize("envhidden", [False, True], ids=["visible", "envhidden"])
def test_a_probe_below_a_square_under_a_constant_sky(envhidden, square_face, gpu, abi, lib, oracle):
    from jtrace import trace
    sc = IR.square_scene()
    sa = abi.SceneABI(sc)
    params = make_params(abi, width=W, height=H, traversal="near", batch=1, seed=IR.SQUARE_SEED, sampler=1, envhidden=envhidden)
    st = trace.TraceState(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, lib)
    got = st.probe_sh(np.zeros((IR.SQUARE_POINTS, 3), F32), 0, IR.SQUARE_SAMPLES).astype(np.float64)
    st.close()
    L = IR.SQUARE_L.astype(np.float64)
    keep, cover = SH.square_expected(square_face)
    assert abs(keep[0] - SH.C0 * 5 / 6) <= 1e-6 and abs(keep[1] + SH.C1 * IR.SQUARE_F / 4) <= 1e-6 and abs(cover[0] - SH.C0 / 6) <= 1e-6
    assert np.abs(keep[[2, 3, 4, 5, 7]]).max() <= 1e-12 and keep[6] > 0.02 and keep[8] > 0.04
    mean = got.mean(0)  # (9, 4)
    se = SH.SQUARE_SH_SE
    print("envhidden", envhidden, "rgb / L", mean[:, :3] / L, "expected", keep, "alpha", mean[:, 3], "expected",
          cover if envhidden else keep + cover, "5 se", 5 * se)
    if not envhidden:
        assert (np.abs(mean[:, :3] / L - keep[:, None]) <= 5 * se).all(), (mean[:, :3] / L, keep)
        # every sample is covered: alpha is the projection of 1, c0 and eight zeros
        assert (np.abs(mean[:, 3] - (keep + cover)) <= 5 * se).all(), mean[:, 3]
    else:
        assert (got[..., :3] == 0).all()
        assert (np.abs(mean[:, 3] - cover) <= 5 * se).all(), (mean[:, 3], cover)


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
            sh = st.probe_sh(r.points, 0, 3)
            rays = st.sphere_rays(r.points, 2)
            assert (sh[:, 0, 3] > 0).any() and rays.shape == (len(r.points), 6) and st.samples == 5
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
    want = st.probe_sh(r.points, 1, 3, stream_base=5)
    want_rays = st.sphere_rays(r.points, 1, stream_base=5)
    dev = torch.device("cuda", int(r.params.device))
    d_points = torch.from_numpy(np.array(r.points)).to(dev)
    got = st.probe_sh(d_points, 1, 3, stream_base=5)
    got_rays = st.sphere_rays(d_points, 1, stream_base=5)
    for t, shape in ((got, (n, 9, 4)), (got_rays, (n, 6))):
        assert isinstance(t, torch.Tensor) and t.device == d_points.device and tuple(t.shape) == shape
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(bits(got_rays.cpu().numpy()), bits(want_rays))
    buf = torch.zeros(n * 36 + 4, dtype=torch.float32, device=dev)
    status = lib.jt_probe_sh_device(st.handle, n, d_points.data_ptr(), 0, 0, 1, buf.data_ptr() + 4)
    assert status == -1 and "d_sh" in lib.jt_last_error().decode() and "aligned" in lib.jt_last_error().decode()
    status = lib.jt_sphere_rays_device(st.handle, n, d_points.data_ptr(), 0, 0, buf.data_ptr() + 4)
    assert status == -1 and "d_rays" in lib.jt_last_error().decode() and "aligned" in lib.jt_last_error().decode()
    assert not buf.any().item()
    with pytest.raises(ValueError, match="shape"):
        st.probe_sh(torch.zeros((n, 6), dtype=torch.float32, device=dev))
    st.close()


def test_the_host_variant_over_a_chunk_boundary_gives_the_bits_of_one_device_call(runs):
    """Option test_probe_chunk (tests only) lowers the host variant's chunk from 2^22 points to
    a third of the case's points and one: the array then takes three chunks, the last one partial,
    each staged and copied out on its own with stream_base advanced."""
    import torch
    r = runs.get_run("features1", "near", {})
    n = len(r.points)
    chunk = n // 3 + 1  # three chunks, the last one partial
    assert n >= 1000 and 2 * chunk < n < 3 * chunk, n
    plain = r.state()
    dev = torch.device("cuda", int(r.params.device))
    want = plain.probe_sh(torch.from_numpy(np.array(r.points)).to(dev), 1, 3, stream_base=5).cpu().numpy()
    plain.close()
    chunked = r.state(test_probe_chunk=chunk)
    got = chunked.probe_sh(r.points, 1, 3, stream_base=5)
    exact = chunked.probe_sh(r.points[:2 * chunk], 1, 3, stream_base=5)  # a whole number of chunks
    small = chunked.probe_sh(r.points[:chunk - 1], 1, 3, stream_base=5)  # less than one
    chunked.close()
    assert got.shape == (n, 9, 4) and (got[:, 0, 3] > 0).sum() > 100
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(exact), bits(want[:2 * chunk])) and np.array_equal(bits(small), bits(want[:chunk - 1]))
