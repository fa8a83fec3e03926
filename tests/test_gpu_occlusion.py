"""jt_ambient_occlusion on the GPU (occlusion_kernel, csrc/jt_intersect.hip): the share of a point's
hemisphere draws that meet nothing within a radius, against the calls it fuses, bit for bit, against
itself, and against a scene whose answer is known in closed form.

The cases, images (67 x 45) and points (gbuffer(-1) where it hits, at least 1000 per case) are those
of tests/test_gpu_irradiance.py: cornell in the three orders, features1, the deep scene through the
overflow stack, test_lds_ring = 2; samples 0 and 7, stream_base 0 and 5; the radius a quarter of the
scene's diagonal, and +inf.

1. One sample: ambient_occlusion(points, R, s, s + 1, base) is 1 - occluded(hemisphere_rays(points,
   s, base), tmax=R) as 0.0 / 1.0, in every bit.
2. The range [3, 8) is (visible one-sample results) / 5 in float32.
3. Halves with stream_base advanced, n = 1, 63, 64, 65, all; 700 copies across refills.
4. The square scene of tests/irradiance_ref.py, 64 points x 1024 samples: the square is at distance
   >= 1, so radius 0.75 gives exactly 1.0 at every point; radius 2 (above sqrt 3, the square's
   farthest point) gives the mean visibility 1 - SQUARE_F within 5 SQUARE_SE, the irradiance test's bar.
5. The context is untouched. 6. The device variant gives the host's bits."""
import numpy as np
import pytest

import irradiance_ref as IR
from conftest import make_params
from test_gpu_irradiance import H, SEED, W, Runs, bits  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = ("reference", "near", "wide")
CASES = [("cornell", ALL, {}), ("features1", ("near",), {}), ("deep_lit", ("wide",), {}), ("cornell", ("near",), {"test_lds_ring": 2})]
RUNS = [pytest.param(name, order, opts, id=f"{name}-{order}" + ("-ring2" if opts else ""))
        for name, orders, opts in CASES for order in orders]
SAMPLES = (0, 7)


@pytest.fixture(scope="module")
def runs(gpu, abi, lib, oracle):
    return Runs(abi, lib, oracle)


def diagonal(scene):
    """The diagonal of the scene's world-space bounding box."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in scene.instances:
        f = np.asarray(inst.frame, np.float64).reshape(4, 3)
        w = np.asarray(scene.shapes[inst.shape].positions, np.float64) @ f[:3] + f[3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return float(np.linalg.norm(hi - lo))


def radii(r):
    return (F32(0.25 * diagonal(r.scene)), F32(np.inf))


def bases_of(name, order, opts):
    return (0, 5) if (name, order) == ("cornell", "near") and not opts else (0,)


# ------------------------------------------------------------------------------ 1: one sample
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_one_sample_is_the_bounded_any_hit_query_of_the_hemisphere_ray(name, order, opts, runs):
    r = runs.get_run(name, order, opts)
    n = len(r.points)
    assert n >= 1000, (name, n)
    if opts:
        assert "ring_used=2" in r.describe, r.describe
    if name == "deep_lit":
        assert "hbm_overflow=1" in r.describe and "traversal=wide" in r.describe, r.describe
    st = r.state()
    seen = set()
    for radius in radii(r):
        for base in bases_of(name, order, opts):
            for s in SAMPLES:
                got = st.ambient_occlusion(r.points, radius, s, s + 1, stream_base=base)
                rays = st.hemisphere_rays(r.points, s, stream_base=base)
                want = np.where(st.occluded(rays, tmax=radius), F32(0), F32(1)).astype(F32)
                assert got.shape == (n,) and got.dtype == F32
                diff = bits(got) != bits(want)
                print(name, order, "radius", radius, "sample", s, "base", base, "points", n, "visible", int((got == 1).sum()),
                      "differing", int(diff.sum()))
                assert not diff.any(), (name, order, radius, s, base, np.flatnonzero(diff)[:8])
                if np.isinf(radius):  # an infinite radius is the unbounded query
                    assert np.array_equal(want == 0, st.occluded(rays))
                seen.add((float(radius), int((got == 1).sum())))
    st.close()
    # a bound can only open the hemisphere, and in the closed box it does
    finite = max(v for rad, v in seen if np.isfinite(rad))
    unbounded = max(v for rad, v in seen if np.isinf(rad))
    assert finite >= unbounded and (name != "cornell" or finite > unbounded), (name, finite, unbounded)


# ------------------------------------------------------------------------------ 2: the quotient
@pytest.mark.parametrize("name", ["cornell", "features1"])
def test_a_range_is_the_visible_count_over_the_samples(name, runs):
    r = runs.get_run(name, "near", {})
    st = r.state()
    for radius in radii(r):
        got = st.ambient_occlusion(r.points, radius, 3, 8)
        count = np.zeros(len(r.points), np.int64)
        for s in range(3, 8):
            one = st.ambient_occlusion(r.points, radius, s, s + 1)
            assert np.isin(one, (0.0, 1.0)).all()
            count += one == 1
        want = count.astype(F32) / F32(5)
        assert want.dtype == F32 and len(np.unique(count)) >= 2
        diff = bits(got) != bits(want)
        assert not diff.any(), (name, radius, int(diff.sum()), got[diff][:4], want[diff][:4])
    st.close()


# ------------------------------------------------------------------------------ 3: partition, grid
def test_partition_and_grid_independence(runs):
    r = runs.get_run("cornell", "near", {})
    st = r.state()
    pts, radius = r.points, radii(r)[0]
    whole = st.ambient_occlusion(pts, radius, 0, 4)
    assert len(np.unique(whole)) >= 3
    for n in (1, 63, 64, 65, len(pts)):
        one = st.ambient_occlusion(pts[:n], radius, 0, 4)
        h = n // 2
        two = np.concatenate([st.ambient_occlusion(pts[:h], radius, 0, 4), st.ambient_occlusion(pts[h:n], radius, 0, 4, stream_base=h)])
        assert one.shape == two.shape == (n,)
        assert np.array_equal(bits(one), bits(two)) and np.array_equal(bits(one), bits(whole[:n])), n
    shifted = st.ambient_occlusion(pts[100:200], radius, 0, 4, stream_base=100)
    assert np.array_equal(bits(shifted), bits(whole[100:200]))
    assert not np.array_equal(bits(st.ambient_occlusion(pts[100:200], radius, 0, 4)), bits(whole[100:200]))
    st.close()


def test_partition_across_refills(runs):
    """700 copies of the points are more than four points for every lane of a 256-unit device's
    persistent grid: lanes finish a point, with all its samples, and take another. Copy k of the
    result is the small call with stream_base k * n, in every bit."""
    COPIES = 700
    r = runs.get_run("cornell", "near", {})
    st = r.state()
    n, radius = len(r.points), radii(r)[0]
    tiled = np.tile(r.points, (COPIES, 1))
    assert COPIES * n > 4 * 256 * 8 * 256
    got = st.ambient_occlusion(tiled, radius, 0, 2)
    assert got.shape == (COPIES * n,)
    for k in (0, 1, 349, 699):
        want = st.ambient_occlusion(r.points, radius, 0, 2, stream_base=k * n)
        assert len(np.unique(want)) >= 2
        assert np.array_equal(bits(got[k * n:(k + 1) * n]), bits(want)), k
    st.close()


# ------------------------------------------------------------------------------ 4: the physics
def test_a_square_overhead_within_and_beyond_the_radius(gpu, abi, lib, oracle):
    from jtrace import trace
    sc = IR.square_scene()
    sa = abi.SceneABI(sc)
    params = make_params(abi, width=W, height=H, traversal="near", batch=1, seed=IR.SQUARE_SEED, sampler=1)
    st = trace.TraceState(sa, oracle.build_bvh(sa), oracle.make_lights(sa), params, lib)
    near = st.ambient_occlusion(IR.square_points(), 0.75, 0, IR.SQUARE_SAMPLES)
    far = st.ambient_occlusion(IR.square_points(), 2.0, 0, IR.SQUARE_SAMPLES).astype(np.float64)
    unbounded = st.ambient_occlusion(IR.square_points(), np.inf, 0, IR.SQUARE_SAMPLES)
    st.close()
    assert near.shape == (IR.SQUARE_POINTS,) and (near == 1.0).all(), near
    mean = far.mean()
    print("mean visibility", mean, "1 - F", 1 - IR.SQUARE_F, "deviation in standard errors", (mean - (1 - IR.SQUARE_F)) / IR.SQUARE_SE)
    assert abs(mean - (1 - IR.SQUARE_F)) <= 5 * IR.SQUARE_SE, (mean, 1 - IR.SQUARE_F)
    assert np.array_equal(bits(unbounded), bits(far.astype(F32)))  # nothing of the scene lies beyond 2


# ------------------------------------------------------------------------------ 5: the context
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
            ao = st.ambient_occlusion(r.points, radii(r)[0], 0, 3)
            assert (ao > 0).any() and (ao < 1).any() and st.samples == 5
        image = st.get_image()
        albedo, normal, hits = st.get_aovs()
        cnt = st.counters()
        cnt.pop("kernel_ms")
        out.append((image, albedo, normal, hits, cnt))
        st.close()
    for x, y in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(out[0][3], out[1][3]) and out[0][4] == out[1][4] and out[0][4]["paths"] == 5 * W * H, out[0][4]


# ------------------------------------------------------------------------------ 6: the device variant
def test_device_variant_gives_the_host_bits_and_rejects_a_misaligned_output(runs, abi, lib):
    import torch
    r = runs.get_run("features1", "near", {})
    st = r.state()
    n, radius = len(r.points), radii(r)[0]
    want = st.ambient_occlusion(r.points, radius, 1, 4, stream_base=5)
    dev = torch.device("cuda", int(r.params.device))
    d_points = torch.from_numpy(np.array(r.points)).to(dev)
    got = st.ambient_occlusion(d_points, radius, 1, 4, stream_base=5)
    assert isinstance(got, torch.Tensor) and got.device == d_points.device and tuple(got.shape) == (n,) and got.dtype == torch.float32
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and len(np.unique(want)) >= 2
    buf = torch.zeros(n + 4, dtype=torch.float32, device=dev)
    status = lib.jt_ambient_occlusion_device(st.handle, n, d_points.data_ptr(), 0, 0, 1, 1.0, buf.data_ptr() + 2)
    assert status == -1 and "d_visibility" in lib.jt_last_error().decode() and "aligned" in lib.jt_last_error().decode()
    assert not buf.any().item()
    st.close()
