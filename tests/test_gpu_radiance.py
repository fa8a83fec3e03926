"""jt_radiance on the GPU (csrc/jt_radiance.hip): the integrator on the caller's own rays against the
megakernel bit for bit, against the oracle, against itself.

Images are 67 x 45 (3015 pixels: the last wave of a launch is partial), the scenes tests/surface_ref.py's
and tests/scenes_ref.py's deep scene, one context per case, order and sample, batch 1, explicit
traversal orders.

1. radiance(camera_rays(s), s, s + 1) is the image of a fresh context that traced [s, s + 1) alone,
   in every bit of every pixel.
2. Against the oracle directly (oracle.trace(..., s, s + 1, first=s)): the pixels where radiance
   differs from the oracle in any bit are a subset of those where the megakernel's image of 1 differs,
   and those are at most 0.1 % of the pixels (3 of 3015), DESIGN.md section 8(c)'s bar. A difference comes
   from a 1-ulp libm difference that flips a discrete decision. The megakernel's own count, measured
   on an MI355X at samples 0 and 7 (the test prints it): 0 of 3015 pixels in every case of CASES
   and every order, at both samples, and 0 for radiance too. So every case keeps samples 0 and 7.
3. The mean over samples: radiance(rays, 3, 8) is the float32 fold, in numpy, of the five one-sample
   calls, acc = acc * (1 - w) + x * w with w = 1 / (c + 1) from 0.
4. Partition and grid independence: one call on rays[:n] equals two calls on its halves, the second
   with stream_base advanced, and the first n results do not depend on n. Once at 2.1 M rays, where
   waves claim and refill many times, blocks of the result equal the small call with their stream_base.
5. Rays no camera makes: alpha is 1 exactly where jt_intersect reports a hit, a miss is four zero
   words, every value is finite and within [0, params.clamp].
6. The context is untouched. 7. The device variant gives the host variant's bits.

The deep scene (scenes_ref.deep_scene) has no light, and the path sampler's sample_lights indexes the
light list without looking at its length, in the reference, the oracle and the kernels alike. So the
case `deep` traces it with the naive sampler, which never samples a light, and `deep_lit` traces it
with the path sampler after giving its material an emission: every triangle of the deep BVH is
then part of an instance light, and the light queries run through the overflow stack too."""
import copy

import numpy as np
import pytest

import scenes_ref as SR
import surface_ref as R
from conftest import make_params

pytestmark = pytest.mark.gpu

W, H, N = R.W, R.H, R.W * R.H
F32 = np.float32
ALL = ("reference", "near", "wide")
# (case, orders, library options)
CASES = [("cornell", ALL, {}), ("cornell_hbm", ("near",), {}), ("naive", ("near",), {}), ("tent", ("near",), {}),
         ("lens", ("near",), {}), ("ortho", ("near",), {}), ("features1", ("near",), {}), ("materials4", ("near",), {}),
         ("materials2", ("near",), {}), ("coplanar", ("near",), {}), ("random", ALL, {}), ("deep", ("wide",), {}),
         ("deep_lit", ("wide",), {}), ("cornell", ("near",), {"test_lds_ring": 2})]
RUNS = [pytest.param(name, order, opts, id=f"{name}-{order}" + ("-ring2" if opts else ""))
        for name, orders, opts in CASES for order in orders]
SAMPLES = (0, 7)
MAX_MISMATCH = 3  # 0.1 % of 3015 pixels


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def scene_of(name):
    if name in ("deep", "deep_lit"):
        sc = SR.deep_scene()
        if name == "deep_lit":
            sc = copy.deepcopy(sc)
            sc.materials[0].emission = np.array([2.0, 1.5, 1.0], F32)
            return sc, {}, {}
        return sc, {"sampler": 2}, {}
    return R.case(name)


class Run:
    """One (case, order, options): the oracle's scene, and contexts opened on demand."""

    def __init__(self, name, order, opts, abi, lib, oracle):
        self.abi, self.lib, self.oracle, self.order = abi, lib, oracle, order
        self.scene, self.kw, o = scene_of(name)
        self.opts = {**o, **opts}
        self.sa = abi.SceneABI(self.scene)
        self.bvh, self.lights = oracle.build_bvh(self.sa), oracle.make_lights(self.sa)
        self.params = make_params(abi, width=W, height=H, traversal=order, batch=1, **self.kw)
        self.pairs = {}

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

    def pair(self, s):
        """(the image of a fresh context that traced [s, s + 1) alone, radiance(camera_rays(s), s,
        s + 1) on that context afterwards, describe()), computed once and shared (read-only)."""
        if s not in self.pairs:
            st = self.state()
            st.trace_range(s, s + 1)
            image = st.get_image().reshape(N, 4).copy()
            describe = st.describe()
            rad = st.radiance(st.camera_rays(s), s, s + 1)
            st.close()
            for a in (image, rad):
                a.setflags(write=False)
            self.pairs[s] = (image, rad, describe)
        return self.pairs[s]


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


# ------------------------------------------------------------------------------ 1: the megakernel
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_radiance_of_camera_rays_is_the_megakernel_image_bit_for_bit(name, order, opts, runs):
    r = runs.get_run(name, order, opts)
    for s in SAMPLES:
        image, rad, describe = r.pair(s)
        if opts:
            assert "ring_used=2" in describe, describe
        if name == "cornell_hbm":
            assert "mode=hbm" in describe, describe
        if name.startswith("deep"):
            assert "hbm_overflow=1" in describe and "traversal=wide" in describe, describe
        assert rad.shape == (N, 4) and rad.dtype == F32
        diff = (bits(image) != bits(rad)).any(1)
        print(name, order, "sample", s, "alpha 1 pixels", int((rad[:, 3] == 1).sum()), "differing pixels", int(diff.sum()))
        assert (rad[:, 3] == 1).sum() > 100, "the camera sees the scene"
        assert not diff.any(), (name, order, s, np.flatnonzero(diff)[:8], image[diff][:4], rad[diff][:4])


# ------------------------------------------------------------------------------ 2: the oracle
@pytest.mark.parametrize("name,order,opts", RUNS)
def test_radiance_differs_from_the_oracle_only_where_the_megakernel_does(name, order, opts, runs):
    r = runs.get_run(name, order, opts)
    for s in SAMPLES:
        image, rad, _ = r.pair(s)
        want = r.oracle.trace(r.sa, r.bvh, r.lights, r.params, W, H, s, s + 1, first=s)[0].reshape(N, 4)
        mega = (bits(image) != bits(want)).any(1)
        mine = (bits(rad) != bits(want)).any(1)
        print(f"MISMATCH {name}-{order}{'-ring2' if opts else ''} sample {s}: megakernel {int(mega.sum())} radiance {int(mine.sum())}")
        assert not (mine & ~mega).any(), (name, order, s, np.flatnonzero(mine & ~mega)[:8])
        assert mega.sum() <= MAX_MISMATCH and mine.sum() <= MAX_MISMATCH, (name, order, s, int(mega.sum()), int(mine.sum()))


# ------------------------------------------------------------------------------ 3: the mean
@pytest.mark.parametrize("name", ["cornell", "features1"])
def test_the_mean_over_samples_is_the_float32_fold_of_one_sample_calls(name, runs):
    st = runs.get_run(name, "near", {}).state()
    rays = st.camera_rays(0)
    got = st.radiance(rays, 3, 8)
    acc = np.zeros((N, 4), F32)
    for c, s in enumerate(range(3, 8)):
        x = st.radiance(rays, s, s + 1)
        w = F32(1) / F32(c + 1)
        acc = acc * (F32(1) - w) + x * w
    st.close()
    assert acc.dtype == F32 and (got[:, 3] > 0).sum() > N // 10
    diff = (bits(got) != bits(acc)).any(1)
    assert not diff.any(), (name, int(diff.sum()), got[diff][:4], acc[diff][:4])


# ------------------------------------------------------------------------------ 4: partition, grid
def test_partition_and_grid_independence(runs):
    st = runs.get_run("cornell", "near", {}).state()
    rays = st.camera_rays(0)
    whole = st.radiance(rays, 0, 2)
    for n in (1, 63, 64, 65, N):
        one = st.radiance(rays[:n], 0, 2)
        h = n // 2
        two = np.concatenate([st.radiance(rays[:h], 0, 2), st.radiance(rays[h:n], 0, 2, stream_base=h)])
        assert one.shape == two.shape == (n, 4)
        assert np.array_equal(bits(one), bits(two)), n
        assert np.array_equal(bits(one), bits(whole[:n])), n
    # the stream is the ray's index plus stream_base, not the ray's place in the call
    shifted = st.radiance(rays[100:200], 0, 2, stream_base=100)
    assert np.array_equal(bits(shifted), bits(whole[100:200]))
    assert not np.array_equal(bits(st.radiance(rays[100:200], 0, 2)), bits(whole[100:200]))
    st.close()


def test_partition_across_refills(runs):
    """The refill past a wave's first claim, which the 3015 rays of every other test never reach (each
    wave claims 64 once). 700 copies of the camera's rays are 2 110 500 rays, more than 4 x 256 x 8 x
    256 (test_gpu_intersect.py's bound: four rays for every lane of a 256-unit device's persistent
    grid), and a wave claims 256 at a time: lanes finish a ray and take another, a reserve spans
    several refills, and the hand-out (csrc/jt_feed.h) runs to its drain inside radiance_kernel.
    Copy k of the result is the small call with stream_base k * N, in every bit."""
    COPIES = 700
    st = runs.get_run("cornell", "near", {}).state()
    rays = st.camera_rays(0)
    tiled = np.tile(rays, (COPIES, 1))
    assert tiled.shape == (COPIES * N, 6) and COPIES * N > 4 * 256 * 8 * 256
    got = st.radiance(tiled, 0, 1)
    assert got.shape == (COPIES * N, 4)
    for k in (0, 1, 349, 699):
        want = st.radiance(rays, 0, 1, stream_base=k * N)
        assert (want[:, 3] == 1).sum() > 100
        assert np.array_equal(bits(got[k * N:(k + 1) * N]), bits(want)), k
    st.close()


# ------------------------------------------------------------------------------ 5: rays no camera makes
def world_box(scene):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for ins in scene.instances:
        ax, o = R._frame(ins.frame)
        p = np.asarray(scene.shapes[ins.shape].positions, np.float64) @ ax + o
        lo, hi = np.minimum(lo, p.min(0)), np.maximum(hi, p.max(0))
    return lo, hi


@pytest.mark.parametrize("name", ["cornell", "random"])
def test_rays_no_camera_makes(name, runs):
    r = runs.get_run(name, "near", {})
    assert name in R.OPAQUE and len(r.scene.environments) == 0
    lo, hi = world_box(r.scene)
    rng = np.random.default_rng(23)
    d = rng.normal(size=(512, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform(lo, hi, size=(512, 3))
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    o[256:] = centre + d[256:] * (2.0 * np.linalg.norm(half))  # outside the box, pointing away from it
    rays = np.concatenate([o, d], 1).astype(F32)
    rays[:, 3:] /= np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1, keepdims=True).astype(F32)
    st = r.state()
    hit = st.intersect(rays)["hit"] != 0
    got = st.radiance(rays, 0, 1)
    clamp = float(r.params.clamp)
    st.close()
    print(name, "hits", int(hit.sum()), "max value", float(got[:, :3].max()), "clamp", clamp)
    assert 8 < hit[:256].sum() < 256 and not hit[256:].any()  # random's geometry is sparse: 16 of its 256 inside rays hit
    assert np.array_equal(got[:, 3], hit.astype(F32))
    assert (bits(got[~hit]) == 0).all()
    assert np.isfinite(got).all() and (got >= 0).all() and (got[:, :3] <= clamp).all(), float(got[:, :3].max())


# ------------------------------------------------------------------------------ 6: the context
def test_the_context_is_untouched(runs):
    r = runs.get_run("cornell", "near", {})
    a, b = r.state(), r.state()
    rays = a.camera_rays(2)
    out = []
    for st in (a, b):
        st.trace_range(0, 4)
        st.get_image()  # flushes: four samples traced
        st.trace_range(4, 5)  # queued
        assert st.samples == 5
        if st is a:
            rad = st.radiance(rays, 0, 3)
            assert (rad[:, 3] > 0).any() and st.samples == 5
        image = st.get_image()
        albedo, normal, hits = st.get_aovs()
        cnt = st.counters()
        cnt.pop("kernel_ms")
        out.append((image, albedo, normal, hits, cnt))
        st.close()
    for x, y in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(out[0][3], out[1][3]) and out[0][4] == out[1][4] and out[0][4]["paths"] == 5 * N, out[0][4]


# ------------------------------------------------------------------------------ 7: the device variant
def test_device_variant_gives_the_host_bits_and_rejects_a_misaligned_output(runs, abi, lib):
    import torch
    r = runs.get_run("features1", "near", {})
    st = r.state()
    rays = st.camera_rays(1)
    want = st.radiance(rays, 1, 3, stream_base=5)
    dev = torch.device("cuda", int(r.params.device))
    d_rays = torch.from_numpy(rays).to(dev)
    got = st.radiance(d_rays, 1, 3, stream_base=5)
    assert isinstance(got, torch.Tensor) and got.device == d_rays.device and tuple(got.shape) == (N, 4)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    buf = torch.zeros(N * 4 + 4, dtype=torch.float32, device=dev)
    status = lib.jt_radiance_device(st.handle, N, d_rays.data_ptr(), 0, 0, 1, buf.data_ptr() + 4)
    assert status == -1 and "aligned" in lib.jt_last_error().decode()
    assert not buf.any().item()
    st.close()
