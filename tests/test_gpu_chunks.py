"""The chunk schedule of a one-stream context (batch <= 1: the reference's --batch 1, one running
mean) at its edge counts.

Such a context traces a range of more than one sample as chunks of one-sample streams
(trace_launch, csrc/jt_trace.hip; the schedule is chunk_plan, csrc/jt_plan.h): chunk i is traced
into buffer set i & 1 on one stream while chain_kernel (csrc/jt_accum.hip) folds chunk i - 1 into
the running mean on a second one. The contract is the bits of one launch per sample. The option
test_trace_chunk (tests only) lowers the chunk from 64 samples, so that at cornellbox 44x36 (6x5
tiles, the last column and row 4 pixels wide) a few tens of samples reach

  - a tail chunk of one sample (n = chunk + 1, 2 chunk + 1, 4 chunk + 1), which must go through the
    chunk buffers like every other chunk;
  - the reuse of a buffer set behind the chain that read it (three and more chunks);
  - a full and a partial last chunk;
  - chunk 1, the fallback when the second stream, the events or the buffers cannot be had: the
    range as one launch of long items;
  - the other routes into a chunked range: a context that starts past sample 0, a second range on
    a non-empty mean, a reset, queued trace_samples calls, exported device buffers, a tile share,
    and the HBM-mode kernels.

The expected value is a context that traces the same samples one launch each (jt_synchronize
after every sample); image, albedo, normal and hits are compared with np.array_equal, the paths,
rays and light_queries counters for equality. Two checks stand apart from the library's own
launches: the oracle, and a float64 mean of the samples' own values.
"""
import numpy as np
import pytest

from conftest import compare_images, make_params

pytestmark = pytest.mark.gpu

W, H = 44, 36
KEYS = ("paths", "rays", "light_queries")
NAMES = ("image", "albedo", "normal", "hits")


def snapshot(st):
    c = st.counters()
    return {"image": st.get_image(), **dict(zip(NAMES[1:], st.get_aovs())), "launches": c["launches"],
            **{k: c[k] for k in KEYS}}


def assert_same(exp, got, label):
    for name in NAMES:
        assert np.array_equal(exp[name], got[name]), (label, name, float(np.abs(exp[name].astype(np.float64) - got[name]).max()))
    for k in KEYS:
        assert exp[k] == got[k], (label, k, exp[k], got[k])
    assert got["hits"].sum() > 0 and got["image"][..., :3].max() > 0, (label, "nothing hit or lit")


class Scene:
    """cornellbox at 44x36 with one stream: contexts, and the per-sample expected values, each
    computed once and shared (they are never written to)."""

    def __init__(self, abi, lib, sa):
        from jtrace import trace
        self.abi, self.lib, self.sa, self.trace = abi, lib, sa, trace
        self.bvh = trace.make_scene_bvh(sa, False, lib)
        self.lights = trace.make_trace_lights(sa, lib)
        self._per_sample = {}

    def params(self, samples, sampler=1):
        return make_params(self.abi, width=W, height=H, samples=samples, batch=1, sampler=sampler)

    def state(self, samples, sampler=1):
        st = self.trace.make_trace_state(self.sa, self.bvh, self.lights, self.params(samples, sampler), self.lib)
        assert st.streams == 1, st.describe()
        assert (st.width, st.height) == (W, H)
        return st

    def launch_per_sample(self, sampler, first, count):
        """snapshots[n - 1]: the running means after samples first .. first + n - 1, one launch each"""
        st = self.state(first + count, sampler)
        snaps = []
        for s in range(first, first + count):
            st.trace_range(s, s + 1)
            st.synchronize()
            snaps.append(snapshot(st))
            assert snaps[-1]["launches"] == s - first + 1  # reading flushes nothing more
        st.close()
        return snaps

    def per_sample(self, sampler, n, first=0):
        """the expected value of samples first .. first + n - 1 (default options, LDS mode)"""
        most = {(1, 0): 129, (2, 0): 21}.get((sampler, first), n)  # the longest range a test of this file asks for
        key = (sampler, first)
        if key not in self._per_sample or len(self._per_sample[key]) < n:
            self._per_sample[key] = self.launch_per_sample(sampler, first, max(n, most))
        return self._per_sample[key][n - 1]


@pytest.fixture(scope="module")
def scene(abi, lib, cornell_abi):
    return Scene(abi, lib, cornell_abi)


def chunked_range(scene, n, sampler=1, first=0):
    st = scene.state(first + n, sampler)
    st.trace_range(first, first + n)
    out = snapshot(st)
    st.close()
    return out


def edge_counts(chunk):
    # at chunk 2, 2 chunk + 1 and 3 chunk - 1 are the same count
    return sorted({chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk - 1, 4 * chunk + 1, 5 * chunk})


EDGE_CASES = ([(4, n, s) for s in (1, 2) for n in edge_counts(4)] +
              [(c, n, 1) for c in (2, 8) for n in edge_counts(c)])


@pytest.mark.parametrize("chunk,n,sampler", EDGE_CASES)
def test_edge_counts_match_per_sample_launches(gpu, scene, options, chunk, n, sampler):
    """One trace_range(0, n) at chunk 2, 4 and 8: a tail of one sample (chunk + 1, 2 chunk + 1,
    4 chunk + 1), set reuse over three to five chunks, a full (2 chunk, 5 chunk) and a partial
    (3 chunk - 1) last chunk; ceil(n / chunk) launches."""
    exp = scene.per_sample(sampler, n)
    options("test_trace_chunk", chunk)
    got = chunked_range(scene, n, sampler)
    assert got["launches"] == -(-n // chunk), got["launches"]
    assert_same(exp, got, (chunk, n, sampler))


@pytest.mark.parametrize("n", [65, 129])
def test_natural_chunk_with_a_tail_of_one(gpu, scene, n):
    """No option: the chunk is 64, and 65 and 129 samples are 64 + 1 and 64 + 64 + 1."""
    exp = scene.per_sample(1, n)
    got = chunked_range(scene, n)
    assert got["launches"] == -(-n // 64), got["launches"]
    assert_same(exp, got, n)


@pytest.mark.parametrize("n", [2, 5])
def test_no_chunks_is_one_launch_of_long_items(gpu, scene, options, n):
    """test_trace_chunk = 1 takes the path of chunk buffers that could not be had: the range is
    one launch whose items run several samples each, then a second range (5, 9) whose items start
    from the running mean of the first (n0 > 0) — the bits of per-sample launches both times."""
    exp, exp9 = scene.per_sample(1, n), scene.per_sample(1, 9)
    options("test_trace_chunk", 1)
    st = scene.state(9)
    st.trace_range(0, n)
    got = snapshot(st)
    assert got["launches"] == 1, got["launches"]
    assert_same(exp, got, n)
    if n == 5:
        st.trace_range(5, 9)
        got = snapshot(st)
        assert got["launches"] == 2, got["launches"]
        assert_same(exp9, got, "second range")
    st.close()


def test_route_context_starting_past_sample_zero(gpu, scene, options):
    """(a) first > 0, a shard's context: trace_range(3, 12) is chunks 4 + 4 + 1 from sample 3, folded
    with n0 = x - first."""
    exp = scene.per_sample(1, 9, first=3)
    options("test_trace_chunk", 4)
    got = chunked_range(scene, 9, first=3)
    assert got["launches"] == 3
    assert_same(exp, got, "first = 3")


def test_route_second_range_on_a_non_empty_mean(gpu, scene, options):
    """(b) (0, 5) then (5, 14) with the image read between them: 4 + 1, then 4 + 4 + 1 with n0 = 5
    at its first chunk."""
    exp5, exp = scene.per_sample(1, 5), scene.per_sample(1, 14)
    options("test_trace_chunk", 4)
    st = scene.state(14)
    st.trace_range(0, 5)
    assert np.array_equal(st.get_image(), exp5["image"])
    st.trace_range(5, 14)
    got = snapshot(st)
    st.close()
    assert got["launches"] == 2 + 3
    assert_same(exp, got, "(0, 5) + (5, 14)")


def test_route_reset_then_a_chunked_range(gpu, scene, options):
    """(c) jt_reset after a chunked range, then trace_range(0, 9): a fresh context's."""
    exp = scene.per_sample(1, 9)
    options("test_trace_chunk", 4)
    st = scene.state(9)
    st.trace_range(0, 9)
    assert st.counters()["launches"] == 3
    st.reset()
    assert st.samples == 0
    st.trace_range(0, 9)
    got = snapshot(st)
    st.close()
    assert got["launches"] == 3  # counted from the reset
    assert_same(exp, got, "after reset")


@pytest.mark.parametrize("read_after", [None, 5])
def test_route_queued_trace_samples(gpu, scene, options, read_after):
    """(d) nine queued trace_samples calls of a 9-sample render: the end-of-render flush, the
    command line's route; (e) five queued, the image read, four more."""
    exp5, exp = scene.per_sample(1, 5), scene.per_sample(1, 9)
    options("test_trace_chunk", 4)
    st = scene.state(9)
    for s in range(9):
        st.trace_samples()
        if read_after == s + 1:
            assert np.array_equal(st.get_image(), exp5["image"])
    assert st.samples == 9
    got = snapshot(st)
    st.close()
    assert got["launches"] == (3 if read_after is None else 2 + 1), got["launches"]
    assert_same(exp, got, read_after)


def test_route_exported_device_buffers(gpu, scene, options):
    """(f) a context whose device pointers were handed out before the range flushes every call;
    the running means read in place equal jt_get_image and jt_get_aovs and the per-sample launches'."""
    torch = pytest.importorskip("torch")
    exp = scene.per_sample(1, 9)
    options("test_trace_chunk", 4)
    st = scene.state(100)  # not the end of a render: the range is traced because the buffers are out
    buf = st.device_buffers()
    st.trace_range(0, 9)

    def view(ptr, n, typestr):
        class _V:
            __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}
        return torch.as_tensor(_V(), device="cuda:0").cpu().numpy()

    torch.cuda.synchronize()
    img = view(buf.image, H * W * 4, "<f4").reshape(H, W, 4)
    alb = view(buf.albedo, H * W * 4, "<f4").reshape(H, W, 4)[..., :3]
    nrm = view(buf.normal, H * W * 4, "<f4").reshape(H, W, 4)[..., :3]
    hit = view(buf.hits, H * W, "<i8").reshape(H, W)
    got = snapshot(st)
    st.close()
    assert got["launches"] == 3
    for name, a in zip(NAMES, (img, alb, nrm, hit)):
        assert np.array_equal(a, got[name]), name
    assert_same(exp, got, "exported")


def test_route_tile_share(gpu, scene, options):
    """(g) the tile share "4,3": tiles 3, 7, ..., 27 of 30 in chunks 4 + 4 + 1, every other pixel zero."""
    options("tile_share", "4,3")
    exp = scene.launch_per_sample(1, 0, 9)[-1]
    options("test_trace_chunk", 4)
    got = chunked_range(scene, 9)
    assert got["launches"] == 3
    assert_same(exp, got, "share 4,3")
    ty, tx = np.divmod(np.arange(30), 6)
    mask = np.zeros((H, W), bool)
    for t in range(3, 30, 4):
        mask[ty[t] * 8:ty[t] * 8 + 8, tx[t] * 8:tx[t] * 8 + 8] = True
    for name in NAMES:
        assert np.all(got[name][~mask] == 0), name
    assert np.any(got["image"][mask] != 0)
    assert got["paths"] == 9 * int(mask.sum())


def test_hbm_mode_kernels(gpu, scene, options):
    """Chunks 4 + 4 + 1 with the scene in HBM (lds_scene = 0): the bits of per-sample launches (those
    of the default LDS mode: the memory mode never changes them)."""
    exp = scene.per_sample(1, 9)
    options("lds_scene", "0")
    options("test_trace_chunk", 4)
    st = scene.state(9)
    assert "mode=lds" not in st.describe(), st.describe()
    st.trace_range(0, 9)
    got = snapshot(st)
    st.close()
    assert got["launches"] == 3
    assert_same(exp, got, "hbm")


@pytest.mark.parametrize("sampler", [1, 2])
def test_chunks_match_the_oracle(gpu, scene, options, oracle, sampler):
    """(i) chunks 4 + 4 + 1 against the CPU oracle's single running mean over samples 0 .. 8, at the
    bars of test_gpu_parity.py test_cornellbox_parity."""
    options("test_trace_chunk", 4)
    got = chunked_range(scene, 9, sampler)
    o = oracle.trace(scene.sa, oracle.build_bvh(scene.sa), oracle.make_lights(scene.sa), scene.params(9, sampler),
                     W, H, 0, 9, streams=1)
    stats = compare_images(got["image"], o[0])
    print("sampler", sampler, stats)
    assert stats["frac_pix_rel_le_1e-3"] >= 0.999, stats
    assert stats["bitwise_frac"] >= 0.999, stats
    assert stats["image_mean_rel"] <= 1e-4, stats
    assert np.array_equal(got["hits"], o[3])
    assert got["paths"] == o[4]["paths"] == W * H * 9
    for a, b in ((got["albedo"], o[1]), (got["normal"], o[2])):
        assert compare_images(a, b)["frac_pix_rel_le_1e-3"] >= 0.999


@pytest.mark.parametrize("sampler", [1, 2])
def test_chunks_match_a_float64_mean_of_the_samples(gpu, scene, options, sampler):
    """(ii) nine fresh contexts trace one sample s each: with first = s the running mean is that
    sample's value v_s itself (0 * 0 + v * 1). The chunked image of samples 0 .. 8 must be their mean.

    Bound, per channel and pixel: 3 n u V with u = 2^-24 and V = max_s |v_s|, three roundings per
    fold step. Step j computes m <- m (1 - w) + v w with w = 1 / j, |m| and |v| at most V: the
    rounding of 1 - w costs at most u V, the two products together u V (their exact sizes add up to
    at most V), the sum u V, and the rounding of w itself 2 w u V more. The later steps scale what
    step j added by j / n, so the total is at most sum_j (3 + 2 / j) (j / n) u V = (1.5 n + 3.5) u V,
    below 3 n u V from n = 3. A dropped, doubled or stale sample moves a lit pixel by about V / n,
    five orders more. Hits are integers: their sum exactly."""
    n = 9
    vs = []
    for s in range(n):
        st = scene.state(s + 1, sampler)
        st.trace_range(s, s + 1)
        vs.append(snapshot(st))
        assert vs[-1]["launches"] == 1
        st.close()
    options("test_trace_chunk", 4)
    got = chunked_range(scene, n, sampler)
    assert got["launches"] == 3
    assert np.array_equal(got["hits"], sum(v["hits"] for v in vs))
    for name in ("image", "albedo", "normal"):
        v = np.stack([x[name].astype(np.float64) for x in vs])
        bound = 3 * n * 2.0 ** -24 * np.abs(v).max(axis=0)
        err = np.abs(got[name].astype(np.float64) - v.mean(axis=0))
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(name, "sampler", sampler, "worst error / bound", worst, "max error", float(err.max()))
        assert np.all(err <= bound), (name, worst)
    lit = got["image"][..., :3].max(axis=2) > 0
    print("lit pixels", int(lit.sum()), "of", W * H)
    assert lit.any()  # the bound is not met by an image of zeros (the naive sampler lights about a quarter at 9 spp)
    for k in KEYS:
        assert got[k] == sum(v[k] for v in vs), k
