"""bench.py end to end on the GPU at a tiny size: a plain run times exactly --steps steps, leaves
the --full legs out of its line, and --dump-outputs writes the image a caller of the timed path
holds after its last step (bitwise what the same render gives through the Python surface)."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT

pytestmark = pytest.mark.gpu

SIZE = ["--width", "64", "--height", "48", "--spp", "8"]


def run_bench(*extra):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        *SIZE, *extra], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [s for s in p.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_image(gpu, tmp_path, abi, lib, cornell_abi):
    from jtrace import trace
    from jtrace.cli import Params
    line = run_bench("--dump-outputs", str(tmp_path / "d"))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    for leg in ("roofline", "reference_order", "image_check", "cpu_baseline"):
        assert line[leg] is None, leg
    img = np.load(tmp_path / "d" / "image.npy")
    cnt = np.load(tmp_path / "d" / "counters.npy")
    assert img.dtype == np.float32 and img.shape == (48, 64, 4)
    assert cnt.dtype == np.float64 and cnt[0] == 64 * 48 * 8
    # value = rays of the timed steps over their time: the dumped step's ray count ties the two
    # (ms_per_step is rounded to a microsecond: up to 0.5 % of a step of 0.1 ms or more)
    assert line["ms_per_step"] >= 0.1
    assert line["value"] == pytest.approx(cnt[1] / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    # the same render through the Python surface, in this process
    params = abi.make_params(Params(scene=CORNELL, samples=8, sampler=1, width=64, height=48, batch=8), 0)
    bvh = trace.make_scene_bvh(cornell_abi, False, lib)
    lights = trace.make_trace_lights(cornell_abi, lib)
    st = trace.make_trace_state(cornell_abi, bvh, lights, params, lib)
    st.trace_range(0, 8)
    ref = st.get_image()
    rays = st.counters()["rays"]
    st.close()
    assert np.array_equal(img, ref)
    assert cnt[1] == rays


def test_full_run_fills_the_legs(gpu):
    line = run_bench("--full", "--cpu-spp", "2")
    assert line["full"] is True and line["steps"] == 3
    assert line["roofline"]["per_ray"]["nodes"] > 0
    assert line["reference_order"]["pixels_differing_from_near"] == 0.0  # cornellbox: bit-identical orders
    cpu = line["cpu_baseline"]  # the bench's own bound: a libm ulp may flip a rare path
    assert abs(cpu["rays"] - cpu["gpu_rays_same_samples"]) <= 1e-3 * cpu["rays"]
    assert line["image_check"]["key"].startswith("cornellbox path 64x48x8spp")
