"""bench.py's host-side helpers on the CPU: the SURVEY §8(d) algorithmic bytes, the shading-record
size, and the roofline-record lookup, which must only ever pick a record of the running build and
workload (a record of other code describes other counts)."""
import json
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402  (no torch, no library at import)


def test_algorithmic_bytes_per_unit():
    c = {"nodes": 10, "instances": 3, "prims": 4, "shades": 2}
    # 32 B per binary pop, 64 B per instance visit, 48 B per triangle test, shade bytes per hit
    assert bench.algorithmic_bytes(c, 240, False) == 32 * 10 + 64 * 3 + 48 * 4 + 240 * 2
    # a wide-record visit is 64 B; quad scenes test 64-B quads
    assert bench.algorithmic_bytes(c, 240, True, wide=True) == 64 * 10 + 64 * 3 + 64 * 4 + 240 * 2


def test_shade_record_bytes_cornellbox(cornell_abi):
    from jtrace import sceneio
    scene = sceneio.load_scene(str(ROOT / "assets" / "scenes" / "cornellbox" / "cornellbox.json"))
    assert bench.shade_record_bytes(scene) == 240  # 64 + 32 + 16 + 80 + 3 x 16


@pytest.mark.parametrize("name", ["cb", "cb_n8", "f2", "b1", "ec"])
def test_committed_records_match_only_their_build(name):
    rec = json.loads((ROOT / "profiles" / "r04_roofline" / f"{name}_final.json").read_text())
    found, src = bench.roofline_record(rec["workload"], rec["kernel"], rec["build"])
    assert found is not None and found["build"] == rec["build"] and src.startswith("profiles/")
    assert bench.roofline_record(rec["workload"], rec["kernel"], "0" * 16) == (None, None)
    assert bench.roofline_record(rec["workload"] + " x", rec["kernel"], rec["build"]) == (None, None)


def test_timed_kernel_is_the_production_instance(tmp_path, monkeypatch):
    """The profiler names a trace kernel with seven template arguments, the last one ADAPT. The
    timed kernel is the production instance (COUNT 0, ADAPT false) whatever time an adapted
    context's instance or a counting instance took, and its record carries jt_describe's
    six-argument name, by which bench.py finds it."""
    sys.path.insert(0, str(ROOT / "scripts"))
    import roofline

    args = "(jtd::DScene, jtd::DParams, int, int, jtk::DAccum)"
    stats = tmp_path / "kernel_stats.csv"
    stats.write_text(
        '"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
        f'"void jtk::trace_kernel_lds<1, 16, false, 0, 8192, false, false>{args}",2,2000,1000.0,20.0,900,1100,100.0\n'
        f'"void jtk::trace_kernel_lds<1, 16, false, 0, 8192, false, true>{args}",3,6000,2000.0,60.0,1900,2100,100.0\n'
        f'"void jtk::trace_kernel_lds<1, 16, false, 1, 8192, false, false>{args}",1,3000,3000.0,30.0,3000,3000,0.0\n')
    kernel, avg_ns, calls = roofline.timed_kernel(str(stats))
    assert (kernel, avg_ns, calls) == ("trace_kernel_lds<1, 16, false, 0, 8192, false>", 1000.0, 2)

    rec = {"workload": "w", "kernel": kernel, "build": "0123456789abcdef"}
    (tmp_path / "profiles" / "x_roofline").mkdir(parents=True)
    (tmp_path / "profiles" / "x_roofline" / "w.json").write_text(json.dumps(rec))
    monkeypatch.setattr(bench, "ROOT", tmp_path)
    desc = "kernel=trace_kernel_lds<1,16,false,0,8192,false> mode=lds scene_lds_bytes=7648"
    found, src = bench.roofline_record("w", desc.split()[0].split("=", 1)[1], rec["build"])
    assert found == rec and src == "profiles/x_roofline/w.json"
