"""Are two builds of the library the same denoisers, bit for bit? Runs trace.denoise_image and
trace.denoise_guided_image over the test suite's shapes and parameter sets (tests/denoise_ref.py,
tests/denoise_guided_ref.py) with each library in a child process of its own, so the two are
never loaded together, writes every output as <out_dir>/<a|b>/<case>.npy and compares them on the
host by their uint32 view.
usage: python scripts/denoise_ab_bits.py <lib_a.so> <lib_b.so> <out_dir>
       python scripts/denoise_ab_bits.py --dump <lib.so> <dir>      (what each child runs)"""
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "julia-raytracer_amd"), str(ROOT / "tests")]


def dump(lib_path, out):
    import denoise_guided_ref as G
    import denoise_ref as R
    from jtrace import abi, trace
    lib = abi.load_library(lib_path)
    out.mkdir(parents=True, exist_ok=True)
    fields = ("iterations", "sigma_color", "sigma_normal", "sigma_albedo", "albedo_floor")
    for H, W in R.SHAPES:
        rgba, alb, nrm = R.synthetic(H, W)
        var = G.synthetic_variance(rgba, H, W)
        for p in R.parameter_sets(H, W):
            got = trace.denoise_image(rgba, alb, nrm, lib=lib, **{k: p[k] for k in fields})
            np.save(out / f"plain_{H}x{W}_it{p['iterations']}_sc{p['sigma_color']:g}.npy", got)
        for p in G.parameter_sets():
            got = trace.denoise_guided_image(rgba, var, alb, nrm, lib=lib, **p)
            np.save(out / f"guided_{H}x{W}_it{p['iterations']}_sv{p['sigma_variance']:g}.npy", got)


def main(lib_a, lib_b, out):
    for side, lib in (("a", lib_a), ("b", lib_b)):
        subprocess.run([sys.executable, __file__, "--dump", lib, str(out / side)], check=True)
    names = sorted(f.name for f in (out / "a").glob("*.npy"))
    assert names and names == sorted(f.name for f in (out / "b").glob("*.npy"))
    print(f"a = {lib_a}\nb = {lib_b}")
    differing = 0
    for name in names:
        a, b = (np.load(out / side / name) for side in "ab")
        words = int((a.view(np.uint32) != b.view(np.uint32)).sum()) if a.shape == b.shape else a.size
        differing += words > 0
        print(f"{name:40s} {a.shape[0]:3d}x{a.shape[1]:<3d} float32 words that differ: {words} of {a.size}")
    print(f"{len(names)} outputs, {differing} differ")
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--dump":
        dump(sys.argv[2], Path(sys.argv[3]))
    elif len(sys.argv) == 4:
        sys.exit(main(sys.argv[1], sys.argv[2], Path(sys.argv[3])))
    else:
        sys.exit(__doc__)
