"""The trace kernels' per-lane work item (csrc/jt_plan.h), enumerated on the CPU.

A lane's item holds its pixel's image coordinates, (j << 16) | i; the sample start decodes the pixel
from it and the item's store derives its launch slot from it by multiply-adds and the host's
reciprocal of the tile stride. tests/item_coords_check.cpp is a stand-alone program (its own main,
nothing loaded into Python) that checks, for widths and heights {1, 7, 8, 9, 13, 64, 70} and tile
shares (stride, offset) of {(1, 0), (2, 1), (3, 2)}, that every pixel encodes to an item, that the
item's decoded pixel and slot agree with slot_pixel, and that the slots are a bijection onto the
launch's slots inside the image. It is built here with the host compiler under the address and
undefined-behaviour sanitizers and run once, as tests/test_plan.py does for the rest of jt_plan.h.
"""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_item_coordinates_and_slots(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "item_coords_check"
    # -ffp-contract=off: the slot's multiply and add stay two roundings, as in the library's build
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    str(ROOT / "tests" / "item_coords_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stderr
    assert " 0 bad" in run.stdout
