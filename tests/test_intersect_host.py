"""Ray queries (include/jtrace.h: jt_intersect, jt_occluded and their device-pointer variants), the
part that needs no GPU: jt_hit's layout in the header against the ctypes and numpy mirrors, the four
exports, and the argument errors that are reported before the context is looked at."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from conftest import ROOT

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_intersect", "jt_occluded", "jt_intersect_device", "jt_occluded_device")


def test_jt_hit_layout_matches_header(abi, tmp_path):
    """The method of tests/test_abi.py test_struct_layouts_match_header, for jt_hit."""
    src = tmp_path / "sz.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("jt_hit %zu\\n", sizeof(jt_hit));']
    for f, _ in abi.jt_hit._fields_:
        lines.append(f'printf("jt_hit.{f} %zu\\n", offsetof(jt_hit, {f}));')
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l)
    assert int(got["jt_hit"]) == C.sizeof(abi.jt_hit) == abi.HIT_DTYPE.itemsize == 24
    assert [f for f, _ in abi.jt_hit._fields_] == list(abi.HIT_DTYPE.names) == ["instance", "element", "u", "v", "t", "hit"]
    for f, _ in abi.jt_hit._fields_:
        assert int(got[f"jt_hit.{f}"]) == getattr(abi.jt_hit, f).offset == abi.HIT_DTYPE.fields[f][1], f


def test_the_four_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5


def test_argument_errors_need_no_device(abi, lib):
    """NULL ctx, NULL arrays, n < 0 and n > 2^30 are JT_ERR_INVALID naming the argument, reported
    before the context is looked at: the handle below is no context and is never read. n == 0 with
    valid pointers is JT_OK."""
    rays = np.zeros((4, 6), np.float32)
    hits = np.zeros(4, abi.HIT_DTYPE)
    occ = np.zeros(4, np.uint8)
    rp, hp, op = rays.ctypes.data_as(abi.f32p), hits.ctypes.data_as(C.POINTER(abi.jt_hit)), occ.ctypes.data_as(abi.u8p)
    fake = C.c_void_p(0x10)  # not a context: these errors come first
    dev = C.c_void_p(0x1000)  # not a device pointer: never read either

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    assert "ctx" in err(lib.jt_intersect(None, 4, rp, None, hp))
    assert "ctx" in err(lib.jt_occluded(None, 4, rp, op))
    assert "ctx" in err(lib.jt_intersect_device(None, 4, dev, None, dev))
    assert "ctx" in err(lib.jt_occluded_device(None, 4, dev, dev))
    assert "rays" in err(lib.jt_intersect(fake, 4, None, None, hp))
    assert "hits" in err(lib.jt_intersect(fake, 4, rp, None, None))
    assert "rays" in err(lib.jt_occluded(fake, 4, None, op))
    assert "occluded" in err(lib.jt_occluded(fake, 4, rp, None))
    assert "d_rays" in err(lib.jt_intersect_device(fake, 4, None, None, dev))
    assert "d_hits" in err(lib.jt_intersect_device(fake, 4, dev, None, None))
    assert "d_rays" in err(lib.jt_occluded_device(fake, 4, None, dev))
    assert "d_occluded" in err(lib.jt_occluded_device(fake, 4, dev, None))
    for n in (-1, -2**40, 2**30 + 1):
        for msg in (err(lib.jt_intersect(fake, n, rp, None, hp)), err(lib.jt_occluded(fake, n, rp, op)),
                    err(lib.jt_intersect_device(fake, n, dev, None, dev)), err(lib.jt_occluded_device(fake, n, dev, dev))):
            assert re.search(r"\bn\b", msg), msg
    assert lib.jt_intersect(fake, 0, rp, None, hp) == 0 and lib.jt_occluded(fake, 0, rp, op) == 0
    assert lib.jt_intersect_device(fake, 0, dev, None, dev) == 0 and lib.jt_occluded_device(fake, 0, dev, dev) == 0
    assert (hits.view(np.uint8) == 0).all() and (occ == 0).all()
