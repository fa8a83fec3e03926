"""The surface calls (include/jtrace.h: jt_eval_hits, jt_camera_rays, jt_gbuffer and their
device-pointer variants), the part that needs no GPU: jt_surface's layout in the header against the
ctypes and numpy mirrors, the six exports, the argument errors that are reported before the context
is looked at, the float64 restatement tests/surface_ref.py against facts it must satisfy, and the
opacity of the GPU tests' scenes (tests/test_gpu_surface.py excludes no pixel on the opaque ones)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import surface_ref as R
from conftest import ROOT, make_params

HEADER = ROOT / "include" / "jtrace.h"
NAMES = ("jt_eval_hits", "jt_camera_rays", "jt_gbuffer", "jt_eval_hits_device", "jt_camera_rays_device", "jt_gbuffer_device")
FIELDS = ["position", "normal", "gnormal", "texcoord", "opacity", "color", "roughness", "emission", "metallic", "material",
          "type", "ior", "hit"]


def test_jt_surface_layout_matches_header(abi, tmp_path):
    src = tmp_path / "sz.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("jt_surface %zu\\n", sizeof(jt_surface));']
    for f, _ in abi.jt_surface._fields_:
        lines.append(f'printf("jt_surface.{f} %zu\\n", offsetof(jt_surface, {f}));')
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l)
    assert int(got["jt_surface"]) == C.sizeof(abi.jt_surface) == abi.SURFACE_DTYPE.itemsize == 96
    assert [f for f, _ in abi.jt_surface._fields_] == list(abi.SURFACE_DTYPE.names) == FIELDS
    for f, _ in abi.jt_surface._fields_:
        assert int(got[f"jt_surface.{f}"]) == getattr(abi.jt_surface, f).offset == abi.SURFACE_DTYPE.fields[f][1], f
    # the header's field order, read from its text
    text = HEADER.read_text()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct jt_surface"):text.index("} jt_surface;")], flags=re.S)
    assert re.findall(r"\b(?:float|int32_t)\s+([a-z]+)", body) == FIELDS


def test_the_six_names_are_declared_mirrored_and_exported(abi, lib):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", str(Path(lib._name))], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b[TW] (jt_[a-z_]+)\b", out))
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in abi.EXPORTED_SYMBOLS and name in exported, name
    assert lib.jt_abi_version() == 5


def test_argument_errors_need_no_device(abi, lib):
    """NULL ctx, NULL arrays, n < 0, n > 2^30 and sample < -1 are JT_ERR_INVALID naming the argument,
    reported before the context is looked at: the handle below is no context and is never read.
    n == 0 with valid pointers is JT_OK."""
    rays = np.zeros((4, 6), np.float32)
    hits = np.zeros(4, abi.HIT_DTYPE)
    surf = np.zeros(4, abi.SURFACE_DTYPE)
    rp, hp = rays.ctypes.data_as(abi.f32p), hits.ctypes.data_as(C.POINTER(abi.jt_hit))
    sp = surf.ctypes.data_as(C.POINTER(abi.jt_surface))
    fake = C.c_void_p(0x10)
    dev = C.c_void_p(0x1000)

    def err(status):
        assert status == -1, status
        return lib.jt_last_error().decode()

    assert "ctx" in err(lib.jt_eval_hits(None, 4, rp, hp, sp))
    assert "ctx" in err(lib.jt_eval_hits_device(None, 4, dev, dev, dev))
    assert "ctx" in err(lib.jt_camera_rays(None, 0, rp)) and "ctx" in err(lib.jt_camera_rays_device(None, 0, dev))
    assert "ctx" in err(lib.jt_gbuffer(None, 0, rp, hp, sp)) and "ctx" in err(lib.jt_gbuffer_device(None, 0, dev, dev, dev))
    assert "rays" in err(lib.jt_eval_hits(fake, 4, None, hp, sp))
    assert "hits" in err(lib.jt_eval_hits(fake, 4, rp, None, sp))
    assert "out" in err(lib.jt_eval_hits(fake, 4, rp, hp, None))
    assert "d_rays" in err(lib.jt_eval_hits_device(fake, 4, None, dev, dev))
    assert "d_hits" in err(lib.jt_eval_hits_device(fake, 4, dev, None, dev))
    assert "d_out" in err(lib.jt_eval_hits_device(fake, 4, dev, dev, None))
    assert "rays" in err(lib.jt_camera_rays(fake, 0, None)) and "d_rays" in err(lib.jt_camera_rays_device(fake, 0, None))
    assert "surfaces" in err(lib.jt_gbuffer(fake, 0, rp, hp, None))
    assert "d_surfaces" in err(lib.jt_gbuffer_device(fake, 0, dev, dev, None))
    for n in (-1, -2**40, 2**30 + 1):
        for msg in (err(lib.jt_eval_hits(fake, n, rp, hp, sp)), err(lib.jt_eval_hits_device(fake, n, dev, dev, dev))):
            assert re.search(r"\bn\b", msg), msg
    for s in (-2, -2**31):
        for msg in (err(lib.jt_camera_rays(fake, s, rp)), err(lib.jt_camera_rays_device(fake, s, dev)),
                    err(lib.jt_gbuffer(fake, s, rp, hp, sp)), err(lib.jt_gbuffer_device(fake, s, dev, dev, dev))):
            assert "sample" in msg, msg
    # a misaligned device pointer: also before the context is looked at
    for args in ((0x1000, 0x1004, 0x1000), (0x1000, 0x1000, 0x1008), (0x1002, 0x1000, 0x1000)):
        assert "aligned" in err(lib.jt_eval_hits_device(fake, 4, *args))
    assert "aligned" in err(lib.jt_camera_rays_device(fake, 0, 0x1004))
    for args in ((0x1004, None, 0x1000), (None, 0x1004, 0x1000), (None, None, 0x1008)):
        assert "aligned" in err(lib.jt_gbuffer_device(fake, 0, *args))
    assert lib.jt_eval_hits(fake, 0, rp, hp, sp) == 0 and lib.jt_eval_hits_device(fake, 0, dev, dev, dev) == 0
    assert (surf.view(np.uint8) == 0).all() and (rays == 0).all()


def test_reference_positions_normals_and_texcoords():
    """tests/surface_ref.py on facts that need no device: at an element's corners the position is the
    transformed vertex; the element normal is a unit vector orthogonal to the transformed edges of
    a rigid frame; a quad's two branches agree along its diagonal; A bounds the value."""
    sc, _, _ = R.case("random")
    for k, ins in enumerate(sc.instances):
        shape = sc.shapes[ins.shape]
        tri, idx = R._elements(shape)
        n = len(idx)
        inst, elem = np.full(n, k), np.arange(n)
        ax, o = R._frame(ins.frame)
        world = np.asarray(shape.positions, np.float64) @ ax + o
        corners = ((0, 0, 0), (1, 0, 1), (0, 1, 2)) if tri else ((0, 0, 0), (1, 0, 1), (1, 1, 2), (0, 1, 3))
        for u, v, c in corners:
            p, A = R.position(sc, inst, elem, np.full(n, u, np.float32), np.full(n, v, np.float32))
            assert np.allclose(p, world[idx[:, c]], rtol=0, atol=1e-12), (k, u, v)
            assert (np.abs(p) <= A + 1e-12).all()
        g, A, cond = R.element_normal(sc, inst, elem)
        assert np.allclose(np.linalg.norm(g, axis=1), 1) and (cond >= 1 - 1e-12).all() and (np.abs(g) <= A + 1e-12).all()
        if not tri:  # along the diagonal p2-p4 (u + v = 1) both triangles interpolate the same point
            u = np.linspace(0.1, 0.9, n).astype(np.float32)
            v = (np.float32(1) - u).astype(np.float32)
            lo, _ = R.position(sc, inst, elem, u, v)
            hi, _ = R.position(sc, inst, elem, u, np.nextafter(v, np.float32(2)))
            assert np.allclose(lo, hi, atol=1e-5)
        tc, _ = R.texcoord(sc, inst, elem, np.full(n, 0.25, np.float32), np.full(n, 0.5, np.float32))
        assert np.array_equal(tc, np.tile([0.25, 0.5], (n, 1)))  # no texcoords: uv itself


def test_reference_hit_points_lie_on_the_rays(abi, oracle):
    """The float64 position of the oracle's hit records is the point o + t d of their rays, to the
    float32 error of t: the restatement and or_query agree on which surface point a record names."""
    import queries_ref as Q
    for name in ("cornell", "random", "quads9"):
        ctx = Q.context(name, abi, oracle)
        r = Q.rays(ctx, "generic", oracle)
        q = oracle.query(ctx.sa, ctx.bvh, ctx.params["reference"], r)
        m = q["hit"] != 0
        p, A = R.position(ctx.scene, q["inst"][m], q["elem"][m], q["u"][m], q["v"][m])
        want = r[m, :3].astype(np.float64) + q["t"][m, None].astype(np.float64) * r[m, 3:].astype(np.float64)
        scale = np.abs(r[m, :3]).max(1) + np.abs(q["t"][m]) + A.max(1)
        assert m.sum() > 100 and (np.abs(p - want).max(1) <= 1e-4 * scale).all(), name


def test_reference_camera():
    """eval_camera in float64: the centre pixel of an odd image looks down the frame's -z axis from
    its origin; every direction is a unit vector; an orthographic camera's directions are all -z."""
    sc, _, _ = R.case("cornell")
    cam = sc.cameras[0]
    uv = R.image_uv(R.W, R.H)
    o, Ao, d, Ad = R.eval_camera(cam, uv, np.zeros_like(uv), aspect=np.float32(R.W) / np.float32(R.H))
    ax, org = R._frame(cam.frame)
    centre = (R.H // 2) * R.W + R.W // 2
    assert np.allclose(d[centre], -ax[2] / np.linalg.norm(ax[2])) and np.allclose(o, org) and np.allclose(np.linalg.norm(d, axis=1), 1)
    assert (np.abs(d) <= Ad + 1e-12).all() and (np.abs(o) <= Ao + 1e-12).all()
    sc, _, _ = R.case("ortho")
    o, _, d, _ = R.eval_camera(sc.cameras[0], uv, np.zeros_like(uv), aspect=np.float32(R.W) / np.float32(R.H))
    assert np.allclose(d, -ax[2] / np.linalg.norm(ax[2])) and np.ptp(o, axis=0).max() > 0.1
    # the tent filter maps [0, 1) onto [-1.5, 2.5), 0.5 to 0.5
    assert R.tent(np.array([0.5]))[0] == 0.5 and R.tent(np.array([0.0]))[0] == -1.5


@pytest.mark.parametrize("name", R.OPAQUE + R.ROUNDED + R.OPACITY)
def test_scene_opacity_groups(name):
    """Nothing on an OPAQUE scene lowers an opacity below 1 (material opacity 1, no colour texture,
    no vertex colours): the integrator never passes through a first hit there, so the G-buffer tests
    exclude no pixel. A ROUNDED scene's sources are all 1 too, but it interpolates an alpha (colour
    textures of alpha 255, vertex alphas of 1). The OPACITY scenes really have a source below 1."""
    sc, _, _ = R.case(name)
    lo, tex = R.opacity_sources(sc), R.has_interpolated_alpha(sc)
    print(name, "smallest opacity source", lo, "interpolated alpha", tex)
    if name in R.OPAQUE:
        assert lo == 1.0 and not tex, (name, lo, tex)
    elif name in R.ROUNDED:
        assert lo == 1.0 and tex, (name, lo, tex)
    else:
        assert lo < 1.0, (name, lo)


def test_interpolated_alpha_of_an_opaque_texture_can_round_below_one(oracle):
    """Why ROUNDED is a group of its own: the reference's eval_texture of a texture whose every alpha
    is 255 returns alphas a few ulp below 1 at some uv (its bilinear weights are rounded products),
    never below ROUNDED_MIN and never above 1 + the same."""
    pix = np.full((4, 4, 4), 255, np.uint8)
    rng = np.random.default_rng(5)
    q = np.concatenate([rng.uniform(0, 1, size=(20000, 2)), np.ones((20000, 1))], 1).astype(np.float32)
    a = oracle.probe_texture(pix, False, q)[:, 3]
    print("alpha of an all-255 texture: min", a.min(), "below 1:", int((a < 1).sum()), "of", len(a))
    assert (a < 1).any() and a.min() >= R.ROUNDED_MIN and a.max() <= 2 - R.ROUNDED_MIN
