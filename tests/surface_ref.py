"""The surface at a hit and the camera ray in float64 numpy, restated from the reference's
src/scene.jl (eval_camera :372, eval_position :435, eval_element_normal :578, eval_texcoord :753,
eval_color :690, eval_material :614) and src/geometry.jl / src/math.jl (interpolate_triangle,
interpolate_quad, triangle_normal, quad_normal, transform_point, transform_normal) — not from the
device code. Shared by tests/test_surface_host.py (CPU) and tests/test_gpu_surface.py.

Every function returns (value, A): A is, componentwise, the sum of the absolute values of the terms
that were added to form the value (1, u and v count as terms of the weight 1 - u - v), the scale a
float32 evaluation's rounding errors are relative to. For a normalised vector the value is the unit
vector, A is that sum before the last normalisation divided by the vector's length, and a third
item is the conditioning factor of the normalisations on the way (1 where there is none). For the
normals A is that of a vector whose every component is as large as its length (a cross product's
component is a difference of products of the whole edges): the frame's absolute column sums over
the transformed normal's length.

The material point's texture reads are exact float32 functions of the record's own texcoord;
material_point32 restates them in float32 with the oracle's eval_texture (oracle.probe_texture).
"""
import numpy as np

F32, F64 = np.float32, np.float64
MIN_ROUGHNESS = F32(0.03) * F32(0.03)  # src/scene.jl:46
TYPES = ["matte", "glossy", "reflective", "transparent", "refractive", "subsurface", "volumetric", "gltfpbr"]
EPS = 2.0 ** -24


def _frame(f):
    f = np.asarray(f, F64).reshape(4, 3)
    return f[:3], f[3]  # axes x, y, z as rows; origin


def _elements(shape):
    tri = len(shape.triangles) != 0
    return tri, np.asarray(shape.triangles if tri else shape.quads, np.int64)


def _tri_weights(u, v):
    """interpolate_triangle's weights and the absolute-term sums of each: w1 = 1 - u - v."""
    w = np.stack([1 - u - v, u, v], -1)
    a = np.stack([1 + np.abs(u) + np.abs(v), np.abs(u), np.abs(v)], -1)
    return w, a


def _interp(vals, idx, tri, u, v):
    """interpolate_triangle / interpolate_quad of the per-vertex rows vals[idx[:, k]] at the float32
    (u, v): (value, A). The quad's branch is taken on the float32 sum u + v, as the reference does."""
    u32, v32 = np.asarray(u, F32), np.asarray(v, F32)
    u, v = u32.astype(F64), v32.astype(F64)
    P = [np.asarray(vals, F64)[idx[:, k]] for k in range(idx.shape[1])]
    if tri:
        w, a = _tri_weights(u, v)
        sel = P[:3]
    else:
        first = (u32 + v32) <= F32(1)
        # second triangle (p3, p4, p2) at 1 - uv, the subtraction rounded to float32 as in the reference
        u2, v2 = (F32(1) - u32).astype(F64), (F32(1) - v32).astype(F64)
        w1, a1 = _tri_weights(u, v)
        w2, a2 = _tri_weights(u2, v2)
        w = np.where(first[:, None], w1, w2)
        a = np.where(first[:, None], a1, a2 + EPS * np.stack([2 * np.ones_like(u), np.ones_like(u), np.ones_like(u)], -1))
        sel = [np.where(first[:, None], P[0], P[2]), np.where(first[:, None], P[1], P[3]), np.where(first[:, None], P[3], P[1])]
    val = sum(sel[k] * w[:, k:k + 1] for k in range(3))
    A = sum(np.abs(sel[k]) * a[:, k:k + 1] for k in range(3))
    return val, A


def _per_instance(scene, inst, fn, width):
    out = [np.zeros((len(inst), width), F64) for _ in range(3)]
    for k in np.unique(inst):
        m = inst == k
        res = fn(scene.instances[k], scene.shapes[scene.instances[k].shape], m)
        for o, r in zip(out, res):
            o[m] = r
    return out


def position(scene, inst, elem, u, v):
    """eval_position: transform_point(frame, interpolate(positions)). (value, A)."""
    def fn(ins, shape, m):
        tri, idx = _elements(shape)
        p, a = _interp(shape.positions, idx[elem[m]], tri, u[m], v[m])
        ax, o = _frame(ins.frame)
        return p @ ax + o, a @ np.abs(ax) + np.abs(o), 0
    val, A, _ = _per_instance(scene, inst, fn, 3)
    return val, A


def _unit(x):
    """normalize (src/math.jl:71-78): a zero vector stays zero. (unit vector, length, 1 where zero)."""
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    n = np.where(n == 0, 1.0, n)
    return x / n, n


def element_normal(scene, inst, elem):
    """eval_element_normal: transform_normal(frame, triangle_normal / quad_normal) = normalize of
    the frame's axes times the unit normal. (value, A, cond): cond = |e1||e2| / |e1 x e2| of the
    triangle (for a quad the larger of its two triangles', times 2 / |n1 + n2|)."""
    def fn(ins, shape, m):
        tri, idx = _elements(shape)
        P = [np.asarray(shape.positions, F64)[idx[elem[m], k]] for k in range(idx.shape[1])]

        def tn(a, b, c):
            e1, e2 = b - a, c - a
            cr = np.cross(e1, e2)
            n, l = _unit(cr)
            zero = np.linalg.norm(cr, axis=-1, keepdims=True) == 0  # a degenerate triangle adds a zero normal
            return n, np.where(zero, 1.0, (np.linalg.norm(e1, axis=-1) * np.linalg.norm(e2, axis=-1))[:, None] / l)
        if tri:
            n, cond = tn(P[0], P[1], P[2])
        else:
            n1, c1 = tn(P[0], P[1], P[3])
            n2, c2 = tn(P[2], P[3], P[1])
            n, l = _unit(n1 + n2)
            cond = np.maximum(c1, c2) * 2 / l
        ax, _ = _frame(ins.frame)
        w, l = _unit(n @ ax)
        # a component of a cross product is a difference of two products of up to |e1||e2|: its error is
        # relative to that, not to the component, so after the division by |e1 x e2| every component
        # of the unit normal carries cond * 2^-24 relative to the vector's length 1, not to itself
        return w, (np.ones(3) @ np.abs(ax)) / l, np.broadcast_to(cond, w.shape)
    return _per_instance(scene, inst, fn, 3)


def has_vertex_normals(scene, inst):
    return np.array([scene.shapes[scene.instances[k].shape].normals is not None and
                     len(scene.shapes[scene.instances[k].shape].normals) != 0 for k in inst])


def vertex_normal(scene, inst, elem, u, v):
    """eval_normal of a shape with vertex normals (src/scene.jl:525-576), unflipped:
    transform_normal(frame, normalize(interpolate(normals))). (value, A, cond): cond is the
    interpolation's, sum |w_k n_k| / |sum w_k n_k| (its largest component ratio bound: the norms').
    Rows of shapes without vertex normals are zero."""
    def fn(ins, shape, m):
        k = int(m.sum())
        if shape.normals is None or len(shape.normals) == 0:
            return np.zeros((k, 3)), np.zeros((k, 3)), np.ones((k, 3))
        tri, idx = _elements(shape)
        n, a = _interp(shape.normals, idx[elem[m]], tri, u[m], v[m])
        nu, l = _unit(n)
        cond = np.linalg.norm(a, axis=-1, keepdims=True) / l
        ax, _ = _frame(ins.frame)
        w, lw = _unit(nu @ ax)
        return w, (np.ones(3) @ np.abs(ax)) / lw, np.broadcast_to(cond, w.shape)  # relative to the length, as above
    return _per_instance(scene, inst, fn, 3)


def texcoord(scene, inst, elem, u, v):
    """eval_texcoord: the interpolated texcoords, or uv where the shape has none. (value, A)."""
    def fn(ins, shape, m):
        if shape.texcoords is None or len(shape.texcoords) == 0:
            uv = np.stack([u[m], v[m]], -1).astype(F64)
            return uv, np.zeros_like(uv), 0
        tri, idx = _elements(shape)
        return (*_interp(shape.texcoords, idx[elem[m]], tri, u[m], v[m]), 0)
    val, A, _ = _per_instance(scene, inst, fn, 2)
    return val, A


def vertex_color(scene, inst, elem, u, v):
    """eval_color: the interpolated vertex colours, (1, 1, 1, 1) where the shape has none. (value, A)."""
    def fn(ins, shape, m):
        if shape.colors is None or len(shape.colors) == 0:
            return np.ones((int(m.sum()), 4)), np.zeros((int(m.sum()), 4)), 0
        tri, idx = _elements(shape)
        return (*_interp(shape.colors, idx[elem[m]], tri, u[m], v[m]), 0)
    val, A, _ = _per_instance(scene, inst, fn, 4)
    return val, A


def has_vertex_colors(scene, inst):
    return np.array([scene.shapes[scene.instances[k].shape].colors is not None and
                     len(scene.shapes[scene.instances[k].shape].colors) != 0 for k in inst])


def _texture32(oracle, scene, tex, tc, as_linear):
    """eval_texture(scene, tex, tc, as_linear) in float32 through the oracle, (n, 4)."""
    if tex < 0:
        return np.ones((len(tc), 4), F32)
    t = scene.textures[tex]
    pix = t.pixelsf if t.pixelsf is not None and np.size(t.pixelsf) else t.pixelsb
    pix = np.ascontiguousarray(pix).reshape(t.height, t.width, 4)
    q = np.concatenate([np.asarray(tc, F32), np.full((len(tc), 1), F32(as_linear))], 1)
    return oracle.probe_texture(pix, t.linear, q)


def material_point32(oracle, scene, inst, tc32, color_shp=None):
    """eval_material in float32 from the records' own float32 texcoords: dict of emission, color,
    opacity, metallic, roughness, ior, material, type. color_shp: the (n, 4) float32 vertex colour
    factor, None for (1, 1, 1, 1)."""
    n = len(inst)
    out = {"emission": np.zeros((n, 3), F32), "color": np.zeros((n, 3), F32), "opacity": np.zeros(n, F32),
           "metallic": np.zeros(n, F32), "roughness": np.zeros(n, F32), "ior": np.zeros(n, F32),
           "material": np.zeros(n, np.int32), "type": np.zeros(n, np.int32)}
    shp = np.ones((n, 4), F32) if color_shp is None else np.asarray(color_shp, F32)
    mats = np.array([scene.instances[k].material for k in inst])
    for mi in np.unique(mats):
        m = mats == mi
        mat = scene.materials[mi]
        tc = tc32[m]
        em = _texture32(oracle, scene, mat.emission_tex, tc, True)
        ct = _texture32(oracle, scene, mat.color_tex, tc, True)
        rt = _texture32(oracle, scene, mat.roughness_tex, tc, False)
        out["emission"][m] = np.asarray(mat.emission, F32) * em[:, :3]
        out["color"][m] = (np.asarray(mat.color, F32) * ct[:, :3]) * shp[m, :3]
        out["opacity"][m] = F32(mat.opacity) * ct[:, 3] * shp[m, 3]
        out["metallic"][m] = F32(mat.metallic) * rt[:, 2]
        r = F32(mat.roughness) * rt[:, 1]
        r = r * r
        if mat.type in ("matte", "gltfpbr", "glossy"):
            r = np.clip(r, MIN_ROUGHNESS, F32(1))
        elif mat.type == "volumetric":
            r = np.zeros_like(r)
        else:
            r = np.where(r < MIN_ROUGHNESS, F32(0), r)
        out["roughness"][m] = r
        out["ior"][m] = F32(mat.ior)
        out["material"][m] = mi
        out["type"][m] = TYPES.index(mat.type)
    return out


def sample_disk(ruv):
    """sample_disk (src/sampling.jl:12-16): sqrt(r.y) * (cos, sin)(2 pi r.x). (value, A): the angle
    phi = 2 pi r.x is itself a rounded float32, and cos and sin move by up to its error whatever their
    own size, so a component's A is r * (|cos or sin| + phi), not r * |cos or sin|."""
    r, phi = np.sqrt(ruv[:, 1]), 2 * np.pi * ruv[:, 0]
    val = np.stack([np.cos(phi) * r, np.sin(phi) * r], -1)
    return val, np.abs(val) + (r * phi)[:, None]


def tent(p):
    """The tent filter's offset of one draw (src/trace.jl:651-674): width 2, offset 0.5."""
    return 2.0 * np.where(p < 0.5, np.sqrt(2 * p) - 1, 1 - np.sqrt(2 - 2 * p)) + 0.5


def image_uv(width, height, draws=None, tentfilter=False):
    """The image uv of every pixel, row-major: the pixel centre (draws None), or (i + puv) / size
    from the sample's first two draws, through the tent filter where the context has it."""
    k = np.arange(width * height)
    i, j = (k % width).astype(F64), (k // width).astype(F64)
    if draws is None:
        return np.stack([(i + 0.5) / width, (j + 0.5) / height], -1)
    p = np.asarray(draws, F64)[:, :2]
    if tentfilter:
        p = tent(p)
    return np.stack([(i + p[:, 0]) / width, (j + p[:, 1]) / height], -1)


def eval_camera(cam, uv, lens_uv, aspect=None, lens_A=None):
    """eval_camera (src/scene.jl:372-411) for image uv (n, 2) and lens uv (n, 2) (lens_A: the lens
    uv's own absolute-term sums, sample_disk's; |lens_uv| when None):
    (o, A_o, d, A_d) with d the unit direction and A_d relative to it. The absolute-term sums are
    carried from the film point on: q's (0.5 and uv are terms of 0.5 - uv), through the normalised
    lens-centre direction to the focus point p, then p - e and the frame."""
    aspect = F64(cam.aspect if aspect is None else aspect)
    film = (F64(cam.film), F64(cam.film) / aspect) if aspect >= 1 else (F64(cam.film) * aspect, F64(cam.film))
    lens, focus, ap = F64(cam.lens), F64(cam.focus), F64(cam.aperture)
    n = len(uv)
    le = np.stack([lens_uv[:, 0] * ap / 2, lens_uv[:, 1] * ap / 2, np.zeros(n)], -1)
    lens_A = np.abs(lens_uv) if lens_A is None else lens_A
    a_le = np.stack([lens_A[:, 0] * ap / 2, lens_A[:, 1] * ap / 2, np.zeros(n)], -1)
    s = 1 / lens if cam.orthographic else 1.0
    q = np.stack([film[0] * (0.5 - uv[:, 0]) * s, film[1] * (uv[:, 1] - 0.5) * s, np.full(n, lens)], -1)
    a_q = np.stack([film[0] * (0.5 + np.abs(uv[:, 0])) * s, film[1] * (np.abs(uv[:, 1]) + 0.5) * s, np.full(n, lens)], -1)
    if not cam.orthographic:
        dc, lq = _unit(q)
        dc = -dc
        e, a_e = le, a_le
        p = dc * focus / np.abs(dc[:, 2:3])
        a_p = (a_q / lq) * focus / np.abs(dc[:, 2:3])
    else:
        flat = np.stack([-q[:, 0], -q[:, 1], np.zeros(n)], -1)
        e, a_e = flat + le, a_le + np.stack([a_q[:, 0], a_q[:, 1], np.zeros(n)], -1)
        p = np.stack([-q[:, 0], -q[:, 1], np.full(n, -focus)], -1)
        a_p = np.stack([a_q[:, 0], a_q[:, 1], np.full(n, focus)], -1)
    d, ld = _unit(p - e)
    a_local = (a_p + a_e) / ld  # the terms of p - e, relative to the unit vector
    ax, o = _frame(cam.frame)
    w, lw = _unit(d @ ax)
    return e @ ax + o, a_e @ np.abs(ax) + np.abs(o), w, (a_local @ np.abs(ax)) / lw


# ------------------------------------------------------------------------------ the test scenes
W, H = 67, 45  # an odd pixel count (3015): the last wave of a launch is partial
# name -> (scene, jt_params fields, library options). tests/test_surface_host.py checks the groups on
# the CPU. OPAQUE: every material opacity is 1 and the scene has neither colour textures nor vertex
# colours, so every record's opacity is exactly 1, the integrator never passes through a first hit
# and no pixel is excluded. ROUNDED: every source is 1 too (texel alphas 255, vertex alphas 1), but
# an alpha is interpolated: the bilinear weights of eval_texture and the barycentric weights of
# eval_color are rounded values that need not sum to 1, so a record's opacity can be a few ulp below
# 1 (the reference's own arithmetic; the integrator then draws against it). Such a pixel is excluded
# and its opacity asserted to be at least ROUNDED_MIN. OPACITY: a source below 1.
OPAQUE = ("cornell", "cornell_hbm", "random", "quads9", "tent", "lens", "ortho", "naive")
ROUNDED = ("features1", "materials4", "shapes1", "vcolor")
OPACITY = ("coplanar", "materials2")
# ((a + b) + c) + d of four products of two rounded factors each, all of alpha 1: at most 3 roundings per
# term and 3 of the sums, each at most 2^-24 relative to a value of at most 1 (a vertex alpha's
# (1 - u - v) + u + v has fewer), times the product with the other alpha
ROUNDED_MIN = 1 - 15 * EPS
ALL_ORDERS = ("cornell", "random", "quads9", "coplanar")  # the small scenes: all three traversal orders


def case(name):
    """(scene, params keywords, options) of a test scene."""
    import copy
    import warnings
    from pathlib import Path
    import scenes_ref as SR
    from jtrace import sceneio
    root = Path(__file__).resolve().parent.parent / "assets" / "scenes"

    def shipped(n):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return sceneio.load_scene(str(root / n / f"{n}.json"), missing="drop")
    kw, opts = {}, {}
    if name in ("features1", "materials4", "materials2", "shapes1"):
        sc = shipped(name)
    elif name == "random":
        sc = SR.random_instanced_scene()
    elif name == "quads9":
        sc = SR.quad_scene(9, False, SR.SEEDS[9])
    else:
        sc = copy.deepcopy(shipped("cornellbox"))
        if name == "cornell_hbm":
            opts = {"lds_scene": 0}
        elif name == "coplanar":
            sc = SR.coplanar_tie_scene(sc)
        elif name == "vcolor":  # tests/test_gpu_variants.py's vertex colours, every alpha 1
            rng = np.random.default_rng(7)
            for s in sc.shapes:
                col = rng.uniform(0.2, 1.0, size=(len(s.positions), 4)).astype(F32)
                col[:, 3] = 1.0
                s.colors = col
        elif name == "tent":
            kw = {"tentfilter": True}
        elif name == "lens":
            sc.cameras[0].aperture = F32(0.25)
        elif name == "ortho":
            sc.cameras[0].orthographic = True
            sc.cameras[0].lens = F32(0.02)
        elif name == "naive":
            kw = {"sampler": 2}
        else:
            assert name == "cornell", name
    return sc, kw, opts


def has_interpolated_alpha(scene):
    """A colour texture or vertex colours: an alpha that eval_material interpolates."""
    return any(m.color_tex >= 0 for m in scene.materials) or any(s.colors is not None and len(s.colors) for s in scene.shapes)


def opacity_sources(scene):
    """The smallest material opacity, colour-texture alpha (as a float) and vertex-colour alpha of a scene."""
    lo = min(float(m.opacity) for m in scene.materials)
    for m in scene.materials:
        if m.color_tex >= 0:
            t = scene.textures[m.color_tex]
            if t.pixelsf is not None and np.size(t.pixelsf):
                lo = min(lo, float(np.asarray(t.pixelsf).reshape(-1, 4)[:, 3].min()))
            else:
                lo = min(lo, float(np.asarray(t.pixelsb).reshape(-1, 4)[:, 3].min()) / 255.0)
    for s in scene.shapes:
        if s.colors is not None and len(s.colors):
            lo = min(lo, float(np.asarray(s.colors)[:, 3].min()))
    return lo
