"""Adversarial curve sets for the curve BLAS (pieces, capsules, split depths), the ribbon test and every curve walk, shared by the
CPU suite (the host's view of the BLAS against the oracle's per-curve test) and the GPU suite (trace and frames against the oracle).

There is no way to hand-build curves in the scene language (CurveGeneratorProcedure grows fur on a mesh), so a stock fur scene is
prepared and the arrays of its ONE curve set are overwritten in the flat scene description (include/fj_scene_desc.h) that the device
core and the oracle both read: CurveScene below.  Plain numpy with fixed seeds; every family is a few lines.
"""
import ctypes as C
import zlib

import numpy as np

from fujiyama_renderer_amd import gpu, host, workloads

SEED = 20261020
CENTRE = np.array([0.0, 0.15, 0.0])       # the furball of the stock scene is a sphere of radius .12 around (0, .13, 0)
SPREAD = 0.2
FUR_W = (0.003, 0.0001)                   # CurveGeneratorProcedure's root and tip widths
FAR = np.array([600.0, -500.0, 640.0])    # |FAR| ~ 1e3: an f32 ulp there (6e-5) is comparable to a ribbon radius
FAR_X0 = np.array([0.0, -780.0, 640.0])

# (rotate, scale factors) of tests/test_light_hull_cpu.py: rotated, non-uniformly scaled, mirrored -- and the identity
XFORMS = {"identity": ((0, 0, 0), (1, 1, 1)), "rotated": ((20, -35, 10), (1, 1, 1)), "nonuniform": ((0, 25, -15), (1, .4, 2.5)),
          "mirrored": ((10, 40, 0), (-1, 1, .7))}


# ------------------------------------------------------------------------------------------- the scene description in ctypes
class _Xf(C.Structure):
    _fields_ = [("transform_order", C.c_int32), ("rotate_order", C.c_int32), ("n", C.c_int32 * 3), ("_pad", C.c_int32),
                ("translate", (C.c_double * 4) * 8), ("rotate", (C.c_double * 4) * 8), ("scale", (C.c_double * 4) * 8)]


class _Curve(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_curves", C.c_int32), ("P", C.c_void_p), ("width", C.c_void_p), ("Cd", C.c_void_p),
                ("uv", C.c_void_p), ("velocity", C.c_void_p), ("indices", C.c_void_p), ("bounds", C.c_double * 6)]


class _Inst(C.Structure):
    _fields_ = [("primset_type", C.c_int32), ("primset", C.c_int32), ("n_shaders", C.c_int32), ("shaders", C.c_int32 * 8),
                ("reflect_target", C.c_int32), ("refract_target", C.c_int32), ("shadow_target", C.c_int32), ("xform", _Xf)]


class _Scene(C.Structure):
    _fields_ = [("n", C.c_int32 * 7), ("target_group", C.c_int32), ("meshes", C.c_void_p), ("curves", C.POINTER(_Curve)),
                ("textures", C.c_void_p), ("shaders", C.c_void_p), ("lights", C.c_void_p), ("instances", C.POINTER(_Inst)),
                ("groups", C.c_void_p)]


def compute_bounds(P, width, indices, velocity=None):
    """Curve::ComputeBounds (reference src/fj_curve.cc:126-149): per curve the box of its four control points widened by ITS larger
    end radius, merged with the same box at time 1 (get_primitive_bounds, :244-257), all merged, then widened by the set's largest
    radius -- in this order of operations"""
    lo, hi, rmax = np.full(3, np.finfo(np.float64).max), np.full(3, -np.finfo(np.float64).max), 0.0
    for i0 in indices:
        cp = P[i0:i0 + 4]
        r = .5 * max(width[i0], width[i0 + 3])
        lo, hi = np.minimum(lo, cp.min(axis=0) - r), np.maximum(hi, cp.max(axis=0) + r)
        if velocity is not None:
            ce = cp + 1.0 * velocity[i0:i0 + 4]
            lo, hi = np.minimum(lo, ce.min(axis=0) - r), np.maximum(hi, ce.max(axis=0) + r)
        rmax = max(rmax, r)
    return np.concatenate([lo - rmax, hi + rmax])


def grid_of(bounds, n_curves):
    """(n [3], cell [3], padded bounds [6]) of the reference grid over a curve set (compute_grid_cellsizes,
    src/fj_grid_accelerator.cc:318-332, as BuildCurveSet restates it)"""
    b = np.concatenate([bounds[:3] - .0001, bounds[3:] + .0001])
    size = b[3:] - b[:3]
    per_unit = 3 * np.power(float(n_curves), 1. / 3) / size.max()
    n = np.clip(np.floor(size * per_unit + .5).astype(np.int64), 1, 512)
    return n, (b[3:] - b[:3]) / n, b


def instance_matrix(xform, translate=(0, 0, 0)):
    """object-to-world matrix [4, 4] and its inverse of a static instance, by the core's own fjgpu_host_make_transform (SRT, ZXY)"""
    rot, fac = XFORMS[xform]
    trs = np.array(list(translate) + list(rot) + list(fac), dtype=np.float64)
    M, Mi = np.empty(16), np.empty(16)
    gpu.lib().fjgpu_host_make_transform(0, 10, trs.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), Mi.ctypes.data_as(C.c_void_p))
    return M.reshape(4, 4), Mi.reshape(4, 4)


class CurveScene(object):
    """the stock fur scene (workloads.furry on the "furball", `nlights` point lights) with its one curve set replaced by `curves`
    = dict(P [n, 3], width [n], Cd [n, 3], indices [m], velocity [n, 3] or None) and, optionally, the curve instance's static
    transform set to XFORMS[xform] and `translate`.  .sp is the scene pointer for gpu.Scene and oracle_ffi.OracleScene alike, .rd
    the render description.  The arrays live as long as this object; the host keeps ONE scene: the next CurveScene (or
    run_scene_text) invalidates this one."""

    def __init__(self, asset_dir, curves, xform="identity", translate=(0, 0, 0), nlights=1, res=(48, 32), spp=(2, 2)):
        text = workloads.furry(asset_dir, res=res, spp=spp, mesh="furball", nlights=nlights)
        host.run_scene_text(text, deferred=True)
        self.sp, self.rd = host.get_desc()
        d = C.cast(self.sp, C.POINTER(_Scene)).contents
        assert d.n[1] == 1, "one curve set"
        self.n_groups, self.target_group = int(d.n[6]), int(d.target_group)
        self.P = np.ascontiguousarray(curves["P"], dtype=np.float64)
        self.width = np.ascontiguousarray(curves["width"], dtype=np.float64)
        self.Cd = np.ascontiguousarray(curves["Cd"], dtype=np.float32)
        self.indices = np.ascontiguousarray(curves["indices"], dtype=np.int32)
        vel = curves.get("velocity")
        self.velocity = None if vel is None else np.ascontiguousarray(vel, dtype=np.float64)
        n = self.P.shape[0]
        assert self.P.shape == (n, 3) and self.width.shape == (n,) and self.Cd.shape == (n, 3)
        assert self.indices.min() >= 0 and self.indices.max() + 3 < n
        assert self.velocity is None or self.velocity.shape == (n, 3)
        self.bounds = compute_bounds(self.P, self.width, self.indices, self.velocity)
        c = d.curves[0]
        c.n_points, c.n_curves = n, len(self.indices)
        c.P, c.width, c.Cd, c.indices = self.P.ctypes.data, self.width.ctypes.data, self.Cd.ctypes.data, self.indices.ctypes.data
        c.uv = None
        c.velocity = None if self.velocity is None else self.velocity.ctypes.data
        for k in range(6):
            c.bounds[k] = float(self.bounds[k])
        self.curve_inst = [k for k in range(d.n[5]) if d.instances[k].primset_type == 1]
        assert len(self.curve_inst) == 1, "one curve instance"
        self.curve_inst = self.curve_inst[0]
        x = d.instances[self.curve_inst].xform
        assert list(x.n) == [1, 1, 1] and x.transform_order == 0 and x.rotate_order == 10
        rot, fac = XFORMS[xform]
        for k in range(3):
            x.translate[0][k], x.rotate[0][k], x.scale[0][k] = float(translate[k]), float(rot[k]), float(fac[k])
        self.M, self.Minv = instance_matrix(xform, translate)

    def groups(self):
        """group 0 and the all-objects group (and group 1 of the stock scene: the mesh and the curves)"""
        return sorted(set([0, 1, self.target_group]) & set(range(self.n_groups)))

    def to_world(self, rays):
        """object-space rays [n, 8] through the instance matrix (MatTransformPoint / MatTransformVector: t is preserved)"""
        m, out = self.M, np.array(rays, dtype=np.float64)
        o, d = rays[:, 0:3], rays[:, 3:6]
        for r in range(3):
            out[:, r] = m[r, 0] * o[:, 0] + m[r, 1] * o[:, 1] + m[r, 2] * o[:, 2] + m[r, 3]
            out[:, 3 + r] = m[r, 0] * d[:, 0] + m[r, 1] * d[:, 1] + m[r, 2] * d[:, 2]
        return out


# ------------------------------------------------------------------------------------------------------------------ families
def _pack(cps, w0, w1, rng, chained=None):
    """cps [m, 4, 3] control points, end widths w0 / w1 (scalars or [m]) -> the arrays of a set with four points of its own per curve;
    widths are linear along a curve (the two inner entries are not read by the ribbon test), colours random"""
    cps = np.asarray(cps, dtype=np.float64)
    m = cps.shape[0]
    w0, w1 = np.broadcast_to(np.asarray(w0, dtype=np.float64), (m,)), np.broadcast_to(np.asarray(w1, dtype=np.float64), (m,))
    width = np.stack([w0, w0 + (w1 - w0) / 3, w0 + 2 * (w1 - w0) / 3, w1], axis=1).reshape(-1)
    Cd = rng.uniform(.1, 1., size=(4 * m, 3)).astype(np.float32)
    return dict(P=cps.reshape(-1, 3), width=width, Cd=Cd, indices=np.arange(m, dtype=np.int32) * 4, velocity=None)


def _strands(rng, m, length=.12, bend=.25, centre=CENTRE, spread=SPREAD):
    """m gently bent strands like the generator's, larger: root, two inner points and tip along a random direction"""
    root = centre + rng.uniform(-spread, spread, size=(m, 3))
    e = rng.normal(size=(m, 3))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    cps = np.empty((m, 4, 3))
    for k in range(4):
        cps[:, k] = root + e * (length * k / 3.) + (rng.normal(size=(m, 3)) * bend * length * (k > 0) * k / 3.)
    return cps


def straight_even(rng):
    """collinear, evenly spaced control points: every second difference is EXACTLY zero (coordinates on a 2^-10 lattice), L0 == 0,
    log(0) = -inf"""
    m = 48
    root = np.round((CENTRE + rng.uniform(-SPREAD, SPREAD, size=(m, 3))) * 1024) / 1024
    step = np.round(rng.uniform(-.05, .05, size=(m, 3)) * 1024) / 1024
    step[np.abs(step).max(axis=1) < 8 / 1024.] = (24 / 1024., -16 / 1024., 8 / 1024.)
    cps = np.stack([root + k * step for k in range(4)], axis=1)
    assert np.all(cps[:, 0] - 2 * cps[:, 1] + cps[:, 2] == 0) and np.all(cps[:, 1] - 2 * cps[:, 2] + cps[:, 3] == 0)
    return _pack(cps, .006, .002, rng)


def zero_width(rng):
    return _pack(_strands(rng, 32), 0., 0., rng)


def needle(rng):
    m = 48
    tip_first = np.arange(m) % 2 == 0
    return _pack(_strands(rng, m), np.where(tip_first, 0., .008), np.where(tip_first, .008, 0.), rng)


def reverse_taper(rng):
    return _pack(_strands(rng, 48), 2e-5, 2e-2, rng)


def point(rng):
    p = CENTRE + rng.uniform(-SPREAD, SPREAD, size=(32, 1, 3))
    return _pack(np.repeat(p, 4, axis=1), .01, .004, rng)


def closed_loop(rng):
    cps = _strands(rng, 40, length=.2, bend=.6)
    cps[:, 3] = cps[:, 0]
    return _pack(cps, .008, .003, rng)


def cusp(rng):
    """control polygons that cross so that the curve has a cusp: p1 and p2 swapped across the chord"""
    m = 40
    cps = _strands(rng, m, length=.15, bend=.05)
    side = np.cross(cps[:, 3] - cps[:, 0], rng.normal(size=(m, 3)))
    side *= .1 / np.linalg.norm(side, axis=1, keepdims=True)
    p1, p2 = cps[:, 1].copy(), cps[:, 2].copy()
    cps[:, 1], cps[:, 2] = p2 + side, p1 + side
    return _pack(cps, .008, .002, rng)


def self_crossing(rng):
    """a loop: the inner control points far beyond the opposite ends"""
    m = 40
    cps = _strands(rng, m, length=.06, bend=.05)
    chord = cps[:, 3] - cps[:, 0]
    side = np.cross(chord, rng.normal(size=(m, 3)))
    side *= .2 / np.linalg.norm(side, axis=1, keepdims=True)
    cps[:, 1], cps[:, 2] = cps[:, 3] + 2 * chord + side, cps[:, 0] - 2 * chord + side
    return _pack(cps, .006, .003, rng)


def hairpin(rng):
    """thin and sharply folded: L0 / width is far beyond 4^5 / 21, the depth clamps at 5"""
    m = 32
    cps = _strands(rng, m, length=.3, bend=.02)
    cps[:, 3] = cps[:, 0] + .05 * (cps[:, 3] - cps[:, 0]) + rng.normal(size=(m, 3)) * .004
    return _pack(cps, .0012, .0004, rng)


def blob(rng):
    """width larger than the curve's length"""
    return _pack(_strands(rng, 24, length=.02, bend=.2), .09, .05, rng)


def duplicates(rng):
    """pairs of identical curves; the two of a pair have different colours at both ends"""
    cps = _strands(rng, 24)
    s = _pack(np.repeat(cps, 2, axis=0), .008, .003, rng)
    s["Cd"][0::8], s["Cd"][3::8] = (1., .05, .05), (.9, .6, .05)          # first of the pair: red to orange
    s["Cd"][4::8], s["Cd"][7::8] = (.05, .1, 1.), (.05, .9, .9)           # second: blue to cyan
    return s


def chained(rng):
    """strands of five cubics that share end control points; indices step by 3 (16 points per strand) as the hair generator lays
    them out"""
    n_strands, per = 12, 5
    P, width, idx = [], [], []
    for s in range(n_strands):
        p = CENTRE + rng.uniform(-SPREAD, SPREAD, size=3)
        e = rng.normal(size=3)
        e /= np.linalg.norm(e)
        base = len(P)
        for k in range(3 * per + 1):
            P.append(p.copy())
            width.append(.008 * (1 - k / (3. * per)) + .001 * k / (3. * per))
            e = e + rng.normal(size=3) * .25
            e /= np.linalg.norm(e)
            p = p + e * .03
        idx += [base + 3 * j for j in range(per)]
    P = np.array(P)
    return dict(P=P, width=np.array(width), Cd=rng.uniform(.1, 1., size=(len(P), 3)).astype(np.float32),
                indices=np.array(idx, dtype=np.int32), velocity=None)


def flat_set(rng):
    """all curves in the plane y = 0 (the floor is there too): the grid is one cell thick"""
    cps = _strands(rng, 48, centre=np.array([.0, .0, .35]), spread=.25)
    cps[:, :, 1] = 0.
    return _pack(cps, .01, .004, rng)


def on_cell_faces(rng):
    """straight axis-parallel curves exactly on the cell boundaries of the reference grid over the set: eight corner curves pin the
    bounds, the grid is computed as BuildCurveSet does, the others are placed on its planes (which leaves bounds and grid alone)"""
    m_in, w = 40, .004
    lo, hi = CENTRE - .2, CENTRE + .2
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    inward = np.sign(CENTRE - corners)
    cps = np.stack([corners + inward * np.array([.05 * k / 3., 0, 0]) for k in range(4)], axis=1)
    flat = cps.reshape(-1, 3)
    n, cell, b = grid_of(compute_bounds(flat, np.full(len(flat), w), np.arange(8) * 4), 8 + m_in)
    inner = np.empty((m_in, 4, 3))
    for i in range(m_in):
        axis = i % 3
        at = np.array([b[a] + rng.randint(2, n[a] - 4) * cell[a] for a in range(3)])        # a grid vertex: on planes of all three axes
        span = rng.randint(1, 4) * cell[axis]
        for k in range(4):
            inner[i, k] = at
            inner[i, k, axis] = at[axis] + span * k / 3.
    s = _pack(np.concatenate([cps, inner], axis=0), w, w, rng)
    n2, cell2, b2 = grid_of(compute_bounds(s["P"], s["width"], s["indices"]), 8 + m_in)
    assert np.array_equal(n, n2) and np.array_equal(cell, cell2) and np.array_equal(b, b2)
    return s


def single(rng):
    return _pack(_strands(rng, 1, length=.2, centre=CENTRE + np.array([.1, .15, .1]), spread=.02), .02, .006, rng)


def _fur(rng, m=48):
    return _strands(rng, m, length=.03, bend=.15, spread=.12)


def far_offset(rng):
    """fur-sized curves at |P| ~ 1e3 in object space (frames put the instance back with translate = -FAR)"""
    return _pack(_fur(rng) + FAR, FUR_W[0], FUR_W[1], rng)


def tiny_scale(rng):
    """the same curves scaled by 1e-4, widths included.  No ray can hit them: at depth 0 the reference refuses a piece whose chord
    is shorter than 1e-3 in ray space (|dir.xy|^2 < 1e-6, src/fj_curve.cc converge_bezier3), and these are 3e-6 long"""
    return _pack(_fur(rng) * 1e-4, FUR_W[0] * 1e-4, FUR_W[1] * 1e-4, rng)


def far_offset_x0(rng):
    """the same at (0, -780, 640): 1e3 away along y and z only, so that the box the reference gives a MIRRORED instance (absolute
    scale factors, src/fj_object_instance.cc:313-356: right only for a set that straddles the mirror plane) still holds the set"""
    return _pack(_fur(rng) + FAR_X0, FUR_W[0], FUR_W[1], rng)


def small_scale(rng):
    """fur at a third of its size, widths included: depth-0 pieces 2e-3 .. 1e-2 long, just above the 1e-3 below which the
    reference refuses a piece (tiny_scale), with radii down to 1.5e-5"""
    return _pack(_strands(rng, 48, length=.01, bend=.15, spread=.04), FUR_W[0] / 3, FUR_W[1] / 3, rng)


def velocity_zero(rng):
    """the `chained` set itself with a velocity array of zeros"""
    s = family("chained")
    s["velocity"] = np.zeros_like(s["P"])
    return s


def velocity_large(rng):
    """every strand moves by several curve lengths over the shutter (a curve is ~.09 long)"""
    s = family("chained")
    per = 16
    v = np.repeat(rng.normal(size=(len(s["P"]) // per, 3)) * .2, per, axis=0)
    s["velocity"] = v + rng.normal(size=s["P"].shape) * .02
    return s


FAMILIES = {"straight_even": straight_even, "zero_width": zero_width, "needle": needle, "reverse_taper": reverse_taper, "point": point,
            "closed_loop": closed_loop, "cusp": cusp, "self_crossing": self_crossing, "hairpin": hairpin, "blob": blob,
            "duplicates": duplicates, "chained": chained, "flat_set": flat_set, "on_cell_faces": on_cell_faces, "single": single,
            "far_offset": far_offset, "far_offset_x0": far_offset_x0, "tiny_scale": tiny_scale, "small_scale": small_scale}
MOVING = {"velocity_zero": velocity_zero, "velocity_large": velocity_large}      # frames only: fjgpu_trace has no time argument
NO_HITS = ("zero_width", "point", "tiny_scale")         # families no ray can hit (zero radius; chords below the reference's 1e-3)
HIT_FLOOR = 200                                          # oracle hits AND misses among the aimed rays of every other family
FRAME_TRANSLATE = {"far_offset": tuple(-FAR), "far_offset_x0": tuple(-FAR_X0)}            # instance translation that brings a family in front of the camera


def family(name):
    """the arrays of a family, seeded by its name (its crc32: adding or renaming a family leaves the others as they are)"""
    both = dict(FAMILIES, **MOVING)
    return both[name](np.random.RandomState((SEED + zlib.crc32(name.encode("ascii"))) % (1 << 32)))


# ---------------------------------------------------------------------------------------------------------------------- rays
def _bezier(cp, v):
    u = 1 - v
    return (u * u * u)[:, None] * cp[:, 0] + (3 * u * u * v)[:, None] * cp[:, 1] + (3 * u * v * v)[:, None] * cp[:, 2] + (v * v * v)[:, None] * cp[:, 3]


def _tangent(cp, v):
    u = 1 - v
    return (3 * u * u)[:, None] * (cp[:, 1] - cp[:, 0]) + (6 * u * v)[:, None] * (cp[:, 2] - cp[:, 1]) + (3 * v * v)[:, None] * (cp[:, 3] - cp[:, 2])


def _unit(a, rng):
    n = np.linalg.norm(a, axis=1, keepdims=True)
    fallback = rng.normal(size=a.shape)
    a = np.where(n > 1e-12, a / np.maximum(n, 1e-300), fallback / np.linalg.norm(fallback, axis=1, keepdims=True))
    return a


def _rays(o, d, tmin=1e-4, tmax=1000.):
    n = len(o)
    return np.concatenate([o, d, np.full((n, 1), tmin), np.full((n, 1), tmax)], axis=1)


def base_rays(curves, n_aimed=1500, seed=SEED):
    """object-space rays for a set, by kind -> (rays [n, 8], kind [n] of KINDS).  "aimed": towards a point of a ribbon at a random
    parameter, offset ACROSS the ribbon (perpendicular to ray and tangent) by -2 .. +2 local radii, so about half graze outside."""
    rng = np.random.RandomState(seed + 7)
    P, width, idx = curves["P"], curves["width"], curves["indices"]
    m = len(idx)
    cps = np.stack([P[idx + k] for k in range(4)], axis=1)
    w0, w1 = width[idx], width[idx + 3]
    size = max(float(np.linalg.norm(cps.max(axis=(0, 1)) - cps.min(axis=(0, 1)))), 1e-3 * float(np.abs(cps).max()), 1e-30)

    def targets(n, max_off):
        c = rng.randint(0, m, size=n)
        v = rng.uniform(0, 1, size=n)
        q, tan = _bezier(cps[c], v), _tangent(cps[c], v)
        r = .5 * ((1 - v) * w0[c] + v * w1[c])
        return c, q, tan, r, rng.uniform(-max_off, max_off, size=n)

    out = []
    # aimed
    c, q, tan, r, off = targets(n_aimed, 2.)
    d = _unit(rng.normal(size=(n_aimed, 3)), rng)
    e = _unit(np.cross(d, tan), rng)
    tgt = q + e * (off * r)[:, None]
    out.append(("aimed", _rays(tgt - d * (rng.uniform(.3, 1.5, size=(n_aimed, 1)) * size), d)))
    # along the chord and the end tangents, through the curve's own end points, both ways, inside the ribbon
    lines = []
    for a, b in ((0, 3), (0, 1), (2, 3)):
        d = _unit(cps[:, b] - cps[:, a], rng)
        for sgn in (1., -1.):
            lines.append(_rays(cps[:, a] - sgn * d * (.4 * size) + rng.normal(size=(m, 3)) * (.2 * np.minimum(w0, w1))[:, None], sgn * d))
    out.append(("along", np.concatenate(lines, axis=0)))
    # directions exactly +-x, +-y, +-z (the ray frame divides by sqrt(dx^2 + dz^2): +-y gives a NaN frame)
    n_ax = 600
    c, q, tan, r, off = targets(n_ax, 1.5)
    d = np.zeros((n_ax, 3))
    d[np.arange(n_ax), np.arange(n_ax) % 3] = np.where((np.arange(n_ax) // 3) % 2 == 0, 1., -1.)
    e = _unit(np.cross(d, tan), rng)
    tgt = q + e * (off * r)[:, None]
    out.append(("axis", _rays(tgt - d * (rng.uniform(.3, 1.5, size=(n_ax, 1)) * size), d)))
    # origins on the curve and inside the ribbon
    n_in = 300
    c, q, tan, r, off = targets(n_in, .9)
    d = _unit(rng.normal(size=(n_in, 3)), rng)
    o = q + _unit(rng.normal(size=(n_in, 3)), rng) * (np.abs(off) * r * (np.arange(n_in) % 2))[:, None]
    out.append(("inside", _rays(o, d)))
    # non-unit directions: aimed rays again with the direction scaled (t scales the other way)
    n_sc = 400
    c, q, tan, r, off = targets(n_sc, 2.)
    d = _unit(rng.normal(size=(n_sc, 3)), rng)
    e = _unit(np.cross(d, tan), rng)
    o = q + e * (off * r)[:, None] - d * (rng.uniform(.3, 1.5, size=(n_sc, 1)) * size)
    k = np.array([1e-3, .5, 7., 1e3])[np.arange(n_sc) % 4]
    out.append(("scaled", np.concatenate([o, d * k[:, None], (1e-4 / k)[:, None], (1000. / k)[:, None]], axis=1)))
    kinds = np.concatenate([np.full(len(r_), KINDS.index(name)) for name, r_ in out])
    return np.concatenate([r_ for _, r_ in out], axis=0), kinds


KINDS = ("aimed", "along", "axis", "inside", "scaled", "bracket")


def bracket_rays(rays, t, hit, n=300):
    """second pass: rays that hit, again with tmax one ulp below / above t and tmin one ulp below / above t (four copies)"""
    pick = np.flatnonzero(hit & np.isfinite(t))[:n]
    out = []
    for col, to in ((7, -np.inf), (7, np.inf), (6, -np.inf), (6, np.inf)):
        r = rays[pick].copy()
        r[:, col] = np.nextafter(t[pick], to)
        out.append(r)
    return np.concatenate(out, axis=0) if len(pick) else np.zeros((0, 8))


def nan_frame(rays_obj):
    """rays whose object-space direction has dx == dz == 0: make_ray_frame / compute_world_to_ray_matrix divide by zero"""
    return (rays_obj[:, 3] == 0) & (rays_obj[:, 5] == 0)


def same_t(a, b):
    """bit-equal where finite, NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)) | (a == b)))
