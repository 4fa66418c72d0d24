"""The per-light hull cones of the light loop (fujiyama-renderer_amd/csrc/device/fjgpu_light_hull.h) must never settle a (surface point,
light) pair whose shadow ray the reference finds occluded: "settled" only where the oracle's trace of the instance (fjo_scene_trace: instance
box, Minv, TriRayIntersect in object space) reports no hit for (Ps, normalize(Pl - Ps), 1e-4, |Pl - Ps|), the ray k_shadow_cull builds.

The records are the ones scene creation builds (fjgpu_host_light_hulls: the upload's own function with the upload's reaches, no device needed), the verdicts come from
the header compiled for the host (lib/libfj_light_hull_host.so, tools/light_hull_host.cc).  Scenes of ONE instance of a mesh -- the "tiny"
bumpy sphere, a cube, a thin plate -- rotated, scaled non-uniformly and mirrored, at scales 1e-2, 1 and 1e3; random segments, segments aimed
1e-14 .. 1e-1 of the scale past the silhouette, points between light and mesh, beyond the light and inside the hull.  The build rules are
checked on their own, and a floor on usefulness -- derived from the six-plane construction, not tuned -- keeps a never-deciding record from
passing.  (On the device a -DFJ_LIGHT_HULL_VALIDATE build walks every settled pair of whole frames: profiles/light_hulls.txt.)"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_ffi
from fujiyama_renderer_amd import gpu, host, synth, workloads
from fujiyama_renderer_amd.fujiyama import SceneInterface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HULL = gpu.LIGHT_HULL
SCALES = (1e-2, 1, 1e3)
# (rotate, scale factors): rotated, non-uniformly scaled, mirrored
XFORMS = {"rotated": ((20, -35, 10), (1, 1, 1)), "nonuniform": ((0, 25, -15), (1, .4, 2.5)), "mirrored": ((10, 40, 0), (-1, 1, .7))}


def _lib():
    path = os.path.join(ROOT, "fujiyama-renderer_amd", "lib", "libfj_light_hull_host.so")
    assert os.path.exists(path), "lib/libfj_light_hull_host.so is not built (csrc/Makefile builds it with the ROCm clang++)"
    assert os.path.exists(oracle_ffi.ORACLE_SO), "oracle/liboracle.so is not built"
    L = C.CDLL(path)
    assert L.fj_light_hull_record_bytes() == HULL.itemsize == 160
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def verdicts(recs, Pl, hull_of, Ps, normalise=1):
    Pl = np.ascontiguousarray(Pl, np.float64).reshape(-1, 3)
    Ps = np.ascontiguousarray(Ps, np.float64)
    hull_of = np.ascontiguousarray(hull_of, np.int32)
    out = np.empty(len(Ps), np.int8)
    _lib().fj_light_hull_test_batch(C.c_int64(len(Ps)), _p(recs), _p(Pl), _p(hull_of), _p(Ps), normalise, _p(out))
    return out != 0


def build_direct(Pl, verts, box=None):
    """records from bare vertex arrays (identity matrix): the build rules"""
    Pl = np.ascontiguousarray(Pl, np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(verts, np.float64)
    if box is None:
        box = np.concatenate([v.min(axis=0) - 1e-4, v.max(axis=0) + 1e-4])
    box = np.ascontiguousarray(box, np.float64)
    M = np.ascontiguousarray(np.eye(4)[:3], np.float64)
    out = np.zeros(len(Pl), HULL)
    fn = _lib().fj_light_hull_build_batch
    fn.restype = C.c_int
    built = fn(C.c_int64(len(Pl)), _p(Pl), C.c_int64(len(v)), _p(v), _p(M), _p(box), _p(out))
    assert built == int((out["count"] > 0).sum())
    return out


def read_ply_vertices(path):
    with open(path, "rb") as f:
        n, nprop, line = 0, 0, b""
        in_vertex = False
        while line.strip() != b"end_header":
            line = f.readline()
            w = line.split()
            if w[:2] == [b"element", b"vertex"]:
                n, in_vertex = int(w[2]), True
            elif w[:1] == [b"element"]:
                in_vertex = False
            elif w[:1] == [b"property"] and in_vertex:
                assert w[1] == b"float"
                nprop += 1
        v = np.fromfile(f, dtype="<f4", count=n * nprop).reshape(n, nprop)[:, :3]
    return v.astype(np.float64)


CUBE_V = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
CUBE_Q = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]], np.int32)


@pytest.fixture(scope="module")
def meshes(tmp_path_factory, asset_dir):
    d = tmp_path_factory.mktemp("light_hull_meshes")
    out = {"tiny": synth.ensure_assets(asset_dir, ("tiny",))["tiny"]}
    out["cube"] = str(d / "cube.ply")
    synth.write_ply(out["cube"], CUBE_V, faces_quads=CUBE_Q)
    out["plate"] = str(d / "plate.ply")
    synth.write_ply(out["plate"], CUBE_V * np.array([1, .002, .6], np.float32), faces_quads=CUBE_Q)
    return out


class Case(object):
    """one instance of a mesh in a group of its own under a few point lights: the upload's records, world vertices, the oracle"""

    def __init__(self, mesh_path, scale, xform, lights):
        rot, fac = XFORMS[xform]
        si = SceneInterface(parse_args=False)
        si.OpenPlugin("plastic_shader", "PlasticShader")
        si.OpenPlugin("stanfordply_procedure", "StanfordPlyProcedure")
        si.NewCamera("cam1", "PerspectiveCamera")
        si.SetProperty3("cam1", "translate", 0, 0, 10 * scale)
        for i, p in enumerate(lights):
            si.NewLight("light%d" % i, "PointLight")
            si.SetProperty3("light%d" % i, "translate", *[float(x) for x in p])
        si.NewShader("shader0", "plastic_shader")
        workloads._ply(si, "mesh0", mesh_path)
        si.NewObjectInstance("obj1", "mesh0")
        si.SetProperty3("obj1", "scale", *[float(scale * f) for f in fac])
        si.SetProperty3("obj1", "rotate", *rot)
        si.SetProperty3("obj1", "translate", .3 * scale, .2 * scale, -.1 * scale)
        si.AssignShader("obj1", "DEFAULT_SHADING_GROUP", "shader0")
        si.NewObjectGroup("group1")
        si.AddObjectToGroup("group1", "obj1")
        si.AssignObjectGroup("obj1", "shadow_target", "group1")
        workloads._renderer(si, (8, 8), (1, 1))
        host.run_scene_text(si.text(), deferred=True)
        self.sp, _ = host.get_desc()
        self.recs, self.Pl, self.M = gpu.host_light_hulls(self.sp, 0)
        assert np.allclose(self.Pl, np.asarray(lights, np.float64), rtol=1e-15, atol=0)
        v = read_ply_vertices(mesh_path)
        self.W = v @ self.M[:, :3].T + self.M[:, 3]            # world vertices
        self.scale = scale
        self.osc = oracle_ffi.OracleScene(self.sp)

    def close(self):
        self.osc.close()

    def hits(self, l, Ps):
        """the oracle on the light loop's ray: Ln = Pl - Ps, distance = sqrt(dot(Ln, Ln)), Ln *= 1 / distance"""
        Ln = self.Pl[l] - Ps
        dist = np.sqrt(Ln[:, 0] * Ln[:, 0] + Ln[:, 1] * Ln[:, 1] + Ln[:, 2] * Ln[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / dist
            d = np.where((dist > 0)[:, None], Ln * inv[:, None], Ln)
        rays = np.concatenate([Ps, d, np.full((len(Ps), 1), 1e-4), dist[:, None]], axis=1)
        t, ids, _ = self.osc.trace(0, rays)
        return ids[:, 0] >= 0

    def check(self, l, Ps, what):
        """-> (settled, hit).  The contract: no verdict where the oracle reports a hit, whichever form of Ln the test gets."""
        hit = self.hits(l, Ps)
        idx = np.full(len(Ps), l, np.int32)
        sure = verdicts(self.recs, self.Pl, idx, Ps, 1) | verdicts(self.recs, self.Pl, idx, Ps, 0)
        bad = sure & hit
        assert not bad.any(), "%s: %d contradictions, first: light %r point %r" % (what, int(bad.sum()), self.Pl[l], Ps[np.argmax(bad)])
        return sure, hit

    def frame(self, l):
        """(c, perpendicular offsets, axial distances) of the world vertices about the axis light -> vertex centroid"""
        c = self.W.mean(axis=0) - self.Pl[l]
        c /= np.linalg.norm(c)
        w = self.W - self.Pl[l]
        cw = w @ c
        return c, w - cw[:, None] * c, cw


def lights_around(scale, rng, n=3):
    """regular lights: a few object sizes away, all around"""
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d * scale * rng.uniform(5, 14, n)[:, None] + scale * np.array([.3, .2, -.1])


def silhouette_targets(case, l, n, rng):
    """points 1e-14 .. 1e-1 of the scale off the outline of the vertex set as the light sees it, either way: an extreme vertex in a random
    direction across the axis, pushed along that direction"""
    c, perp, cw = case.frame(l)
    a = np.cross(c, [1., 0, 0] if abs(c[0]) < .9 else [0, 1., 0])
    a /= np.linalg.norm(a)
    b = np.cross(c, a)
    phi = rng.uniform(0, 2 * np.pi, n)
    e = np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b
    k = np.argmax((e @ (case.W - case.Pl[l]).T) / cw[None, :], axis=1)
    eps = 10.0 ** rng.uniform(-14, -1, n) * case.scale * rng.choice([-1, 1], n)
    return case.W[k] + eps[:, None] * e


@pytest.mark.parametrize("xform", sorted(XFORMS))
@pytest.mark.parametrize("scale", SCALES)
def test_no_verdict_where_the_oracle_finds_a_hit(scale, xform, meshes):
    rng = np.random.default_rng(21)
    total_hit = total_sure = 0
    for name in ("tiny", "cube", "plate"):
        case = Case(meshes[name], scale, xform, lights_around(scale, rng))
        assert (case.recs["count"] == 6).all(), (name, case.recs["count"])
        for l in range(len(case.Pl)):
            n = 3000
            # random segments: points all around, from near the mesh to far away
            Ps = rng.uniform(-1, 1, (n, 3)) * scale * 10.0 ** rng.uniform(-.5, 1.5, n)[:, None]
            s1, h1 = case.check(l, Ps, "%s random" % name)
            # aimed past the silhouette: on the line from the light through the target, between light and mesh, just past the target, well
            # behind the mesh, and on the far side of the light
            T = silhouette_targets(case, l, n, rng)
            s = rng.choice([.3, .9, 1.0 + 1e-9, 1.5, 3., 30., -.5, -5.], n)
            s2, h2 = case.check(l, case.Pl[l] + s[:, None] * (T - case.Pl[l]), "%s aimed" % name)
            # inside the hull (convex combinations of vertices): inside every plane, never settled; and between the light and such a point
            wgt = rng.dirichlet(np.ones(4), n)
            inside = np.einsum("nk,nkj->nj", wgt, case.W[rng.integers(0, len(case.W), (n, 4))])
            s3, h3 = case.check(l, inside, "%s inside" % name)
            assert not s3.any()
            s4, h4 = case.check(l, case.Pl[l] + rng.uniform(.01, .99, n)[:, None] * (inside - case.Pl[l]), "%s between" % name)
            # beyond the light, seen from the mesh: unoccluded, and nearly all of them settled
            s5, h5 = case.check(l, case.Pl[l] + rng.uniform(-3, -.05, n)[:, None] * (inside - case.Pl[l]), "%s beyond" % name)
            assert not h5.any() and s5.mean() > .9
            total_hit += int(h1.sum() + h2.sum() + h3.sum() + h4.sum())
            total_sure += int(s1.sum() + s2.sum() + s4.sum() + s5.sum())
        case.close()
    print("scale %g %s: %d hits of the oracle, %d pairs settled, 0 contradictions" % (scale, xform, total_hit, total_sure))
    assert total_hit > 5000 and total_sure > 5000              # (neither set is vacuous)


def test_build_rules():
    cube = CUBE_V.astype(np.float64)
    # inside the hull, too near (gap below 1e-3 of the scale), too far (beyond 1e5 diagonals), vertices behind the plane through the light
    # across the axis: no record
    for Pl in ([0, 0, 0], [.5, -.2, .9], [0, 1.0005, 0], [0, 3e38, 0], [0, 1e7, 0], [1.2, .5, 0]):
        assert build_direct(np.array(Pl, np.float64), cube)[0]["count"] == 0, Pl
    # a regular light: six planes
    rng = np.random.default_rng(22)
    for scale in SCALES:
        pts = rng.normal(0, 1, (500, 3)) * scale * np.array([1, .3, 2])
        d = rng.normal(0, 1, (2000, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        Pl = d * scale * rng.uniform(12, 300, 2000)[:, None]
        recs = build_direct(Pl, pts)
        assert (recs["count"] == 6).all()
        # unit normals; every vertex inside every plane by the verify pass's slack; every plane within 1e-6 (relative) of touching a vertex
        assert np.allclose(np.linalg.norm(recs["n"], axis=2), 1.0, rtol=0, atol=1e-14)
        w = pts[None, :, :] - Pl[:, None, :]                                        # [lights, verts, 3]
        side = np.einsum("ljk,lvk->ljv", recs["n"], w)
        l1 = np.abs(w).sum(axis=2)
        assert (side <= -1e-12 * l1[:, None, :] * (1 - 1e-3)).all()
        assert ((side / l1[:, None, :]).max(axis=2) >= -1e-6).all()
        # the stored order 0, 2, 4, 1, 3, 5: the first three normals are 120 degrees apart about the axis, the fourth between the first two
        c = pts.mean(axis=0) - Pl
        c /= np.linalg.norm(c, axis=1)[:, None]
        flat = recs["n"] - np.einsum("ljk,lk->lj", recs["n"], c)[:, :, None] * c[:, None, :]
        flat /= np.linalg.norm(flat, axis=2)[:, :, None]
        cos = np.einsum("ljk,lmk->ljm", flat, flat)
        assert np.allclose(cos[:, 0, 1], -.5, atol=1e-6) and np.allclose(cos[:, 1, 2], -.5, atol=1e-6) and np.allclose(cos[:, 0, 2], -.5, atol=1e-6)
        assert np.allclose(cos[:, 0, 3], .5, atol=1e-6) and np.allclose(cos[:, 1, 3], .5, atol=1e-6)


@pytest.mark.parametrize("scale", SCALES)
def test_usefulness_floor(scale, meshes):
    """The six planes bound a hexagon around the projected vertices (projection about the axis onto the plane at distance one): with R the
    largest projected vertex radius every plane lies within R of the axis, so the hexagon lies inside the circle of radius R / cos(30 deg) =
    1.1547 R.  Every usable point (within reach, direction without a zero component) in front of the light whose projected radius exceeds
    1.16 R must be settled -- all of them.  Outside the circle of radius R no segment to the light can meet the mesh: the oracle alone
    reports misses there."""
    rng = np.random.default_rng(23)
    case = Case(meshes["tiny"], scale, "rotated", lights_around(scale, rng, n=4))
    assert (case.recs["count"] == 6).all()
    checked = 0
    for l in range(len(case.Pl)):
        c, perp, cw = case.frame(l)
        R = float((np.linalg.norm(perp, axis=1) / cw).max())
        n = 20000
        Ps = rng.uniform(-1, 1, (n, 3)) * scale * 10.0 ** rng.uniform(-.5, 1.5, n)[:, None]
        x = Ps - case.Pl[l]
        cx = x @ c
        rho = np.linalg.norm(x - cx[:, None] * c, axis=1) / np.where(cx > 0, cx, 1)
        Ln = case.Pl[l] - Ps
        usable = (cx > 0) & (rho > 1.16 * R) & (Ln != 0).all(axis=1) & (np.abs(Ps).max(axis=1) <= case.recs["reach"][l])
        assert usable.sum() > n // 4
        sure, hit = case.check(l, Ps[usable], "floor")
        assert not hit.any()
        assert sure.all(), "%d of %d usable points beyond 1.16 R are not settled" % (int((~sure).sum()), len(sure))
        checked += int(usable.sum())
    case.close()
    print("scale %g: %d points beyond 1.16 R, all settled" % (scale, checked))
