"""Adversarial meshes for the BLAS builders and the traversal stacks, shared by the CPU suite (the oracle alone: the
inputs do what they claim) and the GPU suite (every builder and walk against the oracle).

Plain numpy with fixed seeds.  Every coordinate is an f32 value (the arrays ARE float32), so the device keeps the
36-byte triangle records and a PLY round trip changes nothing.  Meshes go through synth.write_ply into a directory of
the caller's (pytest's tmp_path): no binary asset is committed.
"""
import os

import numpy as np

from fujiyama_renderer_amd import synth, workloads
from fujiyama_renderer_amd.fujiyama import SceneInterface

SEED = 20261017


def _soup(tri_verts):
    """[n, 3, 3] corner coordinates -> (verts [3n, 3] f32, tris [n, 3] i32): every triangle has vertices of its own"""
    v = np.asarray(tri_verts, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------------------ telescope
TELESCOPE_SCALE = 1024.0          # the 1e-4 padding of the builder's bounds stays below the Morton grid's resolution
TELESCOPE_OCTAVES = 48            # 21 of them resolve in the 21-bit Morton axis; the host's SAH build needs the rest to come out deep


def telescope(n=3 * TELESCOPE_OCTAVES, ratio=0.5):
    """n triangles, three per octave, that shrink geometrically towards the apex (the origin) by `ratio` per octave.

    Octave k has size s = SCALE * ratio^k and holds three triangles whose boxes (in units of s) are
        a = 0: [.5, 1] x [.5, 1] x [.5, 1]      centre (.75, .75, .75)   -> Morton bits of octave k: 1 . .
        a = 1: [.125, .625] x [.5, 1] x [.5, 1]  centre (.375, .75, .75)  ->                          0 1 .
        a = 2: [.125, .625]^2 x [.5, 1]          centre (.375, .375, .75) ->                          0 0 1
    and everything of the later octaves lies below .5 s in every axis (bits 0 0 0).  With ratio 1/2 the radix tree of
    the Morton codes therefore peels ONE triangle per level, three levels per octave, 63 levels for the 21 octaves its
    21 bits per axis resolve (the smaller octaves share the last cells).  The binned-SAH build peels about an octave per
    split and the clustering merges from the apex outwards, one pair per round: both come out as deep as the octaves go.  All
    three boxes of an octave contain the piece [.5, .625] s of the diagonal: a ray from the apex along (1, 1, 1) enters
    the boxes of the small octaves first and passes every one of them.  Each triangle spans its box from the corner
    nearest the apex: A = (x0, y0, z0), B = (x1, y1, z0), C = (x0, y1, z1); rays beside the diagonal miss most of them.
    """
    boxes = (((.5, 1.), (.5, 1.), (.5, 1.)), ((.125, .625), (.5, 1.), (.5, 1.)), ((.125, .625), (.125, .625), (.5, 1.)))
    tv = np.empty((n, 3, 3))
    for j in range(n):
        s = TELESCOPE_SCALE * ratio ** (j // 3)
        (x0, x1), (y0, y1), (z0, z1) = boxes[j % 3]
        tv[j] = np.array([(x0, y0, z0), (x1, y1, z0), (x0, y1, z1)]) * s
    return _soup(tv)


def telescope_boxes(verts, tris):
    p = verts[tris].astype(np.float64)
    return p.min(axis=1), p.max(axis=1)


def boxes_passed(rays, bmin, bmax):
    """per ray: how many of the boxes its segment [tmin, tmax] passes (slab test in f64)"""
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0, t1 = (bmin[None] - o) * inv, (bmax[None] - o) * inv
    lo = np.nanmax(np.minimum(t0, t1), axis=2)
    hi = np.nanmin(np.maximum(t0, t1), axis=2)
    return (np.maximum(lo, rays[:, None, 6]) <= np.minimum(hi, rays[:, None, 7])).sum(axis=1)


def axis_rays(n_each=1500, seed=SEED):
    """rays for the telescope: from the apex itself (tmin 0) looking out along the diagonal, and from beyond the largest octave looking
    in, both with lateral offsets of up to a quarter of the local size (a cone around the diagonal: the rays stay inside the nested
    boxes, most of them miss most triangles), plus the exact diagonal both ways"""
    rng = np.random.RandomState(seed)
    diag = np.ones(3) / np.sqrt(3.0)
    lat = rng.normal(size=(n_each, 3))
    lat -= (lat @ diag)[:, None] * diag
    lat /= np.linalg.norm(lat, axis=1, keepdims=True)
    d = diag + lat * rng.uniform(0, .11, size=(n_each, 1))
    d[0] = diag
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = 2.0 * TELESCOPE_SCALE
    out = np.concatenate([np.zeros((n_each, 3)), d, np.zeros((n_each, 1)), np.full((n_each, 1), 1e30)], axis=1)
    into = np.concatenate([d * far, -d, np.full((n_each, 1), 1e-4), np.full((n_each, 1), 1e30)], axis=1)
    return np.concatenate([out, into], axis=0)


# ------------------------------------------------------------------------------------------------------- the other families
def duplicates():
    """one triangle nine times (vertices of their own, the same coordinates), a two-sided quad (two triangles, and the same two again
    with the opposite winding), and a second duplicated pair far enough away to land in another leaf"""
    t0 = np.array([(0., 0., 0.), (1., 0., .25), (.25, 1., .5)])
    q = np.array([(2., 0., 0.), (3., 0., 0.), (3., 1., .5), (2., 1., .5)])
    qa, qb = q[[0, 1, 2]], q[[0, 2, 3]]
    far = np.array([(40., 30., 20.), (41.5, 30., 20.5), (40., 31., 21.)])
    tv = [t0] * 9 + [qa, qb, qa[::-1], qb[::-1]] + [far, far]
    return _soup(np.array(tv))


DUP_GROUPS = (tuple(range(0, 9)), (9, 11), (10, 12), (13, 14))     # primitives that coincide


def tiny(k):
    """k triangles (1, 2, 4, 5, 8: around FJ_TINY_PRIMS = FJ_MAX_LEAF_PRIMS = 4), well apart along a gentle arc"""
    rng = np.random.RandomState(SEED + k)
    tv = np.empty((k, 3, 3))
    for i in range(k):
        c = np.array([.7 * i - .35 * (k - 1), .3 + .12 * (i % 3), .1 * i])
        tv[i] = c + rng.uniform(-.3, .3, size=(3, 3))
    return _soup(tv)


def flat_sheet(axis=1, n=33):
    """n x n quads (two triangles each) in the plane y = 0 -- or, axis = 0, the same sheet turned so that x is the flat axis:
    zero extent in one axis (Morton scale 0) and the same merge distance between all neighbours"""
    g = np.arange(n + 1, dtype=np.float64) / 8.0 - n / 16.0
    u, w = np.meshgrid(g, g, indexing="ij")
    p = np.zeros(((n + 1) * (n + 1), 3))
    a, b = [k for k in range(3) if k != axis]
    p[:, a], p[:, b] = u.ravel(), w.ravel()
    idx = lambda i, j: i * (n + 1) + j
    tris = []
    for i in range(n):
        for j in range(n):
            tris.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            tris.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return p.astype(np.float32), np.array(tris, dtype=np.int32)


def same_centroid(n=64):
    """n triangles of different sizes and orientations whose boxes all have the centre (1, 2, 3): all Morton keys equal.
    Triangle = centre + sg * (a, -b, -c), sg * (-a, b, -c), sg * (-a, -b, c): its box is centre +- (a, b, c) exactly (centre and
    half-sizes are multiples of 1/256 below 1: every sum is an f32 value).  Four orientations (sign patterns sg, two aspects) in sixteen
    sizes each: triangles of one orientation are parallel shells, and sg / -sg lie on opposite sides of the centre, so that few
    triangles cut each other near a centroid (64 random ones through one point hide a third of each other's centroids)."""
    c = np.array([1., 2., 3.])
    sgs = ((1, 1, 1), (-1, -1, -1), (1, 1, -1), (-1, -1, 1))
    tv = np.empty((n, 3, 3))
    for i in range(n):
        p, m = i % 4, 1 + i // 4
        h = np.array(((3, 4, 5), (5, 3, 4))[p // 2]) * (3 * m + p % 2) / 256.0
        tv[i] = c + np.array([(1, -1, -1), (-1, 1, -1), (-1, -1, 1)]) * h * np.array(sgs[p], dtype=np.float64)
    return _soup(tv)


def slivers(n=300):
    """n needle triangles, 1 : 1e4 aspect, random orientation, lengths .5 .. 2 in a cube of side 8"""
    rng = np.random.RandomState(SEED + 2)
    tv = np.empty((n, 3, 3))
    for i in range(n):
        c = rng.uniform(-4, 4, size=3)
        e = rng.normal(size=3)
        e /= np.linalg.norm(e)
        f = np.cross(e, rng.normal(size=3))
        f /= np.linalg.norm(f)
        L = rng.uniform(.5, 2.)
        tv[i] = [c - .5 * L * e, c + .5 * L * e, c + 1e-4 * L * f]
    return _soup(tv)


def blocks(n):
    """n random small triangles in the unit cube (257, 1000, 4099: around the builder's 256-thread blocks)"""
    rng = np.random.RandomState(SEED + n)
    c = rng.uniform(0, 1, size=(n, 1, 3))
    return _soup(c + rng.uniform(-.03, .03, size=(n, 3, 3)))


FAMILIES = {
    "telescope": telescope,
    "duplicates": duplicates,
    "tiny1": lambda: tiny(1), "tiny2": lambda: tiny(2), "tiny4": lambda: tiny(4), "tiny5": lambda: tiny(5), "tiny8": lambda: tiny(8),
    "flat_sheet_y": lambda: flat_sheet(1), "flat_sheet_x": lambda: flat_sheet(0),
    "same_centroid": same_centroid,
    "slivers": slivers,
    "blocks257": lambda: blocks(257), "blocks1000": lambda: blocks(1000), "blocks4099": lambda: blocks(4099),
}


def write_mesh(directory, name, verts, tris):
    path = os.path.join(str(directory), name + ".ply")
    synth.write_ply(path, verts, faces_tris=tris)
    return path


# ------------------------------------------------------------------------------------------------------------------ rays
def _normals_extents(verts, tris):
    p = verts[tris].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm + 0.0                  # (no negative zeros: -0.0 + 0.0 = +0.0; the rays' directions are -n, see below)
    ext = np.linalg.norm(p.max(axis=1) - p.min(axis=1), axis=1)        # the triangle's box diagonal
    return p, nrm, ext


def per_triangle_rays(verts, tris):
    """one ray per triangle: from centroid + 1e-2 extent n towards -n, tmin 1e-4, tmax twice that offset (extent: the diagonal of the
    triangle's box) -- its own triangle is the nearest thing such a ray can hit unless another one really lies in front"""
    p, nrm, ext = _normals_extents(verts, tris)
    off = 1e-2 * ext
    o = p.mean(axis=1) + off[:, None] * nrm
    return np.concatenate([o, 0.0 - nrm, np.full((len(tris), 1), 1e-4), 2 * off[:, None]], axis=1)


def surface_rays(verts, tris, per_tri, seed=SEED):
    """per_tri rays per triangle like per_triangle_rays, through random interior points instead of the centroid"""
    rng = np.random.RandomState(seed)
    p, nrm, ext = _normals_extents(verts, tris)
    rays = []
    for _ in range(per_tri):
        w = rng.dirichlet((2., 2., 2.), size=len(tris))
        at = (p * w[:, :, None]).sum(axis=1)
        off = 1e-2 * ext
        rays.append(np.concatenate([at + off[:, None] * nrm, 0.0 - nrm, np.full((len(tris), 1), 1e-4), 2 * off[:, None]], axis=1))
    return np.concatenate(rays, axis=0)


def soup_rays(verts, n=6000, seed=SEED):
    """random rays around the mesh as in test_trace_groups_bit_exact_against_oracle: 30 % short tmax, axis-aligned directions,
    origins inside the mesh's box"""
    rng = np.random.RandomState(seed + 3)
    lo, hi = verts.min(axis=0).astype(np.float64), verts.max(axis=0).astype(np.float64)
    mid, half = .5 * (lo + hi), .5 * np.maximum(hi - lo, 1e-3 * max(1e-3, float((hi - lo).max())))
    size = float(np.linalg.norm(2 * half))
    o = mid + rng.normal(size=(n, 3)) * half * 1.2
    o[::3] = mid + rng.uniform(-1, 1, size=(len(o[::3]), 3)) * half
    tgt = mid + rng.uniform(-1, 1, size=(n, 3)) * half
    d = tgt - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    d[::97] = [0, -1, 0]
    d[1::97] = [1, 0, 0]
    d[2::97] = [0, 0, -1]
    tmax = np.where(rng.uniform(size=n) < .3, rng.uniform(.02, 1.0, size=n) * size, 1e6 * size)
    return np.concatenate([o, d, np.full((n, 1), 1e-4), tmax[:, None]], axis=1)


# ---------------------------------------------------------------------------------------------------------------- scenes
def trace_scene(mesh_path, instances=((0, 0, 0),), normal_mesh=None):
    """the mesh as the only object (instances: translations) -- group 0 is the all-objects group -- optionally beside one
    instance of a normal mesh; in the style of test_oracle_golden._mesh_scene"""
    si = SceneInterface(parse_args=False)
    si.OpenPlugin("ply", "StanfordPlyProcedure")
    si.OpenPlugin("constant_shader", "ConstantShader")
    si.NewCamera("cam1", "PerspectiveCamera")
    si.NewShader("s", "constant_shader")
    for name, path in (("m", mesh_path),) + ((("nm", normal_mesh),) if normal_mesh else ()):
        si.NewMesh(name)
        si.NewProcedure(name + "_p", "ply")
        si.AssignMesh(name + "_p", "mesh", name)
        si.SetStringProperty(name + "_p", "filepath", path)
        si.RunProcedure(name + "_p")
    if normal_mesh:
        si.NewObjectInstance("normal1", "nm")
        si.SetProperty3("normal1", "translate", 0, -2.5, 0)
        si.AssignShader("normal1", "DEFAULT_SHADING_GROUP", "s")
    for k, t in enumerate(instances):
        si.NewObjectInstance("o%d" % k, "m")
        si.SetProperty3("o%d" % k, "translate", *t)
        si.AssignShader("o%d" % k, "DEFAULT_SHADING_GROUP", "s")
    si.NewFrameBuffer("fb1", "rgba")
    si.NewRenderer("ren1")
    si.AssignCamera("ren1", "cam1")
    si.AssignFrameBuffer("ren1", "fb1")
    si.SetProperty2("ren1", "resolution", 32, 32)
    si.RenderScene("ren1")
    return si.text()


def frame_scene(asset_dir, mesh_path, lights, res=(48, 32), spp=(2, 2), shader="plastic", instances=None, scale=1.0, normal_mesh=None,
                ren_props=()):
    """the mesh over the existing floor (edge_scenes.custom_scene's camera), point lights at the caller's positions (intensity 1 / count).
    shader: "plastic", "glass", or "translucent" (plastic, opacity .35, no reflection: the translucent_occluder edge case).
    instances: (translate, rotate) per instance of the mesh, each scaled by `scale`; default one above the floor."""
    a = synth.ensure_assets(asset_dir, ("tiny",))
    si = SceneInterface(parse_args=False)
    si.OpenPlugin("plastic_shader", "PlasticShader")
    si.OpenPlugin("glass_shader", "GlassShader")
    si.OpenPlugin("stanfordply_procedure", "StanfordPlyProcedure")
    si.NewCamera("cam1", "PerspectiveCamera")
    si.SetProperty3("cam1", "translate", 0.5, 2.0, 6)
    si.SetProperty3("cam1", "rotate", -12, 4, 0)
    si.SetProperty1("cam1", "fov", 40)
    for i, p in enumerate(lights):
        si.NewLight("light%d" % i, "PointLight")
        si.SetProperty3("light%d" % i, "translate", *p)
        si.SetProperty1("light%d" % i, "intensity", 1.0 / len(lights))
    si.NewShader("floor_shader", "plastic_shader")
    si.NewShader("obj_shader", "glass_shader" if shader == "glass" else "plastic_shader")
    if shader == "translucent":
        si.SetProperty1("obj_shader", "opacity", .35)
        si.SetProperty3("obj_shader", "reflect", 0, 0, 0)
    workloads._ply(si, "floor_mesh", a["floor"])
    workloads._ply(si, "obj_mesh", mesh_path)
    si.NewObjectInstance("floor1", "floor_mesh")
    si.AssignShader("floor1", "DEFAULT_SHADING_GROUP", "floor_shader")
    if normal_mesh:
        workloads._ply(si, "normal_mesh", normal_mesh)
        si.NewShader("normal_shader", "plastic_shader")
        si.NewObjectInstance("normal1", "normal_mesh")
        si.SetProperty3("normal1", "translate", -1.6, 1.0, -1.0)
        si.AssignShader("normal1", "DEFAULT_SHADING_GROUP", "normal_shader")
    for k, (t, r) in enumerate(instances or (((0, .4, 0), (0, 0, 0)),)):
        name = "obj%d" % k
        si.NewObjectInstance(name, "obj_mesh")
        si.SetProperty3(name, "rotate", *r)
        si.SetProperty3(name, "scale", scale, scale, scale)
        si.SetProperty3(name, "translate", *t)
        si.AssignShader(name, "DEFAULT_SHADING_GROUP", "obj_shader")
    workloads._renderer(si, res, spp, ren_props)
    return si.text()


# ------------------------------------------------------------------------------------------------- oracle-side helpers
def oracle_trace(text, rays, group=0):
    """(t, ids) of the CPU oracle for the scene text"""
    import oracle_ffi
    from fujiyama_renderer_amd import host
    host.run_scene_text(text, deferred=True)
    sp, _ = host.get_desc()
    osc = oracle_ffi.OracleScene(sp)
    t, ids, _ = osc.trace(group, rays)
    osc.close()
    return t, ids


def duplicate_ties(directory):
    """the `duplicates` mesh, 30 rays per triangle, and which of them tie: traces every triangle ALONE (a mesh of one) and
    returns (mesh path, rays, tied [n] bool, winner [n]): tied where two or more triangles give the bit-equal smallest t, winner the
    LARGEST primitive id among those (the rule stated in fjgpu_dev_traverse.h)"""
    v, t = duplicates()
    path = write_mesh(directory, "duplicates", v, t)
    rays = surface_rays(v, t, 30)
    alone = np.full((len(t), len(rays)), np.inf)
    for k in range(len(t)):
        p = write_mesh(directory, "dup_alone_%d" % k, v[t[k]], np.array([[0, 1, 2]], dtype=np.int32))
        tk, ik = oracle_trace(trace_scene(p), rays)
        alone[k] = np.where(ik[:, 0] >= 0, tk, np.inf)
    tmin = alone.min(axis=0)
    at_min = (alone == tmin[None]) & np.isfinite(tmin)[None]
    tied = at_min.sum(axis=0) >= 2
    winner = np.where(at_min, np.arange(len(t))[:, None], -1).max(axis=0)
    return path, rays, tied, winner


def telescope_head(verts, tris):
    """triangles of the telescope that a per-triangle ray CAN hit: its offset reaches tmin = 1e-4 and the determinant of the
    reference's triangle test (2 x area for a unit direction along the normal) its EPSILON = 1e-6; the rest is the sub-epsilon tail"""
    p = verts[tris].astype(np.float64)
    area2 = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    ext = np.linalg.norm(p.max(axis=1) - p.min(axis=1), axis=1)
    return (area2 >= 2e-6) & (1e-2 * ext >= 2e-4)
