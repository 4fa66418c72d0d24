"""The adversarial meshes of pathological_meshes.py do what they claim -- checked with the CPU oracle alone, so that the GPU suite's
comparisons cannot pass on a set of misses."""
import numpy as np
import pytest

import pathological_meshes as pm


@pytest.mark.parametrize("name", sorted(pm.FAMILIES))
def test_generators_are_deterministic_and_exact_in_f32(name):
    v, t = pm.FAMILIES[name]()
    v2, t2 = pm.FAMILIES[name]()
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert np.array_equal(v, v2) and np.array_equal(t, t2)
    assert np.array_equal(v.astype(np.float64).astype(np.float32), v) and np.isfinite(v).all()
    assert t.min() >= 0 and t.max() < len(v)
    p = v[t].astype(np.float64)
    assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) > 0).all()      # no zero-area triangle


def test_families_have_the_shapes_they_are_named_for():
    v, t = pm.flat_sheet(1)
    assert len(t) == 2 * 33 * 33 and not v[:, 1].any() and v[:, 0].any() and v[:, 2].any()
    v, t = pm.flat_sheet(0)
    assert not v[:, 0].any() and v[:, 1].any()
    v, t = pm.same_centroid()
    p = v[t].astype(np.float64)
    assert len(t) == 64 and np.array_equal(.5 * (p.min(axis=1) + p.max(axis=1)), np.tile([1., 2., 3.], (64, 1)))
    v, t = pm.slivers()
    p = v[t].astype(np.float64)
    e = np.sort(np.stack([np.linalg.norm(p[:, a] - p[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))]), axis=0)
    height = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) / e[2]
    assert len(t) == 300 and (e[2] / height > 5e3).all()
    v, t = pm.duplicates()
    p = v[t]
    for grp in pm.DUP_GROUPS:
        for k in grp[1:]:
            assert np.array_equal(np.sort(p[k].view("f4,f4,f4"), axis=0), np.sort(p[grp[0]].view("f4,f4,f4"), axis=0))
    assert len(np.unique(t)) == 3 * len(t)                       # vertices of their own
    for k in (1, 2, 4, 5, 8):
        assert len(pm.tiny(k)[1]) == k
    for n in (257, 1000, 4099):
        assert len(pm.blocks(n)[1]) == n
    # the telescope: Morton codes of the box centres (21 bits per axis over the mesh's box) differ pairwise in a HIGHER bit the larger
    # the triangle: the radix tree peels one triangle per level
    v, t = pm.telescope()
    p = v[t].astype(np.float64)
    c = .5 * (p.min(axis=1) + p.max(axis=1))
    lo, hi = v.min(axis=0).astype(np.float64) - 1e-4, v.max(axis=0).astype(np.float64) + 1e-4
    q = np.minimum(np.floor((c - lo) / (hi - lo) * 2097151.), 2097151).astype(np.int64)
    keys = [sum(((int(q[j, a]) >> b) & 1) << (3 * b + 2 - a) for b in range(21) for a in range(3)) for j in range(len(t))]
    assert len(t) == 3 * pm.TELESCOPE_OCTAVES
    keys = keys[:60]                                     # (the 20 largest octaves: what the 21 bits resolve with a margin)
    assert all(keys[j] > keys[j + 1] for j in range(len(keys) - 1))
    first_diff = [(keys[j] ^ keys[j + 1]).bit_length() for j in range(len(keys) - 1)]
    assert all(first_diff[j] > first_diff[j + 1] for j in range(len(first_diff) - 1))


@pytest.mark.parametrize("name", sorted(n for n in pm.FAMILIES if n != "duplicates"))
def test_per_triangle_rays_hit_their_own_triangle(name, tmp_path):
    """COVERAGE: the oracle hits the ray's own triangle for at least 95 % of the triangles (the telescope: of those above the
    reference's epsilons), and where it does not it hits another triangle, never nothing"""
    v, t = pm.FAMILIES[name]()
    rays = pm.per_triangle_rays(v, t)
    tt, ids = pm.oracle_trace(pm.trace_scene(pm.write_mesh(tmp_path, name, v, t)), rays)
    pick = pm.telescope_head(v, t) if name == "telescope" else np.ones(len(t), dtype=bool)
    assert pick.sum() >= (45 if name == "telescope" else len(t))
    own = ids[:, 1] == np.arange(len(t))
    print(name, "own", own[pick].mean(), "hit", (ids[pick, 0] >= 0).mean())
    assert own[pick].mean() >= 0.95
    assert (ids[pick, 0] >= 0).all()


def test_duplicates_tie_and_the_largest_id_wins(tmp_path):
    """TIES: at least 200 rays get a t that is bit-equal for two or more primitives (each traced alone), and the oracle reports the
    largest of the tied ids -- the rule fjgpu_dev_traverse.h states for equal t inside one mesh"""
    path, rays, tied, winner = pm.duplicate_ties(tmp_path)
    tt, ids = pm.oracle_trace(pm.trace_scene(path), rays)
    print("tied rays", int(tied.sum()), "of", len(rays))
    assert tied.sum() >= 200
    assert (ids[tied, 0] == 0).all()
    assert np.array_equal(ids[tied, 1], winner[tied])
    assert len(np.unique(winner[tied])) >= 3                      # the nine-fold triangle, the quad and the far pair all tie


def test_axis_rays_run_down_the_telescope():
    """the rays for the stack tests: most of them pass (nearly) every nested box, and among those are rays that hit and rays that miss
    everything -- the latter walk the whole depth without a hit to cut it short"""
    v, t = pm.telescope()
    rays = pm.axis_rays()
    n = len(rays) // 2
    passed = pm.boxes_passed(rays, *pm.telescope_boxes(v, t))
    assert np.median(passed) >= 0.95 * len(t)
    assert (passed[:n] >= 0.9 * len(t)).sum() >= 500 and (passed[n:] >= 0.9 * len(t)).sum() >= 500
