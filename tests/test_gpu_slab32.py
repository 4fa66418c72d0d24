"""GPU suite (-m gpu): the slab tests of the BLAS walks and the node quantiser as the DEVICE computes them (fjgpu_dev_slab32_batch,
fjgpu_dev_quantize_nodes: the walks' own statements, csrc/device/fjgpu_slab32.h) against the host build of the same header
(lib/libfj_slab32_host.so), bit for bit, on 2^18 (ray, box) pairs and 2^14 nodes drawn from the strata of tests/test_slab32_cpu.py.  The host
tool is fed the device's reciprocals, so v_perm_b32, v_pk_fma_f32 and the conversions do what the host twin says, and the contract the CPU
tests hold against exact arithmetic transfers to the device.  Beside it: filter_rcp keeps the 2^-49 the setup relies on, the constructed rays
are accepted on the device, and fjgpu_trace reproduces the oracle's hits for rays aimed at mesh vertices from 1 .. 64 mesh extents away."""
import os

import numpy as np
import pytest

import slab32_cases as sc
import pathological_meshes as pm
import test_gpu_parity as tg
from fujiyama_renderer_amd import gpu, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    rays, grid, ql, qh, sets, t = sc.device_pairs()
    assert len(rays) == 1 << 18
    words = sc.pack_words(ql, qh)
    dev = gpu.slab32_batch(rays, grid, words).view(sc.PROBE).reshape(-1)
    for a in (rays, grid, ql, qh, sets, t, dev):
        a.setflags(write=False)
    return rays, grid, ql, qh, words, sets, t, dev


def test_device_constants_verdicts_and_tnear_equal_the_host_twins(pairs):
    rays, grid, ql, qh, words, sets, t, dev = pairs
    hrays = rays.copy()
    hrays[:, 3:6] = dev["inv"]
    host = sc.probe(sc.host_lib(int(gpu.build_config("slab_perm"))), hrays, grid, words)
    for name in ("q", "f", "tnear_q", "tnear_f", "verdict", "sh"):
        same = dev[name].view(np.uint32) == host[name].view(np.uint32)
        assert same.all(), "%s differs in %d of %d records (first %d: device %r, host %r)" % (
            name, (~same).reshape(len(dev), -1).any(axis=1).sum(), len(dev), np.nonzero(~same.reshape(len(dev), -1).any(axis=1))[0][0],
            dev[name][np.nonzero(~same.reshape(len(dev), -1).any(axis=1))[0][0]], host[name][np.nonzero(~same.reshape(len(dev), -1).any(axis=1))[0][0]])
    assert np.array_equal(dev["inv"].view(np.uint64), host["inv"].view(np.uint64))
    # both overloads of the quantised test agree, and every kind of verdict occurs
    assert (((dev["verdict"] & 1) != 0) == ((dev["verdict"] & 2) != 0)).all()
    assert (dev["verdict"] == 7).sum() > 50000 and (dev["verdict"] == 0).sum() > 5000


def test_filter_rcp_is_within_2_to_minus_49_of_exact_division(pairs):
    """... on normal inputs; the pairs' directions span 1e-32 .. 1e2, a second batch 1e-300 .. 1e300 both signs"""
    rays, grid, ql, qh, words, sets, t, dev = pairs
    rng = np.random.default_rng(1)
    n = 1 << 14
    r2 = rays[:n].copy()
    r2[:, 3:6] = 10.0 ** rng.uniform(-300, 300, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    r2[:64, 3:6] = [[1.0, -1.0, 3.0]] * 64
    inv2 = gpu.slab32_batch(r2, grid[:n], words[:n]).view(sc.PROBE).reshape(-1)["inv"]
    worst = 0.0
    for x, inv in ((rays[sets != 6, 3:6], dev["inv"][sets != 6]), (r2[:, 3:6], inv2)):
        rel = np.abs(inv.astype(sc.LD) * x.astype(sc.LD) - 1)
        assert np.isfinite(inv).all()
        worst = max(worst, float(rel.max()))
    print("filter_rcp: worst relative error %.3g (2^-49 = %.3g)" % (worst, 2.0 ** -49))
    assert worst <= 2.0 ** -49


def test_zero_and_denormal_directions_land_in_the_never_cull_path(pairs):
    rays, grid, ql, qh, words, sets, t, dev = pairs
    m = sets == 6
    d = rays[m, 3:6]
    special = np.abs(d) < 2.0 ** -1025
    assert special.any(axis=1).all()
    assert (~np.isfinite(dev["inv"][m][special])).all()
    for form in ("q", "f"):
        c = dev[form][m].reshape(-1, 3, 3)[special]
        assert (c[:, 0] == 0).all() and (c[:, 1] == np.float32(-1e30)).all() and (c[:, 2] == np.float32(1e30)).all()


def test_constructed_rays_are_accepted_on_the_device(pairs):
    """the construction sets: whatever exact arithmetic accepts the device accepts, with tnear no later than the exact entry distance"""
    rays, grid, ql, qh, words, sets, t, dev = pairs
    for k, bits, tn_name in ((0, 3, "tnear_q"), (1, 3, "tnear_q"), (2, 3, "tnear_q"), (3, 4, "tnear_f")):
        m = sets == k
        if k == 3:
            # (the f32 box the probe decodes; where rounding a flat box's planes to f32 inverted it, no ray passes and none is required to)
            box = sc.f32_box_of(grid[m], ql[m], qh[m])
            inverted = (box[:, 1::2] < box[:, 0::2]).any(axis=1)
            box[:, 1::2] = np.maximum(box[:, 1::2], box[:, 0::2])
            planes = sc.f32_planes(box)
        else:
            planes = sc.decoded_planes(grid[m], ql[m], qh[m])
            inverted = np.zeros(m.sum(), bool)
        acc, tn, tol = sc.exact_box(rays[m, :3], rays[m, 3:6], planes[0], planes[1], planes[2], planes[3], planes[4], rays[m, 6], rays[m, 7])
        acc &= ~inverted
        plain = (rays[m, 6] <= t[m]) & (rays[m, 7] >= t[m]) & (planes[1] > planes[0]).all(axis=1)
        assert acc[plain].mean() > (.5 if k == 2 else .85)
        v = dev["verdict"][m]
        lost = acc & ((v & bits) != bits)
        assert not lost.any(), "set %d: the device rejects %d of %d rays exact arithmetic accepts" % (k, lost.sum(), acc.sum())
        late = acc & ~(dev[tn_name][m].astype(sc.LD) <= tn + tol)
        assert not late.any(), "set %d: tnear above the exact entry distance in %d rows" % (k, late.sum())


def test_quantised_nodes_equal_the_host_twins():
    import test_slab32_cpu as tc
    for g, (origin, ext) in enumerate(tc.QUANT_GRIDS):
        cell = np.maximum(1e-300, ext / 65535. * (1 + 1e-9))
        nodes, empty = tc._nodes(np.random.default_rng(40 + g), 4096, origin, cell, 1.)
        dev = gpu.quantize_nodes(nodes, origin, cell)
        host = sc.quantize(sc.host_lib(int(gpu.build_config("slab_perm"))), nodes, origin, cell)
        assert np.array_equal(dev.reshape(-1), host.view(np.uint8).reshape(-1)), "grid %d" % g
    assert gpu.quantize_nodes(np.zeros(0, sc.NODE), origin, cell).shape == (0, 64)


# ------------------------------------------------------------------ whole walks
def _vertex_rays(v, tris, n, seed):
    """rays aimed at mesh vertices, nudged inside one of the vertex's triangles by 1e-9 .. 1e-6 of its size, from 1 .. 64 mesh extents away;
    every third ray grazes the surface (within 1e-3 .. 1e-1 rad of the triangle's plane)"""
    rng = np.random.default_rng(seed)
    v = v.astype(np.float64)
    tri = tris[rng.integers(0, len(tris), n)]
    P = v[tri]                                              # [n, 3, 3]
    k = rng.integers(0, 3, n)
    vert = P[np.arange(n), k]
    cen = P.mean(axis=1)
    target = vert + (cen - vert) * (10.0 ** rng.uniform(-9, -6, n))[:, None]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1), 1e-300)[:, None]
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    tang = d - (d * nrm).sum(axis=1)[:, None] * nrm
    tang /= np.maximum(np.linalg.norm(tang, axis=1), 1e-300)[:, None]
    graze = tang + nrm * (10.0 ** rng.uniform(-3, -1, n) * rng.choice([-1, 1], n))[:, None]
    graze /= np.linalg.norm(graze, axis=1)[:, None]
    d = np.where((np.arange(n) % 3 == 0)[:, None], graze, d)
    extent = float((v.max(axis=0) - v.min(axis=0)).max())
    o = target - d * (extent * 2.0 ** rng.uniform(0, 6, n))[:, None]
    return np.concatenate([o, d, np.full((n, 1), 1e-4), np.full((n, 1), 1e6)], axis=1)


@pytest.fixture(scope="module")
def vertex_case(tmp_path_factory):
    nu, nv = synth.MESH_CLASSES["teapot"][:2]
    v, q, t = synth.bumpy_sphere(nu, nv, seed=synth.SEED + 6)
    tris = np.concatenate([np.asarray(t).reshape(-1, 3), np.asarray(q)[:, [0, 1, 2]], np.asarray(q)[:, [0, 2, 3]]]).astype(np.int32)
    v = np.asarray(v, np.float32)
    path = pm.write_mesh(tmp_path_factory.mktemp("slab32"), "vertex_mesh", v, tris)
    rays = _vertex_rays(v, tris, 30000, 12)
    text = pm.trace_scene(path)
    to, io = pm.oracle_trace(text, rays)
    assert len(tris) > 4000 and (io[:, 0] >= 0).mean() > .5
    for a in (rays, to, io):
        a.setflags(write=False)
    return text, rays, to, io


@pytest.mark.parametrize("how,flat", [("host_sah", 0), ("radix", 0), ("ploc_root_r16", 0), ("host_sah", 2)])
def test_rays_at_mesh_vertices_from_far_origins_hit_what_the_oracle_hits(how, flat, vertex_case, monkeypatch):
    """t and ids bit-exact against the oracle on the host's, the radix and the clustering tree (general walk) and on the flat walk"""
    from test_gpu_pathological import builder
    text, rays, to, io = vertex_case
    gpu.global_option("flat_groups", flat if flat else 1)
    try:
        with builder(how, monkeypatch):
            sp, _ = tg.prepare(text)
            gs = gpu.Scene(sp)
            t, ids, uv, st = gs.trace(0, rays)
            kernel = int(gs.query("closest_kernel"))
            gs.close()
    finally:
        gpu.global_option("flat_groups", 1)
    assert kernel == (4 if flat else 0)
    assert np.array_equal(t, to)
    assert np.array_equal(ids, io)
