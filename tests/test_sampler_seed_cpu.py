"""Option "sampler_seed" without a GPU (include/fjgpu.h): the host-built tables of the seeded streams and the seeded tile id.

fjgpu_host_xorshift_f01_seeded(seed, n, out) is the table every seeded entry uploads: seed 0 the default-constructed XorShift
(reference src/fj_random.cc:10-16), seed s != 0 XorShift(unsigned seed) (src/fj_random.cc:18-24); NextFloat01 is lines 26-43.  The
restatement below is written from those lines in numpy uint32 arithmetic.  fjgpu_host_seeded_tile_id(seed, id) is what the host writes into
TileDesc.id; the device's sample_uid (csrc/device/fjgpu_dev_shade.h) is restated here to pin the contract of DESIGN.md 4, "Random
streams".
"""
import ctypes as C

import numpy as np
import pytest

from fujiyama_renderer_amd import gpu

M32 = 0xFFFFFFFF


def xorshift_f01(seed, n):
    """the first n NextFloat01() of XorShift() (seed None) or XorShift(seed), src/fj_random.cc:10-43"""
    if seed is None:
        st = [123456789, 362436069, 521288629, 88675123]
    else:
        st, s = [], seed & M32
        for i in range(4):
            s = (1812433253 * (s ^ (s >> 30)) + i) & M32
            st.append(s)
    out = np.zeros(n, dtype=np.float64)
    for k in range(n):
        t = (st[0] ^ (st[0] << 11)) & M32
        st[0], st[1], st[2] = st[1], st[2], st[3]
        st[3] = ((st[3] ^ (st[3] >> 19)) ^ (t ^ (t >> 8))) & M32
        out[k] = np.float64(st[3]) / np.float64(M32)
    return out


def sample_uid(tile_id, k):
    """sample_uid of csrc/device/fjgpu_dev_shade.h"""
    u = ((tile_id & M32) << 20) + k
    return (u & M32) ^ (((u >> 32) & M32) * 0x9E3779B1 & M32)


def seeded(seed, n):
    return gpu.host_xorshift_f01_seeded(seed, n)


def unseeded(n):
    out = np.zeros(n, dtype=np.float64)
    L = gpu.lib()
    L.fjgpu_host_xorshift_f01.argtypes = [C.c_int, C.c_void_p]
    L.fjgpu_host_xorshift_f01.restype = None
    L.fjgpu_host_xorshift_f01(n, out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("seed", [1, 2, 65535])
@pytest.mark.parametrize("n", [0, 1, 4097])
def test_seeded_table_is_the_references_seeded_generator(seed, n):
    got = seeded(seed, n)
    assert got.shape == (n,)
    assert np.array_equal(got, xorshift_f01(seed, n))
    if n:
        assert 0.0 <= got.min() and got.max() <= 1.0


@pytest.mark.parametrize("n", [0, 1, 4097])
def test_seed_0_is_the_unseeded_table_not_xorshift_of_0(n):
    assert np.array_equal(seeded(0, n), unseeded(n))
    assert np.array_equal(seeded(0, n), xorshift_f01(None, n))
    if n:
        assert not np.array_equal(seeded(0, n), xorshift_f01(0, n))


def test_distinct_seeds_give_distinct_tables():
    seeds = [0, 1, 2, 3, 255, 256, 4096, 65534, 65535]
    tabs = [seeded(s, 64) for s in seeds]
    for i in range(len(seeds)):
        for j in range(i + 1, len(seeds)):
            assert not np.array_equal(tabs[i], tabs[j]), (seeds[i], seeds[j])
            assert tabs[i][0] != tabs[j][0], (seeds[i], seeds[j])
    # every accepted seed starts its stream elsewhere
    first = np.array([seeded(s, 1)[0] for s in range(0, 65536, 97)])
    assert len(np.unique(first)) == len(first)


def test_a_longer_table_starts_with_the_shorter_one():
    assert np.array_equal(seeded(7, 1000)[:10], seeded(7, 10))


def test_seeded_tile_id_and_the_uid_contract():
    L = gpu.lib()
    tid = lambda s, t: int(L.fjgpu_host_seeded_tile_id(s, t))
    ks = np.array([0, 1, 2, 1000, (1 << 20) - 1], dtype=np.int64)
    for t in (0, 1, 17, 4095):
        assert tid(0, t) == t                                                # seed 0: today's id, today's uid
        for s in (1, 2, 255, 65535):
            assert tid(s, t) == t + 4096 * s and tid(s, t) < 2 ** 31
            for k in ks:
                assert sample_uid(tid(s, t), int(k)) == sample_uid(t, int(k)) ^ (s * 0x9E3779B1 & M32)
    # under one seed (tile, k) -> uid is injective: the unseeded map xor a constant
    t = np.arange(4096, dtype=np.uint64)[:, None]
    k = np.array([0, 1, 77, 65535, (1 << 20) - 1], dtype=np.uint64)[None, :]
    base = ((t << np.uint64(20)) + k).astype(np.uint64)
    assert base.max() < 2 ** 32 and len(np.unique(base)) == base.size
    # for one sample (tile, k), seed -> uid is injective over the accepted seeds: s -> s * 0x9E3779B1 mod 2^32 is (the constant is odd)
    s = np.arange(65536, dtype=np.uint64)
    fold = (s * np.uint64(0x9E3779B1)) & np.uint64(M32)
    assert len(np.unique(fold)) == 65536
    assert len(np.unique(np.uint64(sample_uid(4095, 12345)) ^ fold)) == 65536
