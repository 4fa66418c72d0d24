"""The frames and rectangle lists that tests/test_accumulate_cpu.py and tests/test_gpu_accumulate.py share: a 37 x 23 frame (no multiple of
the 16 x 16 patch, more than one patch either way) and four lists of rectangles."""
import numpy as np

W, H = 37, 23
SENTINEL = np.float32(-123.25)
LUM_FLOOR = 1e-3

RECTS = {
    "whole": None,
    "whole_listed": [(0, 0, W, H)],
    "ragged_split": [(x0, y0, min(x0 + 16, W), min(y0 + 16, H)) for y0 in range(0, H, 16) for x0 in range(0, W, 16)],
    "one_pixel": [(5, 7, 6, 8)],
    "two_disjoint": [(1, 2, 20, 9), (22, 10, W, H)],
}


def aligned(shape, fill=0.0):
    """a float32 array of `shape` whose data is 16-byte aligned"""
    n = int(np.prod(shape))
    raw = np.empty(n * 4 + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + 4 * n].view(np.float32).reshape(shape)
    a[...] = fill
    return a


def frames(n, seed=11, amplitude=0.5, h=H, w=W):
    """n frames [h, w, 4] f32: a smooth base colour per pixel plus uniform noise of `amplitude` times it, alpha in [0, 1]"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.3 + 0.6 * xx / w, 0.2 + 0.7 * yy / h, 0.5 + 0.4 * np.sin(xx * 0.7 + yy * 0.3), np.ones_like(xx, dtype=float)], axis=2)
    out = []
    for _ in range(n):
        f = base * (1.0 + amplitude * (2.0 * rng.rand(h, w, 4) - 1.0))
        f[..., 3] = rng.rand(h, w)
        a = aligned((h, w, 4))
        a[...] = f.astype(np.float32)
        out.append(a)
    return out


def inside(rects, h=H, w=W):
    """bool [h, w]: the pixels of the list"""
    m = np.zeros((h, w), dtype=bool)
    for x0, y0, x1, y1 in ([(0, 0, w, h)] if rects is None else rects):
        m[y0:y1, x0:x1] = True
    return m


def ulp_distance(a, b):
    """units in the last place between two f32 arrays of finite values of one sign convention (monotone integer mapping)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
