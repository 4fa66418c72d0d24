"""Reader for tests/golden/ref_vectors.bin (written by oracle/ref_vectors.cc) and the golden frames.

A committed fixture stays under 1 MiB: ref_vectors.bin is kept as ref_vectors.bin.part00, .part01, ... (split_file) and
the frames as frames.npz, frames_1.npz, ... (save_frames); the readers put them back together."""
import glob
import io
import os
import struct
import zlib

import numpy as np

PART_BYTES = 1000 * 1000


def split_file(path, part_bytes=PART_BYTES):
    """replace `path` by path.part00, path.part01, ... of at most part_bytes each"""
    data = open(path, "rb").read()
    for old in glob.glob(path + ".part[0-9][0-9]"):
        os.remove(old)
    for k in range(0, max(1, -(-len(data) // part_bytes))):
        with open("%s.part%02d" % (path, k), "wb") as f:
            f.write(data[k * part_bytes:(k + 1) * part_bytes])
    os.remove(path)


def _read_whole(path):
    if os.path.exists(path):
        return open(path, "rb").read()
    parts = sorted(glob.glob(path + ".part[0-9][0-9]"))
    if not parts:
        raise FileNotFoundError(path)
    return b"".join(open(q, "rb").read() for q in parts)


def save_frames(golden_dir, frames, part_bytes=PART_BYTES):
    """frames (name -> array) as frames.npz, frames_1.npz, ...: each compressed file under part_bytes"""
    for old in glob.glob(os.path.join(golden_dir, "frames*.npz")):
        os.remove(old)
    groups, size = [{}], 0
    for name in sorted(frames):
        est = len(zlib.compress(frames[name].tobytes(), 6)) + 1024
        if groups[-1] and size + est > part_bytes * 0.9:
            groups.append({})
            size = 0
        groups[-1][name] = frames[name]
        size += est
    for k, g in enumerate(groups):
        np.savez_compressed(os.path.join(golden_dir, "frames.npz" if k == 0 else "frames_%d.npz" % k), **g)


def load_frames(golden_dir):
    """name -> frame over frames.npz, frames_1.npz, ..."""
    out = {}
    for f in sorted(glob.glob(os.path.join(golden_dir, "frames*.npz"))):
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    return out

_DT = {b"d": np.float64, b"i": np.int32, b"u": np.uint32, b"f": np.float32}


def read_vectors(path):
    out = {}
    with io.BytesIO(_read_whole(path)) as f:
        assert f.read(4) == b"FJGV"
        while True:
            h = f.read(4)
            if len(h) < 4:
                break
            (nl,) = struct.unpack("<I", h)
            name = f.read(nl).decode("ascii")
            dt = _DT[f.read(1)]
            (nd,) = struct.unpack("<I", f.read(4))
            dims = struct.unpack("<%dI" % nd, f.read(4 * nd))
            n = int(np.prod(dims)) if nd else 1
            out[name] = np.frombuffer(f.read(n * np.dtype(dt).itemsize), dtype=dt).reshape(dims).copy()
    return out
