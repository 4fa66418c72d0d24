"""What the compiled reference answered, recorded, so that the tests that hold the product against it need nothing
outside the repository.

  tests/golden/reference_records.json   per key: the call stream of one of the reference's scene scripts (method name
                                        and arguments of every SceneInterface call it made), the outcome of a failing
                                        command in the reference's parser, SHA-256 digests of files the reference wrote
  tests/golden/reference_frames.npz     float32 RGBA frames the reference rendered (oracle/ref_render)
  tests/golden/reference_scenes/*.scn   the reference's hand-maintained scene files, verbatim

The tests read these.  To record them again, where the reference's source tree and its build (`make -C oracle ref`)
exist, run the tests that use them with the reference live:

    FJ_RECORD_REFERENCE=1 FJ_REFERENCE_DIR=<reference tree> python -m pytest tests -m "not gpu" -k reference

In that mode every helper below asks the reference itself and the files are rewritten when the session ends.
"""
import atexit
import hashlib
import json
import os
import struct
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
RECORDS = os.path.join(GOLDEN, "reference_records.json")
FRAMES = os.path.join(GOLDEN, "reference_frames.npz")
SCENES = os.path.join(GOLDEN, "reference_scenes")
REF_BUILT = os.path.join(ROOT, "oracle", "_ref")

RECORDING = os.environ.get("FJ_RECORD_REFERENCE") == "1"
REF_DIR = os.environ.get("FJ_REFERENCE_DIR", "")

_records = None
_frames = None


def _load():
    global _records, _frames
    if _records is None:
        _records = json.load(open(RECORDS)) if os.path.exists(RECORDS) else {}
        _frames = dict(np.load(FRAMES)) if os.path.exists(FRAMES) else {}
        if RECORDING:
            if not (os.path.isdir(os.path.join(REF_DIR, "scenes")) and os.path.exists(os.path.join(REF_BUILT, "ref_render"))):
                raise RuntimeError("FJ_RECORD_REFERENCE=1 needs FJ_REFERENCE_DIR=<reference tree> and oracle/_ref (make -C oracle ref)")
            atexit.register(_save)


def _save():
    with open(RECORDS, "w") as f:
        json.dump(_records, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(FRAMES, **_frames)


def _get(key):
    _load()
    if key not in _records:
        raise KeyError("no recorded reference answer %r in %s" % (key, os.path.relpath(RECORDS, ROOT)))
    return _records[key]


def _put(key, value):
    _load()
    _records[key] = value
    return value


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


# ---------------------------------------------------------------- scene scripts and scene files
def script_calls(name):
    """the SceneInterface calls scenes/<name>.py makes, in order: [[method, [args...]], ...]"""
    key = "script_calls/" + name
    if not RECORDING:
        return _get(key)
    import runpy
    import sys
    import types
    calls = []

    class Recorder(object):
        def __getattr__(self, method):
            def call(*a):
                calls.append([method, list(a)])
                return 0
            return call
    mod = types.ModuleType("fujiyama")
    mod.SceneInterface = lambda *a, **k: Recorder()
    saved = sys.modules.get("fujiyama"), sys.argv
    sys.modules["fujiyama"], sys.argv = mod, [name + ".py"]
    try:
        runpy.run_path(os.path.join(REF_DIR, "scenes", name + ".py"), run_name="__main__")
    finally:
        if saved[0] is None:
            sys.modules.pop("fujiyama", None)
        else:
            sys.modules["fujiyama"] = saved[0]
        sys.argv = saved[1]
    return _put(key, calls)


def scene_file(name):
    """text of the reference's scenes/<name>.scn"""
    path = os.path.join(SCENES, name + ".scn")
    if RECORDING:
        os.makedirs(SCENES, exist_ok=True)
        text = open(os.path.join(REF_DIR, "scenes", name + ".scn")).read()
        with open(path, "w") as f:
            f.write(text)
    return open(path).read()


# ---------------------------------------------------------------- the reference's renderer and tools
def _ref_env():
    return dict(os.environ, LD_LIBRARY_PATH=REF_BUILT)


def render(key, scn, fb_path=None):
    """the frame the reference renders from the scene file `scn` (oracle/ref_render); with `fb_path`, also the SHA-256 of
    the .fb file its SaveFrameBuffer wrote there: (frame, digest)"""
    if RECORDING:
        _load()
        subprocess.run([os.path.join(REF_BUILT, "ref_render"), scn, scn + ".fjfb"], check=True, env=_ref_env(),
                       stdout=subprocess.DEVNULL, timeout=900)
        with open(scn + ".fjfb", "rb") as f:
            b = f.read()
        w, h, c = struct.unpack("<iii", b[4:16])
        _frames[key] = np.frombuffer(b[24:], dtype=np.float32).reshape(h, w, c).copy()
        if fb_path is not None:
            _put("fb_sha256/" + key, sha256(fb_path))
    _load()
    if key not in _frames:
        raise KeyError("no recorded reference frame %r in %s" % (key, os.path.relpath(FRAMES, ROOT)))
    return _frames[key].copy(), (_get("fb_sha256/" + key) if fb_path is not None else None)


def failing_command(key, scn):
    """how the reference's parser ends on the scene file `scn`: {"returncode", "failing_line": [line, text] or None,
    "stdout_stderr": the lines it echoed}"""
    if not RECORDING:
        return _get("failing_command/" + key)
    import re
    p = subprocess.run([os.path.join(REF_BUILT, "ref_render"), scn, scn + ".fjfb"], env=_ref_env(), capture_output=True, text=True,
                       timeout=120)
    m = re.search(r"error: .*?: (\d+): (.*)", p.stderr + p.stdout)
    echoed = [ln for ln in (p.stdout + p.stderr).splitlines() if ln.startswith("-- ")]
    return _put("failing_command/" + key, {"returncode": p.returncode, "failing_line": [int(m.group(1)), m.group(2).strip()] if m else None,
                                           "echoed": echoed})


def hdr2mip_sha256(key, hdr, tmp_dir):
    """SHA-256 of the .mip the reference's hdr2mip converter writes from `hdr`"""
    if not RECORDING:
        return _get("hdr2mip_sha256/" + key)
    out = os.path.join(tmp_dir, "ref.mip")
    subprocess.run([os.path.join(REF_BUILT, "hdr2mip"), hdr, out], check=True, stdout=subprocess.DEVNULL, env=_ref_env())
    return _put("hdr2mip_sha256/" + key, sha256(out))
