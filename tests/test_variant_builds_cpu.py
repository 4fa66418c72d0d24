"""The two variant builds of the product libraries that __graft_entry__.build() makes beside the default one (csrc/Makefile, targets stack4 and
validate) are what their names say: both libraries are there, and each libfjgpu.so reports the constants it was compiled with
(fjgpu_build_config, which needs no device).  A variant that silently fell back to the default flags would pass every comparison of
tests/test_gpu_variant_builds.py without reaching the code those tests are about.

ffi.LIB_DIR is read at import, so every library is asked in a child process of its own."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fujiyama-renderer_amd")
LIB_DIRS = {"default": os.path.join(PKG, "lib"), "stack4": os.path.join(PKG, "lib_var", "stack4"), "validate": os.path.join(PKG, "lib_var", "validate")}

STACK_NAMES = ("stack_lds", "stack_lds_curves", "stack_lds_anyhit", "stack_lds_canyhit", "stack_lds_min")
SWITCHES = ("tri_filter_validate", "light_cone_validate", "light_hull_validate")
DEFAULT_STACK = dict(zip(STACK_NAMES, (32, 20, 12, 16, 12)))
EXPECTED = {
    "default": dict(DEFAULT_STACK, **{s: 0 for s in SWITCHES}),
    "stack4": dict({n: 4 for n in STACK_NAMES}, **{s: 0 for s in SWITCHES}),
    "validate": dict(DEFAULT_STACK, **{s: 1 for s in SWITCHES}),
}

ASK = """
import json, sys
sys.path.insert(0, %r)
from fujiyama_renderer_amd import ffi, gpu
out = {"lib_dir": ffi.LIB_DIR, "config": {n: gpu.build_config(n) for n in %r}}
try:
    gpu.build_config("no_such_name")
    out["unknown"] = "accepted"
except gpu.GpuError as e:
    out["unknown"] = str(e)
print(json.dumps(out))
"""


def ensure_variant(variant):
    """the variant's directory, built now if build() has not left it (one make call, objects in csrc/build/var_<variant>)"""
    d = LIB_DIRS[variant]
    if variant != "default" and not all(os.path.exists(os.path.join(d, n)) for n in ("libfjgpu.so", "libfjscene.so")):
        r = subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", os.path.join(PKG, "csrc"), variant],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout[-4000:]
    return d


@pytest.mark.parametrize("variant", ["stack4", "validate"])
def test_build_leaves_both_libraries_of_the_variant(variant):
    """after build() -- conftest's session fixture ran it if the default libraries were missing -- both directories hold both libraries"""
    import __graft_entry__
    if not os.path.exists(os.path.join(LIB_DIRS[variant], "libfjgpu.so")):
        __graft_entry__.build()
    for name in ("libfjgpu.so", "libfjscene.so"):
        assert os.path.getsize(os.path.join(LIB_DIRS[variant], name)) > 0


@pytest.mark.parametrize("variant", ["default", "stack4", "validate"])
def test_the_library_reports_what_it_was_built_with(variant):
    env = dict(os.environ)
    env.pop("FJGPU_LIBDIR", None)
    if variant != "default":
        env["FJGPU_LIBDIR"] = ensure_variant(variant)
    r = subprocess.run([sys.executable, "-c", ASK % (ROOT, STACK_NAMES + SWITCHES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert os.path.samefile(got["lib_dir"], LIB_DIRS[variant])
    assert got["config"] == EXPECTED[variant]
    assert all(float(v) == int(v) for v in got["config"].values())
    assert "fjgpu error -2" in got["unknown"] and "no_such_name" in got["unknown"]         # FJGPU_EINVAL
