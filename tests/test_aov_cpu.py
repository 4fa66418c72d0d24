"""The AOV entry points (include/fjgpu.h: fjgpu_render_aov, fjgpu_camera_samples) as far as they go without a GPU:
exported, refusing NULL arguments with a message, and no way round the device."""
import ctypes as C

import pytest

from fujiyama_renderer_amd import ffi, gpu, host, workloads

FJGPU_ENODEV, FJGPU_EINVAL = -1, -2


def _err():
    return gpu.lib().fjgpu_last_error().decode("utf-8", "replace")


def test_library_exports_the_entry_points():
    L = gpu.lib()
    assert callable(L.fjgpu_render_aov) and callable(L.fjgpu_camera_samples)
    # the binding's struct is fjgpu_aov_buffers: six pointers, in the header's order
    assert C.sizeof(ffi.AovBuffers) == 6 * C.sizeof(C.c_void_p)
    assert [n for n, _ in ffi.AovBuffers._fields_] == list(gpu.AOV_NAMES) == ["depth", "position", "normal", "uv", "ids", "coverage"]
    assert hasattr(gpu.Scene, "render_aov") and hasattr(gpu.Scene, "camera_samples")


def test_null_arguments_are_refused_with_a_message():
    L = gpu.lib()
    rd = ffi.RenderDesc()
    bufs = ffi.AovBuffers()
    st = ffi.GpuStats()
    assert L.fjgpu_render_aov(None, C.byref(rd), None, 0, C.byref(bufs), None, C.byref(st)) == FJGPU_EINVAL
    assert "fjgpu_render_aov" in _err() and "null" in _err().lower()
    assert L.fjgpu_render_aov(None, None, None, 0, None, None, None) == FJGPU_EINVAL
    assert L.fjgpu_camera_samples(None, C.byref(rd), 0, None, 0) == FJGPU_EINVAL
    assert "fjgpu_camera_samples" in _err() and "null" in _err().lower()
    assert L.fjgpu_camera_samples(None, None, 0, None, 0) == FJGPU_EINVAL


def test_unknown_aov_name_is_a_python_error():
    class _NoScene(gpu.Scene):
        def __init__(self):
            self._h = C.c_void_p()
            self._device = 0
    with pytest.raises(ValueError, match="unknown AOV"):
        _NoScene().render_aov(ffi.RenderDesc(), want=("depth", "albedo"))


def test_without_a_device_scene_creation_still_fails(asset_dir):
    """there is no CPU path to an AOV: without a device no scene exists to call it on (as before)"""
    if gpu.device_count() > 0:
        pytest.skip("a GPU is present: the device path is covered by tests/test_gpu_aov.py")
    host.run_scene_text(workloads.teapot(asset_dir, res=(16, 16), spp=(1, 1), mesh="tiny"), deferred=True)
    sp, _ = host.get_desc()
    h = C.c_void_p()
    assert gpu.lib().fjgpu_scene_create(sp, 0, C.byref(h)) == FJGPU_ENODEV
    assert not h.value and _err()
    with pytest.raises(gpu.GpuError):
        gpu.Scene(sp)
