"""CPU suite, part 2: the drop-in boundary -- C-ABI export lists, the Si* scene
API / command parser semantics, the Py3 emitter, and loud failure without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fujiyama_renderer_amd import ffi, fujiyama, gpu, host, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_records  # noqa: E402
HAVE_GPU = gpu.device_count() > 0


def _declared(header, prefix):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, text)))


def _exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ffi.LIB_DIR, lib)],
                         stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_libfjgpu_exports_every_declared_symbol():
    names = _declared("fjgpu.h", "fjgpu_")
    assert len(names) >= 13
    exp = _exported("libfjgpu.so")
    assert [n for n in names if n not in exp] == []


def test_libfjscene_exports_c_and_cxx_api():
    names = _declared("fj_scene_interface.h", "fj_")
    assert len([n for n in names if n.startswith("fj_Si")]) == 41       # every one of the 41 Si functions has its C twin
    exp = _exported("libfjscene.so")
    assert [n for n in names if n not in exp] == []
    # the C++ spelling (namespace fj, Itanium mangling) of the 41-function interface
    cxx = [s for s in exp if s.startswith("_ZN2fj2Si") or s.startswith("_ZN2fj")]
    for fn in ("SiOpenScene", "SiRenderScene", "SiNewMesh", "SiSetProperty3", "SiAssignShader",
               "SiSetSampleProperty3", "SiSetTileReportCallback", "SiGetPropertyList"):
        assert any(fn in s for s in cxx), fn


def test_libraries_load_and_report_no_device_loudly(asset_dir):
    assert isinstance(gpu.device_count(), int)
    if HAVE_GPU:
        pytest.skip("GPU present: the no-device failure path cannot be exercised")
    host.run_scene_text(workloads.teapot(asset_dir, res=(32, 32), spp=(1, 1), mesh="tiny"), deferred=True)
    sp, rd = host.get_desc()
    with pytest.raises(gpu.GpuError) as e:
        gpu.Scene(sp)
    assert "no CPU fallback" in str(e.value)
    # and through the host API: RenderScene fails, the parser reports the line
    with pytest.raises(host.SceneError) as e2:
        host.run_scene_text(workloads.teapot(asset_dir, res=(32, 32), spp=(1, 1), mesh="tiny"), deferred=False)
    assert "RenderScene" in str(e2.value) and "no CPU fallback" in str(e2.value)


def test_global_options_and_host_build_paths_without_a_device(asset_dir):
    """process-wide options of the core are validated without a GPU, and scene creation walks
    the whole host-side preparation (flatten, BLAS build or its device-build bypass, instance
    boxes, light tables) before it reports the missing device"""
    gpu.global_option("device_build", 1)
    gpu.global_option("device_build", -1)
    with pytest.raises(gpu.GpuError) as e:
        gpu.global_option("no_such_option", 1)
    assert "unknown global option" in str(e.value)
    if HAVE_GPU:
        return
    for builder, kw in (("motion", dict(res=(32, 24), spp=(1, 1), mesh="tiny", kind="velocity+object")),
                        ("arealights", dict(res=(32, 24), spp=(1, 1), mesh="tiny", kind="both")),
                        ("furry", dict(res=(32, 24), spp=(1, 1), mesh="furball", nlights=2, hair=True))):
        for dev in (0, 1):
            gpu.global_option("device_build", dev)
            try:
                host.run_scene_text(workloads.BUILDERS[builder](asset_dir, **kw), deferred=True)
                sp, rd = host.get_desc()
                with pytest.raises(gpu.GpuError) as e:
                    gpu.Scene(sp)
                assert "no CPU fallback" in str(e.value)
            finally:
                gpu.global_option("device_build", -1)


def test_parser_grammar_and_errors(asset_dir):
    ok = "# comment\n\nNewCamera cam1 PerspectiveCamera\nSetProperty3 cam1 translate 0 1 7\nSetProperty1 cam1 rotate_order ORDER_XYZ\n"
    assert host.run_scene_text(ok, deferred=True) == 0
    cases = {
        "Frobnicate x\n": "unknown command",
        "NewCamera cam1\n": "too few arguments",
        "NewCamera cam1 a b\n": "too many arguments",
        "NewCamera c x\nNewCamera c x\n": "already exists",
        "SetProperty1 nosuch fov 30\n": "not found",
        "NewCamera c x\nSetProperty1 c fov abc\n": "bad number",
        "NewCamera c x\nSetProperty3 c fov 1 2 3\n": "command failed",     # arity must match the property
        "NewLight l LaserLight\n": "bad light type",
        "OpenPlugin p /x/UnknownShader.so\n": "no device implementation",
        "NewTexture t /nonexistent/file.mip\n": "cannot load texture",
        "NewVolume v\n": "outside the device path",
    }
    for text, msg in cases.items():
        with pytest.raises(host.SceneError) as e:
            host.run_scene_text(text, deferred=True)
        assert msg in str(e.value), (text, str(e.value))
    with pytest.raises(host.SceneError) as e:
        host.run_scene_text("NewCamera a x\n\nBogus\n", deferred=True)
    assert ": 3: Bogus" in str(e.value)            # 1-based line number + the line, like bin/scene


def test_renderer_defaults_and_property_semantics():
    text = ("NewCamera cam1 PerspectiveCamera\nNewFrameBuffer fb1 rgba\nNewRenderer ren1\n"
            "AssignCamera ren1 cam1\nAssignFrameBuffer ren1 fb1\n%sRenderScene ren1\n")
    host.run_scene_text(text % "", deferred=True)
    _, rd = host.get_desc()
    # defaults of src/internal/fj_property_list_include.cc:451-473
    assert (rd.xres, rd.yres, rd.tile_w, rd.tile_h, rd.rate_x, rd.rate_y) == (320, 240, 32, 32, 3, 3)
    assert (rd.filter_w, rd.filter_h, rd.jitter, rd.cast_shadow) == (2.0, 2.0, 1.0, 1)
    assert (rd.max_diffuse_depth, rd.max_reflect_depth, rd.max_refract_depth) == (3, 3, 3)
    assert tuple(rd.region) == (0, 0, 320, 240) and (rd.time_start, rd.time_end) == (0.0, 1.0)
    assert (rd.sampler_type, rd.adaptive_max_subdivision) == (0, 1) and abs(rd.adaptive_subdivision_threshold - .05) < 1e-8
    # sampler selection (Renderer::SetSamplerType: unknown types fall back to the fixed grid)
    host.run_scene_text(text % ("SetProperty1 ren1 sampler_type 1\nSetProperty1 ren1 adaptive_max_subdivision 3\n"
                                "SetProperty1 ren1 adaptive_subdivision_threshold 0.02\n"), deferred=True)
    _, rd = host.get_desc()
    assert (rd.sampler_type, rd.adaptive_max_subdivision) == (1, 3) and abs(rd.adaptive_subdivision_threshold - .02) < 1e-8
    host.run_scene_text(text % "SetProperty1 ren1 sampler_type 7\n", deferred=True)
    assert host.get_desc()[1].sampler_type == 0
    with pytest.raises(Exception):
        host.run_scene_text(text % "SetProperty1 ren1 adaptive_max_subdivision -1\n", deferred=True)
    # resolution resets the render region; a later render_region sticks
    host.run_scene_text(text % "SetProperty4 ren1 render_region 1 2 3 4\nSetProperty2 ren1 resolution 64 48\n", deferred=True)
    _, rd = host.get_desc()
    assert tuple(rd.region) == (0, 0, 64, 48)
    host.run_scene_text(text % "SetProperty2 ren1 resolution 64 48\nSetProperty4 ren1 render_region 8 8 40 32\n", deferred=True)
    _, rd = host.get_desc()
    assert tuple(rd.region) == (8, 8, 40, 32)
    fb = host.framebuffer(0)
    assert fb.shape == (48, 64, 4) and not fb.any()      # Resize(x, y, 4) at RenderScene


def test_python_emitter_matches_command_language(asset_dir):
    si = fujiyama.SceneInterface(argv=["-R", "80", "60", "-S", "2", "2"])
    si.OpenPlugin("plastic_shader", "PlasticShader")
    si.NewCamera("cam1", "PerspectiveCamera")
    si.SetProperty3("cam1", "translate", 0, 1.5, 7)
    si.NewFrameBuffer("fb1", "rgba")
    si.NewRenderer("ren1")
    si.AssignCamera("ren1", "cam1")
    si.AssignFrameBuffer("ren1", "fb1")
    si.RenderScene("ren1")
    lines = si.text().splitlines()
    assert lines[0] == "OpenPlugin plastic_shader PlasticShader.so"      # DSO extension appended
    assert lines[2] == "SetProperty3 cam1 translate 0 1.5 7"
    assert lines[-3:] == ["SetProperty2 ren1 resolution 80 60", "SetProperty2 ren1 pixelsamples 2 2", "RenderScene ren1"]
    with pytest.raises(TypeError):
        si.SetProperty3("cam1", "translate", 1, 2)
    host.run_scene_text(si.text(), deferred=True)
    _, rd = host.get_desc()
    assert (rd.xres, rd.yres, rd.rate_x) == (80, 60, 2)


def test_workload_scene_structure(asset_dir):
    """C2: 16 instances of one mesh + floor + dome, shadow group of the 16, all-objects target"""
    host.run_scene_text(workloads.buddhas(asset_dir, res=(64, 36), spp=(1, 1), mesh="tiny"), deferred=True)
    sp, rd = host.get_desc()

    class SD(C.Structure):
        _fields_ = [("n", C.c_int32 * 7), ("target_group", C.c_int32)]
    d = C.cast(sp, C.POINTER(SD)).contents
    n_meshes, n_curves, n_tex, n_shaders, n_lights, n_inst, n_groups = list(d.n)
    assert (n_meshes, n_curves, n_tex, n_shaders, n_lights, n_inst) == (3, 0, 1, 18, 32, 18)
    assert n_groups == 2 and d.target_group == 1


class _MeshDesc(C.Structure):            # fj_mesh_desc, include/fj_scene_desc.h
    _fields_ = [("n_points", C.c_int32), ("n_faces", C.c_int32), ("P", C.POINTER(C.c_double)), ("N", C.POINTER(C.c_double)),
                ("uv", C.POINTER(C.c_float)), ("velocity", C.POINTER(C.c_double)), ("indices", C.POINTER(C.c_int32)),
                ("face_group", C.POINTER(C.c_int32)), ("bounds", C.c_double * 6), ("vertex_N", C.POINTER(C.c_double))]


class _SceneHead(C.Structure):           # the head of fj_scene_desc
    _fields_ = [("n", C.c_int32 * 7), ("target_group", C.c_int32), ("meshes", C.POINTER(_MeshDesc))]


def test_wavefront_obj_procedure_face_groups_and_corner_normals(asset_dir):
    """WavefrontObjProcedure (reference procedures/wavefrontobj_procedure: ObjParser.cc:158-236, ObjBuffer.h:55-146, ObjBuffer.cc:6-116)
    through the product's reader: fan triangulation, groups in order of first appearance with the default group 0 in front, point normals
    accumulated when the file has no `vn`, per-corner normals (relative indices, creases) when it has; instance shader lists with an
    unassigned slot.  (The pictures these meshes give are pinned against the compiled reference: edge cases obj_face_groups / obj_vertex_normals.)"""
    import edge_scenes
    host.run_scene_text(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["obj_face_groups"]), deferred=True)
    sp, _ = host.get_desc()
    d = C.cast(sp, C.POINTER(_SceneHead)).contents
    m = d.meshes[2]                                   # floor, dome, the OBJ object
    nf = m.n_faces
    assert m.n_points == 98 and nf == 192             # 12 x 9 bumpy sphere: 84 quads -> 168 triangles, + 24 cap triangles
    groups = np.ctypeslib.as_array(m.face_group, shape=(nf,))
    assert sorted(set(groups.tolist())) == [0, 1, 2, 3, 4] and groups[0] == 0
    # (faces are written band by band: default, A, B, C, D, then A again -- the id of a group is fixed at its first `g` line)
    first = [int(np.argmax(groups == g)) for g in range(5)]
    assert first == sorted(first) and groups[-1] == 1
    assert bool(m.N) and not bool(m.vertex_N)
    N = np.ctypeslib.as_array(m.N, shape=(m.n_points, 3))
    assert np.allclose(np.linalg.norm(N, axis=1), 1.0)
    P = np.ctypeslib.as_array(m.P, shape=(m.n_points, 3))
    assert np.array_equal(P, P.astype(np.float32).astype(np.float64))          # f32 values written exactly: the lean any-hit walk takes this mesh

    host.run_scene_text(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["obj_vertex_normals"]), deferred=True)
    sp, _ = host.get_desc()
    d = C.cast(sp, C.POINTER(_SceneHead)).contents
    m = d.meshes[2]
    assert m.n_faces == 192 and bool(m.vertex_N) and not bool(m.N)
    vN = np.ctypeslib.as_array(m.vertex_N, shape=(m.n_faces, 3, 3)).copy()
    ix = np.ctypeslib.as_array(m.indices, shape=(m.n_faces, 3)).copy()
    P = np.ctypeslib.as_array(m.P, shape=(m.n_points, 3)).copy()
    assert not np.array_equal(P, P.astype(np.float32).astype(np.float64))      # arbitrary doubles: the FP64 triangle records
    # a crease: some point carries different normals on different faces
    by_point = {}
    for f in range(m.n_faces):
        for k in range(3):
            by_point.setdefault(int(ix[f, k]), set()).add(tuple(np.round(vN[f, k], 12)))
    assert max(len(v) for v in by_point.values()) >= 2
    # the flat faces carry their own (unnormalised) face normal on all three corners
    flat = [f for f in range(m.n_faces) if np.array_equal(vN[f, 0], vN[f, 1]) and np.array_equal(vN[f, 1], vN[f, 2])]
    assert len(flat) >= 40
    f = flat[0]
    ng = np.cross(P[ix[f, 1]] - P[ix[f, 0]], P[ix[f, 2]] - P[ix[f, 0]])
    assert abs(np.dot(ng / np.linalg.norm(ng), vN[f, 0] / np.linalg.norm(vN[f, 0]))) > 0.999999
    groups = np.ctypeslib.as_array(m.face_group, shape=(m.n_faces,))
    assert sorted(set(groups.tolist())) == [0, 1]


def test_wavefront_obj_procedure_errors(tmp_path, asset_dir):
    """missing file, a file without faces, an index past the vertices: SiRunProcedure fails (wavefrontobj_procedure.cc:77-99 returns -1)"""
    head = ("OpenPlugin wavefrontobj_procedure WavefrontObjProcedure.so\nNewMesh m\nNewProcedure p wavefrontobj_procedure\nAssignMesh p mesh m\n"
            "SetStringProperty p filepath %s\nRunProcedure p\n")
    bad = tmp_path / "bad.obj"
    for text in (None, "v 0 0 0\nv 1 0 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 7\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1 2 3\n"):
        if text is None:
            path = tmp_path / "absent.obj"
        else:
            bad.write_text(text)
            path = bad
        with pytest.raises(RuntimeError):
            host.run_scene_text(head % path, deferred=True)


def test_curve_generator_random_stream_is_glibc_rand():
    """CurveGeneratorProcedure seeds libc's generator per (face, strand) and takes the first values after it (curve_generator_procedure.cc:171-186);
    the library computes that stream itself (thread-safe, libc-independent): held here against the C library's own srand / rand on this host
    (glibc -- the library the reference's golden frames were made with)"""
    L = host.lib()
    L.fj_dev_seeded_rand.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
    L.fj_dev_seeded_rand.restype = None
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    rng = np.random.RandomState(5)
    seeds = [0, 1, 2, 12, 49, 1232, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1] + [int(x) for x in rng.randint(0, 2 ** 32, size=200, dtype=np.uint64)]
    out = (C.c_uint32 * 40)()
    for sd in seeds:
        L.fj_dev_seeded_rand(sd, 40, out)
        libc.srand(C.c_uint(sd))
        assert [libc.rand() for _ in range(40)] == list(out), sd


def test_save_framebuffer_text_format(tmp_path):
    out = tmp_path / "x.fb"
    text = ("NewCamera cam1 PerspectiveCamera\nNewFrameBuffer fb1 rgba\nNewRenderer ren1\nAssignCamera ren1 cam1\n"
            "AssignFrameBuffer ren1 fb1\nSetProperty2 ren1 resolution 4 2\nRenderScene ren1\nSaveFrameBuffer fb1 %s\n" % out)
    host.run_scene_text(text, deferred=True)
    lines = out.read_text().splitlines()
    assert lines[0] == "#PTO Plain Text Object" and lines[2] == "resolution 4 2" and lines[3] == "channel_count 4"
    assert lines[4] == "begin pixels" and lines[-1] == "end pixels" and len(lines) == 4 * 2 + 6


REF_SHADERS = "/root/reference/shaders"


# (the five sources compiled against include/ by `make -C oracle ref`, which build() runs where the reference tree is present)
ABI_SHADERS = os.path.join(ROOT, "oracle", "_ref", "abi_shaders")


@pytest.mark.skipif(not (os.path.exists(os.path.join(ABI_SHADERS, "constant_retabled.so")) or os.path.isdir(REF_SHADERS)),
                    reason="needs the reference's shader sources, or oracle/_ref/abi_shaders built from them")
def test_reference_shader_sources_load_as_plugins_through_the_dso_abi(tmp_path):
    """The Shader plugin ABI (include/fj_plugin_abi.h).  The reference's five shader sources are
    compiled UNCHANGED against include/ (they only #include "fj_shader.h"), the DSOs are opened by
    SiOpenPlugin through the reference's protocol -- dlopen, Initialize(PluginInfo *), validation
    (src/fj_plugin.cc:28-69) -- and identified by PluginInfo.plugin_name, not by file name.  The
    DSO's own Property table is what SiGetPropertyList returns, its defaults equal the built-in
    table of the device twin, and its setters are driven by SiSetProperty*."""
    L = host.lib()
    L.fj_SiOpenPlugin.restype = C.c_long
    L.fj_SiOpenPlugin.argtypes = [C.c_char_p]
    L.fj_SiNewShader.restype = C.c_long
    L.fj_SiNewShader.argtypes = [C.c_long]
    L.fj_SiSetProperty3.argtypes = [C.c_long, C.c_char_p, C.c_double, C.c_double, C.c_double]
    L.fj_SiSetProperty1.argtypes = [C.c_long, C.c_char_p, C.c_double]
    L.fj_scene_property_table.restype = C.c_int
    L.fj_scene_property_table.argtypes = [C.c_char_p, C.c_char_p, C.c_int]

    def table(name):
        buf = C.create_string_buffer(8192)
        n = L.fj_scene_property_table(name.encode(), buf, len(buf))
        return None if n < 0 else buf.value.decode().splitlines()

    builtins = {}
    L.fj_SiOpenScene()
    assert table("PlasticShader") is None                     # a plugin's table exists once it is opened
    for name in ("PlasticShader", "GlassShader", "ConstantShader", "HairShader", "PathtracingShader"):
        assert L.fj_SiOpenPlugin(name.encode()) >= 0           # no DSO of that name around: the built-in twin, by name
        builtins[name] = table(name)
        assert builtins[name]
    L.fj_SiCloseScene()

    # the same five, now as DSOs built from the reference's sources against OUR headers, under
    # file names that say nothing about what is inside
    L.fj_SiOpenScene()
    for k, (src, name) in enumerate((("plastic", "PlasticShader"), ("glass", "GlassShader"), ("constant", "ConstantShader"),
                                     ("hair", "HairShader"), ("pathtracing", "PathtracingShader"))):
        so = str(tmp_path / ("plugin_%d.so" % k))
        built = os.path.join(ABI_SHADERS, "%s_shader.so" % src)
        if os.path.exists(built):
            shutil.copy(built, so)
        else:
            subprocess.run(["g++", "-std=c++11", "-O1", "-fPIC", "-shared", "-w", "-I" + os.path.join(ROOT, "include"),
                            "-o", so, "%s/%s_shader/%s_shader.cc" % (REF_SHADERS, src, src)], check=True)
        und = subprocess.run(["nm", "-D", "--undefined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
        need = [l.split()[-1] for l in und.splitlines() if "_ZN" in l and "2fj" in l or "_ZTIN2fj" in l]
        exp = _exported("libfjscene.so")
        assert [s for s in need if s not in exp] == []        # every fj:: symbol the DSO imports is exported
        pid = L.fj_SiOpenPlugin(so[:-3].encode())             # ".so" is appended like OsDlopen does
        assert pid >= 0, host.lib().fj_scene_last_error()
        assert table(name) == builtins[name], (name, table(name), builtins[name])
        sid = L.fj_SiNewShader(pid)
        assert sid >= 0
        if name != "ConstantShader":
            assert L.fj_SiSetProperty1(sid, b"roughness", .25) == 0
        assert L.fj_SiSetProperty3(sid, b"diffuse", .1, .2, .3) == 0
        assert L.fj_SiSetProperty3(sid, b"no_such_property", 1, 2, 3) == -1
        assert L.fj_SiSetProperty1(sid, b"diffuse", 1) == -1               # PropFind is by type AND name
    L.fj_SiCloseScene()

    # a whole scene through the DSOs: the flat description the HIP core receives (shader
    # parameters after the setters' clamps included) is the one the built-in twins produce --
    # checked through the CPU oracle, which reads nothing but that description
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi
    text = workloads.teapot(str(tmp_path / "assets"), res=(32, 32), spp=(1, 1), mesh="tiny", nlights=3)
    frames = []
    for use_dso in (False, True):
        t = text
        if use_dso:
            t = t.replace("OpenPlugin plastic_shader PlasticShader", "OpenPlugin plastic_shader %s" % (tmp_path / "plugin_0"))
            t = t.replace("OpenPlugin glass_shader GlassShader", "OpenPlugin glass_shader %s" % (tmp_path / "plugin_1"))
            t = t.replace("OpenPlugin constant_shader ConstantShader", "OpenPlugin constant_shader %s" % (tmp_path / "plugin_2"))
            assert t.count("plugin_") == 3
        host.run_scene_text(t, deferred=True)
        sp, rd = host.get_desc()
        osc = oracle_ffi.OracleScene(sp)
        frames.append(osc.render(rd, threads=2)[0])
        osc.close()
    assert frames[0][..., 3].max() > 0 and np.array_equal(frames[0], frames[1])
    host.close_scene()

    # a DSO that is no plugin, and one whose plugin has no device twin
    L.fj_SiOpenScene()
    bad = str(tmp_path / "not_a_plugin.so")
    (tmp_path / "x.cc").write_text("int forty_two() { return 42; }\n")
    subprocess.run(["g++", "-fPIC", "-shared", "-o", bad, str(tmp_path / "x.cc")], check=True)
    assert L.fj_SiOpenPlugin(bad.encode()) == -1 and L.fj_SiGetErrorNo() == 6      # SI_ERR_INIT_PLUGIN_FUNC_NOT_EXIST
    other = str(tmp_path / "other.so")
    if os.path.exists(os.path.join(ABI_SHADERS, "constant_renamed.so")):
        shutil.copy(os.path.join(ABI_SHADERS, "constant_renamed.so"), other)
    else:
        src = open("%s/constant_shader/constant_shader.cc" % REF_SHADERS).read().replace('"ConstantShader"', '"MyOwnShader"')
        (tmp_path / "other.cc").write_text(src)
        subprocess.run(["g++", "-std=c++11", "-fPIC", "-shared", "-w", "-I" + os.path.join(ROOT, "include"), "-o", other,
                        str(tmp_path / "other.cc")], check=True)
    assert L.fj_SiOpenPlugin(other.encode()) == -1
    assert "no device implementation" in host.lib().fj_scene_last_error().decode()
    # ... and one that KEEPS a known plugin_name but is not that shader (another property table): refused, not rendered as the stock one
    modified = str(tmp_path / "modified.so")
    if os.path.exists(os.path.join(ABI_SHADERS, "constant_retabled.so")):
        shutil.copy(os.path.join(ABI_SHADERS, "constant_retabled.so"), modified)
    else:
        src = open("%s/constant_shader/constant_shader.cc" % REF_SHADERS).read()
        assert '"texture"' in src and '"ConstantShader"' in src
        (tmp_path / "modified.cc").write_text(src.replace('"texture"', '"my_texture"'))
        subprocess.run(["g++", "-std=c++11", "-fPIC", "-shared", "-w", "-I" + os.path.join(ROOT, "include"), "-o", modified,
                        str(tmp_path / "modified.cc")], check=True)
    assert L.fj_SiOpenPlugin(modified.encode()) == -1
    assert "is not the shader the device code of that name implements" in host.lib().fj_scene_last_error().decode()
    # the C spelling of SiGetPropertyList: an opaque table read through accessors, the same rows as the text form
    L.fj_SiGetPropertyList.restype = C.c_void_p
    L.fj_SiGetPropertyList.argtypes = [C.c_char_p]
    for fn, rt in (("fj_property_name", C.c_char_p), ("fj_property_type_string", C.c_char_p), ("fj_property_is_valid", C.c_int), ("fj_property_default", C.c_int)):
        getattr(L, fn).restype = rt
    L.fj_property_name.argtypes = L.fj_property_type_string.argtypes = L.fj_property_is_valid.argtypes = [C.c_void_p, C.c_int]
    L.fj_property_default.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    assert L.fj_SiGetPropertyList(b"NoSuchType") is None
    tab = L.fj_SiGetPropertyList(b"Renderer")
    rows, k = [], 0
    while L.fj_property_is_valid(tab, k):
        d = (C.c_double * 4)()
        assert L.fj_property_default(tab, k, d) == 0
        rows.append("%s %s %.17g %.17g %.17g %.17g" % (L.fj_property_type_string(tab, k).decode(), L.fj_property_name(tab, k).decode(), d[0], d[1], d[2], d[3]))
        k += 1
    assert rows == table("Renderer") and len(rows) == 16 and L.fj_property_name(tab, k) is None
    L.fj_SiCloseScene()


def _write_hdr(path, img, rle):
    """Radiance RGBE writer for the test (flat or new-style RLE scanlines): img [h, w, 3] float"""
    h, w, _ = img.shape
    m = img.max(axis=2)
    e = np.where(m > 1e-32, np.floor(np.log2(np.maximum(m, 1e-38))) + 1, 0).astype(np.int64)
    scale = np.where(m > 1e-32, 256.0 / np.exp2(e.astype(np.float64)), 0.0)
    rgbe = np.zeros((h, w, 4), dtype=np.uint8)
    rgbe[..., :3] = np.clip(img * scale[..., None], 0, 255).astype(np.uint8)
    rgbe[..., 3] = np.where(m > 1e-32, e + 128, 0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
        for y in range(h):
            if not rle:
                f.write(rgbe[y].tobytes())
                continue
            f.write(bytes([2, 2, w >> 8, w & 255]))
            for c in range(4):
                row, x = rgbe[y, :, c], 0
                while x < w:
                    run = 1
                    while x + run < w and run < 127 and row[x + run] == row[x]:
                        run += 1
                    if run >= 4:
                        f.write(bytes([128 + run, int(row[x])]))
                        x += run
                    else:
                        n = 1
                        while x + n < w and n < 128 and not (x + n + 3 < w and row[x + n] == row[x + n + 1] == row[x + n + 2] == row[x + n + 3]):
                            n += 1
                        f.write(bytes([n]) + row[x:x + n].tobytes())
                        x += n


@pytest.mark.parametrize("shape,rle", [((128, 256), True), ((150, 300), True), ((64, 64), False), ((40, 100), False), ((9, 7), False)])
def test_hdr2mip_matches_the_reference_converter(shape, rle, tmp_path):
    """bin/hdr2mip (tools/hdr2mip of the reference; src/fj_mipmap.cc:246-300): RGBE decode of flat
    and run-length encoded scanlines, resampling to powers of two, tiling -- the .mip is the
    reference converter's byte for byte (its digest recorded: tests/reference_records.py), and the host's texture loader
    reads it back."""
    rng = np.random.RandomState(shape[0] * 1000 + shape[1])
    h, w = shape
    img = rng.uniform(0, 1, size=(h, w, 3)) ** 3 * rng.choice([.01, 1, 40], size=(h, w, 1))
    img[: h // 3, : w // 2] = (.25, .5, 8.0)               # long runs for the RLE coder
    img[h // 2, :] = 0
    hdr = str(tmp_path / "t.hdr")
    _write_hdr(hdr, img, rle)
    ours = str(tmp_path / "ours.mip")
    tool = os.path.join(ROOT, "fujiyama-renderer_amd", "bin", "hdr2mip")
    subprocess.run([tool, hdr, ours], check=True)
    b = open(ours, "rb").read()
    assert b[:4] == b"MIPM"
    ver, mw, mh, nc, ts = np.frombuffer(b[4:24], dtype="<i4")
    p2 = lambda v: 1 << int(np.ceil(np.log2(v)))
    assert (ver, mw, mh, nc, ts) == (1, p2(w), p2(h), 3, min(64, p2(w), p2(h))) and len(b) == 24 + mw * mh * 3 * 4
    key = "%dx%d_%s" % (h, w, "rle" if rle else "flat")
    assert reference_records.sha256(ours) == reference_records.hdr2mip_sha256(key, hdr, str(tmp_path))
    # ... and the emitter converts a .hdr texture on the way (reference fujiyama.py:222-236)
    si = fujiyama.SceneInterface(parse_args=False)
    si.NewTexture("tex1", hdr)
    line = si.text().strip()
    assert line.startswith("NewTexture tex1 ") and line.endswith(".mip") and open(line.split()[-1], "rb").read() == b


REF_BUILT = os.path.join(ROOT, "oracle", "_ref")


@pytest.mark.skipif(not os.path.exists(os.path.join(REF_BUILT, "PlasticShader.so")), reason="needs the reference build in oracle/_ref")
def test_shader_dsos_built_by_the_reference_load_unchanged(tmp_path):
    """north_star: "shader DSOs load unchanged".  The five shader DSOs of the reference BUILD
    (oracle/_ref: compiled from /root/reference against the reference's own headers, linked against
    its libscene.so) are copied next to a `libscene.so` that is libfjscene.so; SiOpenPlugin dlopens
    them, every symbol they import resolves to the product's export of the same mangled name,
    Initialize / create_instance / the property setters run, and the tables they bring are the
    built-in ones."""
    import shutil
    L = host.lib()
    L.fj_SiOpenPlugin.restype = C.c_long
    L.fj_SiOpenPlugin.argtypes = [C.c_char_p]
    L.fj_SiNewShader.restype = C.c_long
    L.fj_SiNewShader.argtypes = [C.c_long]
    L.fj_SiSetProperty3.argtypes = [C.c_long, C.c_char_p, C.c_double, C.c_double, C.c_double]
    L.fj_scene_property_table.restype = C.c_int
    L.fj_scene_property_table.argtypes = [C.c_char_p, C.c_char_p, C.c_int]

    def table(name):
        buf = C.create_string_buffer(8192)
        return None if L.fj_scene_property_table(name.encode(), buf, len(buf)) < 0 else buf.value.decode()

    names = ("PlasticShader", "GlassShader", "ConstantShader", "HairShader", "PathtracingShader")
    L.fj_SiOpenScene()
    builtin = {}
    for n in names:
        assert L.fj_SiOpenPlugin(n.encode()) >= 0
        builtin[n] = table(n)
    L.fj_SiCloseScene()
    os.symlink(os.path.join(ffi.LIB_DIR, "libfjscene.so"), str(tmp_path / "libscene.so"))   # their DT_NEEDED, RUNPATH $ORIGIN
    L.fj_SiOpenScene()
    for n in names:
        shutil.copy(os.path.join(REF_BUILT, n + ".so"), str(tmp_path))
        pid = L.fj_SiOpenPlugin(str(tmp_path / n).encode())
        assert pid >= 0, L.fj_scene_last_error()
        assert table(n) == builtin[n]
        sid = L.fj_SiNewShader(pid)
        assert sid >= 0 and L.fj_SiSetProperty3(sid, b"diffuse", .1, .2, .3) == 0
        assert L.fj_SiSetProperty3(sid, b"nonsense", 1, 2, 3) == -1
    L.fj_SiCloseScene()


def _reference_bvh_leaf_order(boxes):
    """BVHAccelerator::build over primitive boxes, restated: build_bvh sorts the range by centroid on the
    cycling axis (std::sort; stable for the few elements of a range here) and splits it where find_median says
    (src/fj_bvh_accelerator.cc:253-334); returns the leaves in depth-first (left first) order and, for every
    subtree, its (first leaf position, size)."""
    cent = [[.5 * (b[k] + b[3 + k]) for k in range(3)] for b in boxes]       # Box::Centroid, src/fj_box.cc:63-66
    order = list(range(len(boxes)))
    subtrees = []

    def find_median(begin, end, axis):
        low, high, mid = begin, end - 1, -1
        key = (cent[order[low]][axis] + cent[order[high]][axis]) / 2
        while low != mid:
            mid = (low + high) // 2
            c = cent[order[mid]][axis]
            if key < c:
                high = mid
            elif c < key:
                low = mid
            else:
                break
        return mid + 1

    def build(begin, end, axis):
        subtrees.append((begin, end - begin))
        if end - begin == 1:
            return
        order[begin:end] = sorted(order[begin:end], key=lambda i: (cent[i][axis], i))
        m = find_median(begin, end, axis)
        build(begin, m, (axis + 1) % 3)
        build(m, end, (axis + 1) % 3)

    build(0, len(boxes), 0)
    return order, subtrees


@pytest.mark.parametrize("n", [1, 3, 5, 12, 40, 150, 777])
def test_instance_level_is_the_reference_bvh_in_depth_first_order(n, asset_dir):
    """the instance level of a group (fjgpu_build.cc: BuildGroupNodes; the device builds the same list): its
    leaves are the depth-first leaf order of the reference's BVH over the instances -- restated above, independent
    of the builder --, an inner node with the union box sits in front of every subtree of more than 4 leaves,
    and its skip link points behind that subtree"""
    host.run_scene_text(workloads.crowd(asset_dir, res=(32, 24), spp=(1, 1), mesh="tiny", n=n, nlights=1), deferred=True)
    sp, _ = host.get_desc()
    best = None
    for g in range(64):                      # the group with the most instances (the crowd's trace target)
        try:
            inst, skip, box = gpu.host_instance_level(sp, g)
        except gpu.GpuError:
            break
        if best is None or (inst >= 0).sum() > (best[0] >= 0).sum():
            best = (inst, skip, box)
    inst, skip, box = best
    leaves = np.flatnonzero(inst >= 0)
    assert len(leaves) >= n
    # leaf boxes in GROUP order (the builder breaks centroid ties by position in the group): instance ids ascend with it
    by_inst = {int(inst[k]): box[k] for k in leaves}
    ids = sorted(by_inst)
    order, subtrees = _reference_bvh_leaf_order([by_inst[i] for i in ids])
    assert [int(inst[k]) for k in leaves] == [ids[j] for j in order]
    # inner nodes: exactly the subtrees of more than 4 leaves, in depth-first order, with union boxes and skip links
    want_inner = [(b, sz) for (b, sz) in subtrees if sz > 4]
    inner = np.flatnonzero(inst < 0)
    assert len(inner) == len(want_inner)
    leaf_pos = {int(k): j for j, k in enumerate(leaves)}
    for k, (b, sz) in zip(inner, want_inner):
        under = [int(x) for x in leaves if k < x < skip[k]]
        assert [leaf_pos[x] for x in under] == list(range(b, b + sz))
        lo = np.min(box[under][:, :3], axis=0)
        hi = np.max(box[under][:, 3:], axis=0)
        assert np.all(box[k][:3] <= lo) and np.all(box[k][3:] >= hi)
        assert np.all(lo - box[k][:3] <= 1e-8 * (np.abs(lo) + np.abs(hi)) + 1e-11)
        assert skip[k] == leaves[b + sz - 1] + 1          # the node after the subtree's last leaf


@pytest.mark.parametrize("bad", [
    "SetProperty1 cam1 no_such_property 1",            # unknown property name
    "SetProperty3 cam1 fov 1 2 3",                     # right name, wrong arity / type
    "SetStringProperty cam1 no_such_string x",
    "AssignCamera cam1 cam1",                          # an id of the wrong type
    "SetProperty1 nobody fov 1",                       # unknown entry name (a parser error, not an Si error)
    "NewCamera cam1 PerspectiveCamera",                # duplicate entry name
], ids=["unknown_property", "wrong_arity", "unknown_string_property", "wrong_id_type", "unknown_entry", "duplicate_entry"])
def test_failed_commands_abort_like_the_reference(bad, tmp_path):
    """error behaviour of the boundary's caller: a failing command stops the script AT THAT LINE with exit status -1, in
    the reference's `scene` (tools/scene_parser/main.cc:34-43; CommandResult::IsFail, command.cc:687-690,731-734: a command
    that creates no entry keeps the id SI_BADID, so its SI_FAIL is fatal -- a failed SetProperty* is NOT ignored) and in
    the product's bin/scene alike; the lines before it were accepted by both.  (The reference's outcome is recorded:
    tests/reference_records.py.)"""
    scn = str(tmp_path / "bad.scn")
    with open(scn, "w") as f:
        f.write("NewCamera cam1 PerspectiveCamera\nSetProperty1 cam1 fov 40\n%s\nNewFrameBuffer fb1 rgba\n" % bad)
    ref = reference_records.failing_command(bad, scn)
    ours = subprocess.run([os.path.join(ROOT, "fujiyama-renderer_amd", "bin", "scene"), scn], capture_output=True, text=True, timeout=120)
    assert ref["returncode"] != 0 and ours.returncode != 0

    def failing_line(p):
        m = re.search(r"error: .*?: (\d+): (.*)", p.stderr + p.stdout)
        return (int(m.group(1)), m.group(2).strip()) if m else None
    assert tuple(ref["failing_line"]) == failing_line(ours) == (3, bad)
    assert ours.returncode in (255, -1)                    # `return -1` of main, like the reference's
    # the accepted lines were echoed by both (`-- Name: [arg] ...`, parser.cc:274-285)
    assert any("-- SetProperty1: [cam1] [fov] [40]" in ln for ln in ref["echoed"])
    assert "-- SetProperty1: [cam1] [fov] [40]" in ours.stdout + ours.stderr
