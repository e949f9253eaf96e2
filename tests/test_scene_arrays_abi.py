"""gsr_set_scene_arrays on a box without a GPU: declared in the header, exported by the library, mirrored by the hosts, and it
refuses what it can refuse without a device; the two kernels behind it and behind gsr_read_scene are in the gfx950 code object."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSR_ERR_ARG = -1


def test_header_declares_it_and_the_library_exports_it():
    import gsplat_hip as gh
    src = open(os.path.join(ROOT, "include", "gsplat_hip.h")).read()
    assert re.search(r"int gsr_set_scene_arrays\(gsr_ctx \*ctx, const uint32_t \*data, const float \*positions, const float \*rotations,\s*"
                     r"const float \*scales,\s*uint32_t n\);", src)
    assert "gsr_set_scene_arrays" in gh.EXPORTS
    L = gh.load_library()
    assert L.gsr_set_scene_arrays.argtypes is not None and len(L.gsr_set_scene_arrays.argtypes) == 6
    assert "set_scene_arrays" in gh.HIPRenderer.__dict__


def test_it_refuses_a_null_context():
    import gsplat_hip as gh
    L = gh.load_library()
    buf = (ctypes.c_uint32 * 8)()
    p = ctypes.addressof(buf)
    assert L.gsr_set_scene_arrays(None, p, p, p, p, 1) == GSR_ERR_ARG
    assert L.gsr_set_scene_arrays(None, None, None, None, None, 0) == GSR_ERR_ARG


def test_null_arrays_and_too_many_splats_are_refused_in_front_of_any_device_call():
    """The argument checks stand in front of the first HIP call (a live context is refused the same way on the GPU:
    tests/test_gpu_scene_binding.py)."""
    src = open(os.path.join(ROOT, "gsplat.js_amd", "csrc", "gsr_scene.cpp")).read()
    body = src[src.index("int gsr_set_scene_arrays("):]
    body = body[:body.index("\n}\n")]
    assert "!data || !positions || !rotations || !scales" in body and "GSR_ERR_ARG" in body and "hip" not in body
    helper = src[src.index("int upload_scene("):]
    assert helper.index("too many splats") < helper.index("hipSetDevice")


def test_the_node_addon_binds_it():
    src = open(os.path.join(ROOT, "gsplat.js_amd", "js", "native", "addon.cc")).read()
    assert '{"setSceneArrays", SetSceneArrays}' in src and '{"readSceneArrays", ReadSceneArrays}' in src
    assert "gsr_set_scene_arrays(" in src


def test_cpp_caller_has_the_two_scene_legs():
    exe = os.path.join(ROOT, "gsplat.js_amd", "lib", "bench_cabi")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert "--scene-arrays" in r.stdout + r.stderr and "--scene-edit" in r.stdout + r.stderr


def test_library_holds_the_two_kernels():
    import gsplat_hip as gh
    out = subprocess.run(["strings", "-a", gh.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out and "k_scene_import" in out and "k_scene_export" in out


def test_bounds_twin_counts_the_scene_kernels():
    lib = os.path.join(ROOT, "gsplat.js_amd", "lib_exp", "bounds", "libgsplat_hip.so")
    out = subprocess.run(["nm", "-D", lib], capture_output=True, text=True).stdout
    assert "gsr_debug_bounds_scene" in out
    shipped = subprocess.run(["nm", "-D", os.path.join(ROOT, "gsplat.js_amd", "lib", "libgsplat_hip.so")], capture_output=True, text=True).stdout
    assert "gsr_set_scene_arrays" in shipped and "gsr_debug_bounds_scene" not in shipped
