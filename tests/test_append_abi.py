"""Growing the scene, the part that needs no GPU: the five entry points are exported by the library, prototyped by the Python host
and documented in include/gsplat_hip.h rule by rule, and the sources are wired into every build, the way tests/test_edit_abi.py
holds editing the selection to the header."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_scene_reserve", "gsr_scene_capacity", "gsr_scene_duplicate_selected", "gsr_scene_append_selected", "gsr_scene_append_arrays")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, u32, u32p = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
    assert lib.gsr_scene_reserve.argtypes == [vp, u32]
    assert lib.gsr_scene_capacity.argtypes == [vp, u32p]
    assert lib.gsr_scene_duplicate_selected.argtypes == [vp, u32p, u32p]
    assert lib.gsr_scene_append_selected.argtypes == [vp, vp, u32p, u32p]
    assert lib.gsr_scene_append_arrays.argtypes == [vp, vp, vp, vp, vp, u32, u32p]
    # a NULL context is refused by every one of them, with nothing touched
    a, b = u32(7), u32(9)
    for call in (lambda: lib.gsr_scene_reserve(None, 10), lambda: lib.gsr_scene_capacity(None, ctypes.byref(a)),
                 lambda: lib.gsr_scene_duplicate_selected(None, ctypes.byref(a), ctypes.byref(b)),
                 lambda: lib.gsr_scene_append_selected(None, None, ctypes.byref(a), ctypes.byref(b)),
                 lambda: lib.gsr_scene_append_arrays(None, None, None, None, None, 0, ctypes.byref(a))):
        assert call() == -1
    assert (a.value, b.value) == (7, 9)


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("int gsr_scene_reserve(gsr_ctx *ctx, uint32_t rows);",
                 "int gsr_scene_capacity(gsr_ctx *ctx, uint32_t *rows);",
                 "int gsr_scene_duplicate_selected(gsr_ctx *ctx, uint32_t *first, uint32_t *count);",
                 "int gsr_scene_append_selected(gsr_ctx *ctx, gsr_ctx *from, uint32_t *first, uint32_t *count);",
                 "int gsr_scene_append_arrays(gsr_ctx *ctx, const uint32_t *data, const float *positions, const float *rotations, "
                 "const float *scales, uint32_t m, uint32_t *first);"):
        assert decl in flat, decl
    assert src.index("/* ---- editing the selection ----") < src.index("/* ---- growing the scene ----") < src.index("/* ---- contribution ----")
    m = re.search(r"/\* ---- growing the scene ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on growing the scene"
    doc = " ".join(m.group(0).replace(" * ", " ").split())
    # duplicate; append selected; append arrays; state afterwards; capacity; ordering; refusals
    for words in ("the selected indices in ascending order", "n + k splats", "Rows [0, n) are not written at all", "Row n + j holds the bits of row idx[j]",
                  "bit for bit, NaNs and -0.0 included", "no arithmetic and no re-packing of the covariance", "*first = n, *count = k",
                  "nothing is read back to learn it", "With k == 0 the call returns GSR_OK with count 0, touches nothing and is not an edit",
                  "the last frame stays valid",
                  "duplicate with the rows read from `from`'s scene and `from`'s selection", "must be on the same device",
                  "from == ctx, or a member of the same shared scene, is exactly duplicate", "`from`'s scene, selection and frame state are not changed",
                  "waited for on the device, not on the host", "`from`'s SH rows are not carried", "the copies keep their rgba word",
                  "the same repack and check as gsr_set_scene_arrays", "no new arithmetic", "GSR_ERR_SCENE: positions differ from data words 0..2",
                  "leaves everything as it was, the count and the capacity included", "A scene with no splats and no rotations / scales accepts the call",
                  "the selection becomes exactly the new rows [first, first + count)", "a REPLACE", "gsr_scene_translate_selected moves the copies",
                  "its version moves", "the bits are set on the device, no upload proportional to n is made", "The hidden set keeps its bits",
                  "new rows are visible, and so is the copy of a hidden selected splat", "keep the old rows' values and `frames`", "new rows start at zero",
                  "they stay \"never reset\"", "Indices of existing splats do not move", "The context stays in its shared scene",
                  "If n + k <= capacity nothing of the scene arrays is re-allocated and no old row is copied",
                  "max(n + k, capacity + capacity / 2)", "0x7fffffff / 8", "the old rows are carried by device copies",
                  "The selection, hidden and contribution buffers grow with the capacity where they exist",
                  "gsr_scene_reserve performs the growth alone", "it never shrinks, no splat changes", "scene_bytes reports the capacity",
                  "gsr_scene_limit_box and gsr_scene_erase_selected keep their behaviour",
                  "blocking scene replacements like gsr_scene_limit_box", "the other members' streams are waited for",
                  "every member re-sizes its per-splat buffers before its next frame", "every member's frame and sorted order as edited",
                  "gsr_select_region, gsr_pick, gsr_depth_async, gsr_contrib_accumulate_async and gsr_overlay_async return GSR_ERR_ARG until the next frame",
                  "a NULL ctx", "a NULL `from`", "a NULL data / positions / rotations / scales with m > 0", "a destination without rotations / scales",
                  "a `from` on another device", "n + k above the upload's limit", "a destination that has SH rows (sh_count != 0)",
                  "SH rows are indexed by splat order and the bands are index thresholds", "would fall into the top band and has no SH row to read"):
        assert words in doc, words


def test_python_host_has_the_methods():
    import gsplat_hip as gh
    sig = lambda name: inspect.signature(getattr(gh.HIPRenderer, name)).parameters
    assert list(sig("scene_reserve")) == ["self", "rows"]
    assert list(sig("scene_capacity")) == ["self"]
    assert list(sig("scene_duplicate_selected")) == ["self"]
    assert list(sig("scene_append_selected")) == ["self", "other"]
    assert list(sig("scene_append_arrays")) == ["self", "data", "positions", "rotations", "scales"]


class _Lib:
    """records the calls the Python host makes and answers like a scene of 100 splats with 7 selected"""

    def __init__(self):
        self.calls = []

    def gsr_scene_reserve(self, ctx, rows):
        self.calls.append(("reserve", rows))
        return 0

    def gsr_scene_capacity(self, ctx, rows):
        rows._obj.value = 150
        return 0

    def gsr_scene_duplicate_selected(self, ctx, first, count):
        self.calls.append(("duplicate",))
        first._obj.value, count._obj.value = 100, 7
        return 0

    def gsr_scene_append_selected(self, ctx, other, first, count):
        self.calls.append(("append_selected", other))
        first._obj.value, count._obj.value = 107, 3
        return 0

    def gsr_scene_append_arrays(self, ctx, data, pos, rot, scl, m, first):
        self.calls.append(("append_arrays", m))
        first._obj.value = 110
        return 0


def test_python_host_returns_first_and_count_and_follows_the_count():
    import numpy as np
    import gsplat_hip as gh
    r, other = object.__new__(gh.HIPRenderer), object.__new__(gh.HIPRenderer)
    r._L, r._ctx, r._check, r._n, r._scene, r._shared = _Lib(), None, lambda rc: None, 100, None, False
    other._ctx = 1234
    r.scene_reserve(150)
    assert r.scene_capacity() == 150
    assert r.scene_duplicate_selected() == (100, 7) and r._n == 107
    assert r.scene_append_selected(other) == (107, 3) and r._n == 110
    assert r.scene_append_arrays(np.zeros(16, np.uint32), np.zeros(6, np.float32), np.zeros(8, np.float32), np.zeros(6, np.float32)) == 110 and r._n == 112
    assert r._L.calls == [("reserve", 150), ("duplicate",), ("append_selected", 1234), ("append_arrays", 2)]
    import pytest
    with pytest.raises(ValueError):
        r.scene_append_arrays(np.zeros(16, np.uint32), np.zeros(6, np.float32), np.zeros(4, np.float32), np.zeros(6, np.float32))


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    for f in ("gsr_append.cpp", "k_append.hip"):
        assert f in srcs and os.path.exists(os.path.join(CSRC, f)), f   # SRCS feeds the objects, the build id and the bounds build
    build_id = re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "$(SRCS)" in build_id
    host = open(os.path.join(CSRC, "gsr_append.cpp")).read()
    for word in ("sync_members(c)", "adopt_scene(c)", "++sc.generation", "invalidate_members(c, true)", "overlay_before_selection_change(c)", "require_rows(c)",
                 "launch_append_gather(", "launch_append_select_range(", "upload_rows(c, who, v, n, m,", "sc.sh_count", "hipStreamWaitEvent(c->stream"):
        assert word in host, word
    # the repack and its check are the upload's own (one hop further: the helper gsr_set_scene_arrays goes through)
    scene = open(os.path.join(CSRC, "gsr_scene.cpp")).read()
    helper = re.search(r"^int gsr::upload_rows\(.*?^}", scene, flags=re.S | re.M)
    assert helper, "gsr_scene.cpp does not define upload_rows"
    for word in ("launch_repack_scene(", "launch_scene_import("):
        assert word in helper.group(0), word
    assert scene.count("upload_rows(") == 2 and "launch_repack_scene(" not in scene.replace(helper.group(0), "")   # defined once, called by the upload
    internal = open(os.path.join(CSRC, "gsr_internal.h")).read()
    for word in ("void launch_append_gather(", "void launch_append_select_range(", "uint32_t append_blocks("):
        assert word in internal, word
    kern = open(os.path.join(CSRC, "k_append.hip")).read()
    for word in ("GSR_BOUNDS_DECL(append)", "GSR_BOUND(append, 0,", "GSR_BOUND(append, 1,", "GSR_BOUND(append, 2, row, dst_rows)", "GSR_BOUND(append, 3,",
                 "k_append_count", "k_append_scan", "k_append_gather", "k_append_select_range", "__popc(", "__shfl("):
        assert word in kern, word
    assert "pack_cov" not in kern and "__ballot" not in kern   # bits travel as they are; the selection words are the ballot already


def test_existing_kernels_are_untouched():
    """k_scene.hip's compaction templates are not what grows the scene: nothing of k_append is named there."""
    assert "append" not in open(os.path.join(CSRC, "k_scene.hip")).read()
