"""Hidden splats, the part that needs no GPU: the four entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h rule by rule, the way tests/test_select_abi.py holds the selection to the header."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_hide_selected", "gsr_hidden_set", "gsr_read_hidden", "gsr_select_hidden")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u32p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
    assert lib.gsr_hide_selected.argtypes == [vp, i32, u32p]
    assert lib.gsr_hidden_set.argtypes == [vp, vp, u32, i32, u32p]
    assert lib.gsr_read_hidden.argtypes == [vp, vp, u32, u32p]
    assert lib.gsr_select_hidden.argtypes == [vp, i32, u32p]
    # a NULL context is refused by every one of them, with nothing touched
    for call in (lambda: lib.gsr_hide_selected(None, 1, None), lambda: lib.gsr_hidden_set(None, None, 0, 0, None),
                 lambda: lib.gsr_read_hidden(None, None, 0, None), lambda: lib.gsr_select_hidden(None, 0, None)):
        assert call() == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("int gsr_hide_selected(gsr_ctx *ctx, int32_t op, uint32_t *hidden);",
                 "int gsr_hidden_set(gsr_ctx *ctx, const uint32_t *words, uint32_t nwords, int32_t op, uint32_t *hidden);",
                 "int gsr_read_hidden(gsr_ctx *ctx, uint32_t *words, uint32_t nwords, uint32_t *hidden);",
                 "int gsr_select_hidden(gsr_ctx *ctx, int32_t op, uint32_t *selected);"):
        assert decl in flat, decl
    assert src.index("/* ---- selection ----") < src.index("/* ---- hidden splats ----") < src.index("/* ---- contribution ----")   # behind the selection's
    m = re.search(r"/\* ---- hidden splats ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on hidden splats"
    doc = " ".join(m.group(0).replace(" * ", " ").split())
    # no reference interface; the layout; nothing allocated; one set; the frame; sorted all the same; downstream; the empty set; the calls;
    # the edit and its order; compaction; where it is replaced; interplay
    for words in ("No interface of the reference", "limitBox and nothing softer", "src/core/Scene.ts:307-366", "non-destructive",
                  "bit i & 31 of word i >> 5", "bits at and above n are always 0", "reads as all zeros", "allocated nothing", "scene_bytes is unchanged",
                  "ONE hidden set", "fails the frame's culls, as if its pixel box were empty", "no record and no bin rectangle", "in no bin list",
                  "gsr_timings.visible / bin_entries / tile_entries", "optical-mass words", "not a survivor", "(x0 > x1)", "still sorted",
                  "gsr_read_depth_index", "gsr_sort does not look at H", "follows from the lists", "see through it", "no weight", "does not draw it",
                  "a null pointer, not an all-zero mask", "show all", "H = H op S", "H = H & ~S (show)", "H = H | S (hide)", "(NULL, 0, GSR_SELOP_REPLACE)",
                  "words may be NULL: count only", "S = S op H", "an ordinary picker", "does not touch H or any frame", "may be NULL",
                  "nwords >= ceil(n / 32)", "host bits at or above n are dropped", "changes nothing", "ordered like gsr_scene_translate",
                  "a scene from gsr_set_scene can hide", "every member's frame state as edited", "GSR_ERR_ARG until the next frame",
                  "before the call see the old H", "see the new one", "no host wait on other members' streams", "waits for its own stream",
                  "would change no bit still counts as an edit", "re-captured", "H'[new index of i] = H[i]", "the tail is 0 and the count is recomputed",
                  "still dropped", "gsr_select_hidden(REPLACE) + gsr_scene_erase_selected(0)", "afterwards H is empty",
                  "gsr_set_scene* leaves nothing hidden", "ctx has `from`'s H", "starts with nothing hidden", "hidden ones included",
                  "so `below` picks it", "gsr_select_hidden(SUBTRACT)"):
        assert words in doc, words


def test_python_host_has_the_methods():
    import gsplat_hip as gh
    import inspect
    for name in ("hide_selected", "set_hidden", "hidden", "hidden_words", "hidden_count", "select_hidden"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    sig = lambda name: inspect.signature(getattr(gh.HIPRenderer, name)).parameters
    assert sig("hide_selected")["op"].default == "add"
    assert sig("set_hidden")["op"].default == "replace" and list(sig("set_hidden"))[1] == "hidden" and sig("set_hidden")["hidden"].default is None
    assert sig("select_hidden")["op"].default == "replace"


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "gsr_hidden.cpp" in srcs and os.path.exists(os.path.join(CSRC, "gsr_hidden.cpp"))   # SRCS feeds the objects, the build id and the bounds build
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    scene = open(os.path.join(CSRC, "k_scene.hip")).read()
    assert "k_box_compact_bits" in scene and re.search(r"GSR_BOUND\(scene, 6,", scene) and re.search(r"GSR_BOUND\(scene, 7,", scene)
    assert scene.index("GSR_BOUNDS_DECL(scene)") < scene.index("void k_box_compact_bits")
    proj = open(os.path.join(CSRC, "k_project.hip")).read()
    assert "if (sc.hidden)" in proj
    internal = open(os.path.join(CSRC, "gsr_internal.h")).read()
    assert "const uint32_t* hidden;" in internal
    # the edit's order is the scene edits': the three helpers are shared, not copied
    ctx = open(os.path.join(CSRC, "gsr_ctx.h")).read()
    for decl in ("int edit_begin(gsr_ctx* c);", "int edit_end(gsr_ctx* c);", "void invalidate_members(gsr_ctx* c, bool lists);"):
        assert decl in ctx, decl
    hid = open(os.path.join(CSRC, "gsr_hidden.cpp")).read()
    for word in ("edit_begin(c)", "edit_end(c)", "invalidate_members(c", "launch_select_apply(", "select_fold_and_count("):
        assert word in hid, word
