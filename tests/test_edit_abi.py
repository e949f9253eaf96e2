"""Editing the selection, the part that needs no GPU: the five entry points are exported by the library, prototyped by the Python
host and documented in include/gsplat_hip.h rule by rule, the way tests/test_hide_abi.py holds the hidden set to the header."""
import ctypes
import glob
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
NAMES = ("gsr_selection_bounds", "gsr_scene_translate_selected", "gsr_scene_rotate_selected", "gsr_scene_scale_selected",
         "gsr_scene_set_rgba_selected")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    assert lib.gsr_selection_bounds.argtypes == [vp, ctypes.POINTER(gh.GsrSelectionBounds)]
    assert ctypes.sizeof(gh.GsrSelectionBounds) == 28
    assert lib.gsr_scene_translate_selected.argtypes == [vp, vp]
    assert lib.gsr_scene_rotate_selected.argtypes == [vp, vp, vp]
    assert lib.gsr_scene_scale_selected.argtypes == [vp, vp, vp]
    assert lib.gsr_scene_set_rgba_selected.argtypes == [vp, u32, u32]
    # a NULL context is refused by every one of them, with nothing touched
    v = (ctypes.c_double * 4)(0, 0, 0, 1)
    b = gh.GsrSelectionBounds()
    for call in (lambda: lib.gsr_selection_bounds(None, ctypes.byref(b)), lambda: lib.gsr_scene_translate_selected(None, ctypes.addressof(v)),
                 lambda: lib.gsr_scene_rotate_selected(None, ctypes.addressof(v), None), lambda: lib.gsr_scene_scale_selected(None, ctypes.addressof(v), None),
                 lambda: lib.gsr_scene_set_rgba_selected(None, 0, 0)):
        assert call() == -1


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("struct gsr_selection_bounds { uint32_t count; float min[3]; float max[3]; };",
                 "int gsr_selection_bounds(gsr_ctx *ctx, struct gsr_selection_bounds *out);",
                 "int gsr_scene_translate_selected(gsr_ctx *ctx, const double *t );",
                 "int gsr_scene_rotate_selected(gsr_ctx *ctx, const double *q , const double *pivot );",
                 "int gsr_scene_scale_selected(gsr_ctx *ctx, const double *s , const double *pivot );",
                 "int gsr_scene_set_rgba_selected(gsr_ctx *ctx, uint32_t rgba, uint32_t byte_mask);"):
        assert decl in flat, decl
    assert src.index("/* ---- hidden splats ----") < src.index("/* ---- editing the selection ----") < src.index("/* ---- contribution ----")
    m = re.search(r"/\* ---- editing the selection ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on editing the selection"
    doc = " ".join(m.group(0).replace(" * ", " ").split())
    # transforms; pivot; recolour; bounds; ordering; what survives; requirements and refusals
    for words in ("src/core/Scene.ts:182-305", "a Scene that held only the selected splats", "f64 arithmetic in the reference's order",
                  "wherever the reference stores into a Float32Array", "Every other splat is not written at all",
                  "equals gsr_scene_translate / _rotate / _scale bit for bit", "translate(-pivot), the operation, translate(+pivot)",
                  "each step rounding to f32", "one read and one write per selected splat", "pivot == NULL means the operation alone",
                  "not the same as a pivot of zero", "turns -0.0 into +0.0",
                  "rgba[i] = (rgba[i] & ~byte_mask) | (rgba & byte_mask)", "data[8i+7]", "opacity in the top byte",
                  "(index > bandsIndices[0]) the projection reads only the opacity byte",
                  "axis-aligned box of their centres as f32", "enters min only through x < min", "max only through x > max",
                  "a NaN coordinate is counted but never enters the box", "count is 0, min is +inf and max is -inf",
                  "hidden splats that are selected count like any other", "order-free, so it is exact", "28 bytes are copied back", "no host loop over n",
                  "ordered like gsr_scene_translate", "no host wait on other members' streams", "read the old scene", "read the new scene",
                  "every member's frame and sorted order as edited", "gsr_select_region, gsr_pick, gsr_depth_async, gsr_contrib_accumulate_async and gsr_overlay_async",
                  "GSR_ERR_ARG until the next frame", "would change no bit still counts as an edit", "no kernel is launched",
                  "the selection, the hidden set and the contribution accumulators are untouched", "indices do not move",
                  "the accumulators then describe the old geometry", "require a scene with rotations / scales",
                  "refused while gsr_set_sh_follow is on and the scene has SH rows", "the SH frame is one per scene and a partial rotation has none",
                  "translate and set_rgba are allowed in that state", "Each scale component must be finite", "zero is allowed",
                  "A NULL ctx or a NULL required pointer returns GSR_ERR_ARG with nothing touched"):
        assert words in doc, words


def test_python_host_has_the_methods():
    import gsplat_hip as gh
    for name in ("selection_bounds", "scene_translate_selected", "scene_rotate_selected", "scene_scale_selected", "scene_set_rgba_selected"):
        assert callable(getattr(gh.HIPRenderer, name)), name
    sig = lambda name: inspect.signature(getattr(gh.HIPRenderer, name)).parameters
    assert list(sig("selection_bounds")) == ["self"]
    assert list(sig("scene_translate_selected")) == ["self", "t"]
    assert list(sig("scene_rotate_selected")) == ["self", "q_xyzw", "pivot"] and sig("scene_rotate_selected")["pivot"].default is None
    assert list(sig("scene_scale_selected")) == ["self", "s", "pivot"] and sig("scene_scale_selected")["pivot"].default is None
    assert list(sig("scene_set_rgba_selected")) == ["self", "rgba", "channels"] and sig("scene_set_rgba_selected")["channels"].default == "rgba"


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    for f in ("gsr_edit.cpp", "k_edit.hip"):
        assert f in srcs and os.path.exists(os.path.join(CSRC, f)), f   # SRCS feeds the objects, the build id and the bounds build
    build_id = re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert "$(SRCS)" in build_id and "k_pack_cov.h" in build_id
    assert re.search(r"^\$\(OUT\)/%\.o: %\.hip .*k_pack_cov\.h", mk, flags=re.M), "the .hip rule does not depend on the shared header"
    edit = open(os.path.join(CSRC, "gsr_edit.cpp")).read()
    for word in ("edit_begin(c)", "edit_end(c)", "invalidate_members(c", "launch_edit_translate(", "launch_edit_rotate(", "launch_edit_scale(",
                 "launch_edit_rgba(", "launch_edit_bounds("):
        assert word in edit, word
    kern = open(os.path.join(CSRC, "k_edit.hip")).read()
    for word in ("GSR_BOUNDS_DECL(edit)", "GSR_BOUND(edit, 0,", "GSR_BOUND(edit, 1,", "GSR_BOUND(edit, 2,", "k_edit_translate", "k_edit_rotate", "k_edit_scale",
                 "k_edit_rgba", "k_edit_bounds", "template <bool PIVOT>", "__popc(", "__shfl_xor(", '#include "k_pack_cov.h"'):
        assert word in kern, word


def test_the_covariance_arithmetic_exists_once():
    defs = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path):
            text = open(path, errors="replace").read()
            for fn in ("pack_cov", "pack_half2", "float_to_half_trunc"):
                if re.search(r"__device__[^;{]*\b%s\(" % fn, text):
                    defs.setdefault(fn, []).append(os.path.basename(path))
    assert defs == {"pack_cov": ["k_pack_cov.h"], "pack_half2": ["k_pack_cov.h"], "float_to_half_trunc": ["k_pack_cov.h"]}, defs
    assert '#include "k_pack_cov.h"' in open(os.path.join(CSRC, "k_scene.hip")).read()


def _csrc_files_with(pattern):
    """the files of csrc/ whose text matches `pattern`, comments included"""
    return [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*")))
            if os.path.isfile(p) and re.search(pattern, open(p, errors="replace").read())]


def test_the_transform_arithmetic_exists_once():
    """Scene.rotate's matrix and quaternion product are written in one file (pack_cov's own matrix is of another quaternion and
    names its entries qx..qw), and the three units that need them include it."""
    assert _csrc_files_with(re.escape("1 - 2 * y * y - 2 * z * z")) == ["k_splat_ops.h"]
    assert _csrc_files_with(re.escape("w1 * x2 + x1 * w2")) == ["k_splat_ops.h"]
    for f in ("k_scene.hip", "k_edit.hip", "gsr_scene.cpp"):
        assert '#include "k_splat_ops.h"' in open(os.path.join(CSRC, f)).read(), f
    for fn in ("quat_matrix", "splat_translate", "splat_rotate", "splat_scale", "copy_splat_row", "set_live_bits", "set_word", "set_bit"):
        assert _csrc_files_with(r"__device__[^;{]*\b%s\(" % fn) == ["k_splat_ops.h"], fn
    # the tail mask of a set's last word and the bit test are spelled out nowhere else
    assert _csrc_files_with(re.escape("(1u << rest) - 1u")) == ["k_splat_ops.h"]
    # (the frame path's two readers, k_project.hip and k_overlay.hip, are not the editing layer's)
    assert _csrc_files_with(r">> \(i & 31u\)\) & 1u") == ["k_overlay.hip", "k_project.hip", "k_splat_ops.h"]
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_splat_ops.h" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert re.search(r"^\$\(OUT\)/%\.o: %\.hip .*k_splat_ops\.h", mk, flags=re.M), "the .hip rule does not depend on the shared header"
    assert re.search(r"^\$\(OUT\)/gsr_%\.o: gsr_%\.cpp .*k_splat_ops\.h", mk, flags=re.M), "the host rule does not depend on the shared header"


def test_the_analysis_helpers_exist_once():
    """The scope of an analysis call, a picker's mask store, the workgroup reductions, the near walk and the host's scope are each
    defined in one file of csrc/, the copies they replaced are defined nowhere, and a unit names its bounds sites through a struct
    of its own instead of a define in front of an include."""
    for fn in ("scope_word", "in_scope", "mask_store_ballot", "lds_counters_zero", "lds_counters_flush", "workgroup_sum_u64", "f32_finite", "f64_nan", "f64_inf"):
        assert _csrc_files_with(r"__device__[^;{]*\b%s\(" % fn) == ["k_splat_ops.h"], fn
    assert _csrc_files_with(r"\buint32_t mask_blocks\(uint32_t nwords, uint32_t threads\)\s*\{") == ["k_splat_ops.h"]
    assert _csrc_files_with(r"__device__[^;{]*\bnb_each_near\(") == ["k_neighbours.h"]
    assert _csrc_files_with(r"(?m)^int gsr::scope_check\(") == ["gsr_attr.cpp"]
    assert _csrc_files_with(r"\bAttrScope scene_scope\([^;{)]*\)\s*\{") == ["gsr_ctx.h"]
    for old in ("attr_scope_word", "nb_scope_word", "knn_scope_word", "cl_scope_word", "mg_scope_word", "nb_in_scope", "knn_in_scope", "attr_in_scope",
                "cl_store_ballot", "mg_store_ballot", "cl_each_near", "nb_finite", "mg_finite", "knn_nan", "knn_inf", "attr_nan", "cl_mask_blocks"):
        assert _csrc_files_with(r"\b%s\b" % old) == [], old
    # the store of a ballot's two words, the scope's flag test and the scope's assembly on the host are spelled out once each
    assert _csrc_files_with(re.escape("[w + 1u] = (uint32_t)(m >> 32)")) == ["k_splat_ops.h"]
    assert _csrc_files_with(re.escape("sc.flags & ATTR_SCOPE_SELECTED")) == ["k_splat_ops.h"]
    assert _csrc_files_with(re.escape("* 32u + ")) == ["k_splat_ops.h"]                          # "one lane per bit of the mask"
    assert _csrc_files_with(re.escape("sel.mask, sc.sel.words, sc.hid.mask, sc.hid.words}")) == ["gsr_ctx.h"]
    assert _csrc_files_with(re.escape("unknown scope flags")) == ["gsr_attr.cpp"]
    # every picker stores its mask through the one helper, launched with the one grid
    for f, stores in (("k_attr.hip", 1), ("k_neighbours.hip", 1), ("k_knn.hip", 1), ("k_clusters.hip", 2), ("k_merge.hip", 3), ("k_contrib.hip", 1), ("k_select.hip", 1)):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "k_splat_ops.h"' in text, f
        assert len(re.findall(r"\bmask_store_ballot<\w+>\(", text)) == stores, f
        assert text.count("dim3(mask_blocks(") == (2 if f in ("k_clusters.hip", "k_merge.hip") else 1), f
    for f in ("k_attr.hip", "k_neighbours.hip", "k_knn.hip", "k_merge.hip"):                     # the four LDS histograms
        text = open(os.path.join(CSRC, f)).read()
        assert "lds_counters_zero(s_hist, " in text and re.search(r"lds_counters_flush<\w+_sites>\(s_hist, ", text), f
    # no site is named by a define in front of an include: k_neighbours.h is an ordinary header
    assert _csrc_files_with(r"NB_BOUND_BUCKET") == []
    assert "#error" not in open(os.path.join(CSRC, "k_neighbours.h")).read()
    for f in ("k_neighbours.hip", "k_knn.hip", "k_clusters.hip", "k_merge.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert text.index('#include "k_neighbours.h"') < text.index("GSR_BOUNDS_DECL("), f


def test_the_splat_set_is_sized_and_allocated_once():
    """the sizes of a one-bit-per-splat set are defined in one file, and neither set allocates for itself"""
    for fn in ("words_of", "fold_words", "counter_words", "op_ok"):
        assert _csrc_files_with(r"\b(uint32_t|bool) %s\([^;{)]*\)\s*\{" % fn) == ["gsr_ctx.h"], fn
    for path, fn in (("gsr_select.cpp", "select_ensure"), ("gsr_hidden.cpp", "hidden_ensure")):
        body = re.search(r"^int gsr::%s\(gsr_ctx\* c\)\s*\{.*?\}\s*$" % fn, open(os.path.join(CSRC, path)).read(), flags=re.S | re.M)
        assert body and "set_ensure(" in body.group(0) and ".alloc(" not in body.group(0), fn
    assert _csrc_files_with(r"(?m)^int gsr::set_ensure\(") == ["gsr_select.cpp"]
    append = open(os.path.join(CSRC, "gsr_append.cpp")).read()
    assert "set_ensure(c, sel, nullptr, sc.arr_rows" in append and "sel.mask.alloc(" not in append   # an append sizes for the capacity
