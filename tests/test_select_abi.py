"""Selection, the part that needs no GPU: the six entry points are exported by the library, prototyped by the Python host and
documented in include/gsplat_hip.h, the way tests/test_share_abi.py holds shared scenes to the header."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsplat_hip.h")
NAMES = ("gsr_select_region", "gsr_select_box", "gsr_selection_set", "gsr_selection_invert", "gsr_read_selection", "gsr_scene_erase_selected")


def test_symbols_are_exported_and_prototyped():
    import gsplat_hip as gh
    lib = gh.load_library()
    for n in NAMES:
        assert hasattr(lib, n), "libgsplat_hip.so does not export %s" % n
        assert n in gh.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    vp, i32, u32, u32p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
    assert lib.gsr_select_region.argtypes == [vp, ctypes.POINTER(gh.GsrRegion), i32, i32, u32p]
    assert lib.gsr_select_box.argtypes == [vp, vp, i32, u32p]
    assert lib.gsr_selection_set.argtypes == [vp, vp, u32, i32, u32p]
    assert lib.gsr_selection_invert.argtypes == [vp, u32p]
    assert lib.gsr_read_selection.argtypes == [vp, vp, u32, u32p]
    assert lib.gsr_scene_erase_selected.argtypes == [vp, i32, u32p]
    # gsr_region: four int32, a pointer, two int32
    assert [f[0] for f in gh.GsrRegion._fields_] == ["x0", "y0", "x1", "y1", "mask", "mask_stride", "reserved"]
    assert ctypes.sizeof(gh.GsrRegion) == 32 and gh.GsrRegion.mask.offset == 16 and gh.GsrRegion.mask_stride.offset == 24
    assert gh.SELECT_MODES == {"centre": 0, "hit": 1} and gh.SELECT_OPS == {"replace": 0, "add": 1, "subtract": 2, "intersect": 3}


def test_header_declares_and_documents_them():
    src = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    flat = " ".join(code.split())
    for decl in ("#define GSR_SELECT_CENTRE 0", "#define GSR_SELECT_HIT 1", "#define GSR_SELOP_REPLACE 0", "#define GSR_SELOP_ADD 1",
                 "#define GSR_SELOP_SUBTRACT 2", "#define GSR_SELOP_INTERSECT 3",
                 "typedef struct gsr_region { int32_t x0, y0, x1, y1; const uint8_t *mask; int32_t mask_stride; int32_t reserved; } gsr_region;",
                 "int gsr_select_region(gsr_ctx *ctx, const gsr_region *region, int32_t mode, int32_t op, uint32_t *selected);",
                 "int gsr_select_box(gsr_ctx *ctx, const double *box , int32_t op, uint32_t *selected);",
                 "int gsr_selection_set(gsr_ctx *ctx, const uint32_t *words, uint32_t nwords, int32_t op, uint32_t *selected);",
                 "int gsr_selection_invert(gsr_ctx *ctx, uint32_t *selected);",
                 "int gsr_read_selection(gsr_ctx *ctx, uint32_t *words, uint32_t nwords, uint32_t *selected);",
                 "int gsr_scene_erase_selected(gsr_ctx *ctx, int32_t keep_selected, uint32_t *new_count);"):
        assert decl in flat, decl
    m = re.search(r"/\* ---- selection ----.*?\*/", src, flags=re.S)
    assert m, "the header has no section on selection"
    doc = " ".join(m.group(0).replace(" * ", " ").split())
    # the layout, the two modes, the region, the box, the ops, blocking, the frame, the errors, erase and its exception, where it is cleared
    for words in ("bit i & 31 of word i >> 5", "bits at and above n are always 0", "reads as all zeros", "ONE selection", "select through",
                  "(int)floorf(cx)", "outside the image never selects", "select the surface", "hit_alpha of that moment", "mask_stride >= x1 - x0",
                  "inside the band", "needs no frame", "min >= max", "S = S & ~P", "may be NULL", "blocking", "no events between them",
                  "settles the frame as gsr_pick does", "GSR_ERR_OVERFLOW", "reserved != 0", "sort-only", "nwords >= ceil(n / 32)",
                  "keeps the tail at 0", "order-preserving", "gsr_set_sh_follow", "nothing would be removed", "gsr_pick still answers",
                  "the selection is empty", "does not survive a limitBox", "translate, rotate and scale keep it", "starts empty", "scene_bytes",
                  "allocates nothing"):
        assert words in doc, words


def test_python_host_has_the_methods():
    import gsplat_hip as gh
    for name in ("select_region", "select_box", "set_selection", "invert_selection", "selection", "selection_words", "scene_erase_selected"):
        assert callable(getattr(gh.HIPRenderer, name)), name


def test_sources_are_wired_into_every_build():
    mk = open(os.path.join(ROOT, "gsplat.js_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "k_select.hip" in srcs and "gsr_select.cpp" in srcs          # SRCS feeds the objects, the build id and (scripts/build_exp.sh) the bounds build
    assert "$(SRCS)" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    exp = open(os.path.join(ROOT, "scripts", "build_exp.sh")).read()
    assert "make" in exp and "OUT=../lib_exp/$name" in exp
    src = open(os.path.join(ROOT, "gsplat.js_amd", "csrc", "k_select.hip")).read()
    assert "GSR_BOUNDS_DECL(select)" in src
    for site in range(6):
        assert re.search(r"GSR_BOUND\(select, %d," % site, src), site
