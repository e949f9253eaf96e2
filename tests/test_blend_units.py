"""The compositor's two translation units: k_blend1.hip holds the one-wave-per-tile kernels and is built
without the SLP vectoriser, k_blend.hip holds the two-waves-per-tile kernels and the rest with the default flags, and both
instantiate the one body of k_blend_body.h.  Checked here: the Makefile wires them so, and the built libraries hold all four
kernels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsplat.js_amd", "csrc")
KERNELS = ("_ZN3gsr7k_blendEPKj", "_ZN3gsr8k_blend2EPKj", "_ZN3gsr15k_blend_unfusedEPKj", "_ZN3gsr16k_blend2_unfusedEPKj")


def test_makefile_builds_the_two_units_with_their_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    for f in ("k_blend.hip", "k_blend1.hip"):
        assert srcs.count(f) == 1 and os.path.exists(os.path.join(CSRC, f)), f
    assert re.search(r"^FLAGS_k_blend1 := -fno-slp-vectorize\s*$", mk, flags=re.M)
    assert not re.search(r"^FLAGS_k_blend\s*[:+?]?=", mk, flags=re.M)              # k_blend2's unit keeps the default flags
    assert "$(FLAGS_$*)" in mk                                                     # the pattern rule applies a unit's flags
    # the shared body reaches the build id and rebuilds both units
    assert "k_blend_body.h" in re.search(r"^BUILD_ID := (.*)$", mk, flags=re.M).group(1)
    assert re.search(r"^\$\(OUT\)/%\.o: %\.hip .*k_blend_body\.h", mk, flags=re.M)


def test_the_body_is_stated_once_and_kernels_are_handed_over_by_their_unit():
    body, one, two = (open(os.path.join(CSRC, f)).read() for f in ("k_blend_body.h", "k_blend1.hip", "k_blend.hip"))
    assert body.count("void blend_body(") == 1 and "GSR_ASM_WALK_STEP()" in body
    for unit in (one, two):
        assert '#include "k_blend_body.h"' in unit and "void blend_body(" not in unit and "GSR_ASM_QUAD" not in unit
    code = re.sub(r"//.*", "", two)
    assert "blend_body<1," not in two and "blend_body<2," not in one
    assert "blend1_kernel(true)" in code and "blend1_kernel(false)" in code        # never the address of another unit's __global__
    assert not re.search(r"\bk_blend\b", code) and not re.search(r"\bk_blend_unfused\b", code)
    assert "BlendFn blend1_kernel(bool fused)" in one and "BlendFn blend1_kernel(bool fused);" in body


def test_libraries_hold_all_four_compositor_kernels():
    import gsplat_hip as gh
    libs = [gh.LIB_PATH] + [os.path.join(ROOT, "gsplat.js_amd", "lib_exp", twin, "libgsplat_hip.so") for twin in ("bounds", "cppwalk")]
    for p in libs:
        assert os.path.exists(p), p
        out = subprocess.run(["strings", "-a", p], capture_output=True, text=True).stdout
        assert "gfx950" in out
        for k in KERNELS:
            assert k in out, (p, k)
