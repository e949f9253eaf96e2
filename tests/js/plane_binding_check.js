// HIPRenderer's plane methods against a stub native layer (no GPU, no addon): what reaches the addon, with what flags and
// defaults, and what comes back.  Usage: node plane_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
let found = 1;
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    fitPlane: (h, threshold, hypotheses, seed, scope, budget, scores) => {
        calls.push(["fitPlane", h.handle, threshold, hypotheses, seed, scope, budget, scores]);
        const r = { plane: Float64Array.of(0, 1, 0, -0.5), triple: Uint32Array.of(3, 1, 2), found, best: 7, inliers: 40, degenerate: 2, inScope: 50, nonfinite: 1,
                    hypotheses, tests: hypotheses * 49, budget: budget || 2 ** 34 };
        if (scores) r.scores = new Uint32Array(hypotheses).fill(5);
        return r;
    },
    planeInliers: (h, planes, count, threshold, scope, budget) => {
        calls.push(["planeInliers", h.handle, Array.from(planes), count, threshold, scope, budget]);
        return { inliers: new Uint32Array(count).fill(9), inScope: 50, nonfinite: 1, hypotheses: count, tests: count * 49, budget: budget || 2 ** 34 };
    },
    selectPlane: (h, plane, lo, hi, op) => { calls.push(["selectPlane", h.handle, Array.from(plane), lo, hi, op]); return 4; },
    planeAlignment: (plane, axis) => { calls.push(["planeAlignment", Array.from(plane), Array.from(axis)]); return { q: Float64Array.of(0.5, 0, 0, 0.75), t: Float64Array.of(0, -0.5, 0) }; },
};
// the addon's place in the module cache: HIPRenderer's loadNative() finds the stub there
const m = new Module(nativePath, null);
m.filename = nativePath; m.loaded = true; m.exports = stub;
require.cache[nativePath] = m;
const { HIPRenderer } = require(path.join(root, "renderers", "HIPRenderer.js"));
const { Quaternion } = require(path.join(root, "math", "Quaternion.js"));
const { Vector3 } = require(path.join(root, "math", "Vector3.js"));

const checks = [], failed = [];
function check(name, fn) {
    checks.push(name);
    try { if (fn() === false) failed.push(name); } catch (e) { failed.push(name + ": " + e.message); }
}
const eq = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const header = fs.readFileSync(path.join(__dirname, "..", "..", "include", "gsplat_hip.h"), "utf8");

const r = new HIPRenderer({ width: 64, height: 48 }, []);
check("constants_follow_the_header", () =>
    /#define GSR_PLANE_MAX_HYPOTHESES 4096u/.test(header) && /#define GSR_NEIGHBOUR_DEFAULT_BUDGET \(1ull << 34\)/.test(header) &&
    /#define GSR_SCOPE_SELECTED 1u/.test(header) && /#define GSR_SCOPE_VISIBLE  2u/.test(header));
check("fit_defaults_scopes_and_result", () => {
    calls.length = 0;
    const a = r.fitPlane(0.01);
    const b = r.fitPlane(0.5, { hypotheses: 4096, seed: 2 ** 40 + 1, scope: "selected", scores: true });
    r.fitPlane(2, { hypotheses: 1, scope: ["visible", "selected"], budget: 2 ** 36 });
    r.fitPlane(1, { scope: ["visible"], budget: null });
    return eq(calls.map((c) => c.slice(2)), [[0.01, 512, 0, 0, 0, false], [0.5, 4096, 2 ** 40 + 1, 1, 0, true], [2, 1, 0, 3, 2 ** 36, false], [1, 512, 0, 2, 0, false]]) &&
           a.plane instanceof Float64Array && eq(Array.from(a.plane), [0, 1, 0, -0.5]) && a.found === true && a.triple instanceof Uint32Array &&
           eq(Object.keys(a), ["plane", "found", "best", "triple", "inliers", "degenerate", "inScope", "nonfinite", "hypotheses", "tests"]) &&
           a.best === 7 && a.inliers === 40 && a.degenerate === 2 && a.inScope === 50 && a.nonfinite === 1 && a.tests === 512 * 49 && a.scores === undefined &&
           b.scores instanceof Uint32Array && b.scores.length === 4096;
});
check("nothing_found_is_a_null_plane", () => {
    found = 0;
    const a = r.fitPlane(0.01);
    found = 1;
    return a.plane === null && a.found === false;
});
check("inliers_flatten_the_planes", () => {
    calls.length = 0;
    const a = r.planeInliers([[0, 1, 0, 0], Float64Array.of(1, 0, 0, -2)], 0.25, { scope: "visible", budget: 1000 });
    r.planeInliers([[0, 0, 2, 1]], 0);
    return a instanceof Uint32Array && eq(Array.from(a), [9, 9]) &&
           eq(calls.map((c) => c.slice(2)), [[[0, 1, 0, 0, 1, 0, 0, -2], 2, 0.25, 2, 1000], [[0, 0, 2, 1], 1, 0, 0, 0]]);
});
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = r.selectPlane([0, 1, 0, -0.5]);
    // (JSON has no infinities: compared apart)
    return k === 4 && eq(calls[0][2], [0, 1, 0, -0.5]) && calls[0][3] === -Infinity && calls[0][4] === Infinity && calls[0][5] === 0;
});
check("within_is_lo_minus_t_hi_t", () => {
    calls.length = 0;
    r.selectPlane([0, 1, 0, 0], { within: 0.01 });
    r.selectPlane([0, 1, 0, 0], { hi: -0.01, op: "add" });
    r.selectPlane(Float64Array.of(0, 1, 0, 0), { lo: 0.5, hi: 2, op: "intersect" });
    r.selectPlane([0, 1, 0, 0], { lo: 3, op: "subtract" });
    return eq(calls.map((c) => [c[3], c[4], c[5]]), [[-0.01, 0.01, 0], [null, -0.01, 1], [0.5, 2, 3], [3, null, 2]]) && calls[1][3] === -Infinity && calls[3][4] === Infinity;
});
check("alignment_returns_a_quaternion_and_a_vector", () => {
    calls.length = 0;
    const a = r.planeAlignment([0, 0, 1, -0.5]);
    r.planeAlignment([0, 0, 1, -0.5], { axis: [0, 0, 1] });
    r.planeAlignment([0, 0, 1, -0.5], { axis: new Vector3(1, 0, 0) });
    return a.rotation instanceof Quaternion && a.translation instanceof Vector3 && eq(a.rotation.flat(), [0.5, 0, 0, 0.75]) &&
           eq([a.translation.x, a.translation.y, a.translation.z], [0, -0.5, 0]) &&
           eq(calls.map((c) => c.slice(1)), [[[0, 0, 1, -0.5], [0, 1, 0]], [[0, 0, 1, -0.5], [0, 0, 1]], [[0, 0, 1, -0.5], [1, 0, 0]]]);
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => r.fitPlane(1, { hypotheses: 0 }), /hypotheses must be/], [() => r.fitPlane(1, { hypotheses: 4097 }), /hypotheses must be/],
                   [() => r.fitPlane(1, { hypotheses: 2.5 }), /hypotheses must be/], [() => r.fitPlane(1, { seed: -1 }), /seed must be/],
                   [() => r.fitPlane(1, { seed: 0.5 }), /seed must be/], [() => r.fitPlane(1, { scope: "hidden" }), /must be one of/],
                   [() => r.fitPlane(1, { budget: -1 }), /budget must be/], [() => r.planeInliers([], 1), /1 \.\. 4096 planes/],
                   [() => r.planeInliers([[0, 1, 0]], 1), /a plane is/], [() => r.planeInliers([[0, 1, 0, 0]], 1, { scope: ["all"] }), /must be one of/],
                   [() => r.selectPlane([0, 1, 0]), /a plane is/], [() => r.selectPlane([0, 1, 0, 0], { op: "xor" }), /must be one of/],
                   [() => r.selectPlane([0, 1, 0, 0], { within: 1, hi: 2 }), /within goes alone/], [() => r.planeAlignment([0, 1]), /a plane is/],
                   [() => r.planeAlignment([0, 1, 0, 0], { axis: [0, 1] }), /axis is/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.fitPlane;
    stub.fitPlane = () => { throw new Error("gsr_fit_plane failed (-1): the scoring pass would make 16448 tests (64 planes x 257 candidates), above the budget of 1"); };
    let msg = "";
    try { r.fitPlane(0.01, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.fitPlane = keep;
    return /16448 tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
