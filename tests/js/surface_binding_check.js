// HIPRenderer's point-to-plane methods against a stub native layer (no GPU, no addon): what reaches the addon, with what flags and
// defaults, and what comes back.  Usage: node surface_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
let handles = 0;
const flat = (m) => (m === null ? null : Array.from(m));
const fitOf = (history) => {
    const r = { transform: Float64Array.of(1, 0, 0, 0.5, 0, 1, 0, -1, 0, 0, 1, 2), q: Float64Array.of(0, 0, 0.6, 0.8), t: Float64Array.of(0.5, -1, 2), status: 0,
                iterations: 3, pairs: 900, surfacePairs: 850, rms: 0.03, surfaceRms: 0.001, delta: 0, valid: 1200 };
    if (history) {
        r.stepPairs = Float64Array.of(880, 900, 900); r.stepSurfacePairs = Float64Array.of(830, 850, 850);
        r.stepRms = Float64Array.of(0.1, 0.04, 0.03); r.stepSurfaceRms = Float64Array.of(0.1, 0.01, 0.001);
    }
    return r;
};
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: ++handles }; },
    destroy: () => {},
    matchSurface: (h, t, m, radius, scope, targetScope, budget, source, nradius, k, nbudget) => {
        calls.push(["matchSurface", h.handle, t.handle, flat(m), radius, scope, targetScope, budget, source, nradius, k, nbudget]);
        return { pairs: 3, surfacePairs: 2, sums: new Float64Array(29).fill(0.5), inScope: 4, nonfinite: 0, targetIndexed: 5, matched: 3, pairBound: 40, budget: budget || 2 ** 34,
                 d2Min: 0, d2Max: 0.25 };
    },
    registerSurface: (h, t, m, radius, scope, targetScope, budget, source, nradius, k, nbudget, steps, tolerance, history) => {
        calls.push(["registerSurface", h.handle, t.handle, flat(m), radius, scope, targetScope, budget, source, nradius, k, nbudget, steps, tolerance, history]);
        return fitOf(history);
    },
    registerTo: (h, t, m, radius, scope, targetScope, budget, steps, tolerance, history) => {
        calls.push(["registerTo", h.handle, t.handle, flat(m), radius, scope, targetScope, budget, steps, tolerance, history]);
        return { transform: Float64Array.of(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), q: Float64Array.of(0, 0, 0, 1), t: Float64Array.of(0, 0, 0), status: 1, iterations: 32, pairs: 9,
                 rms: 0.5, delta: 0.1 };
    },
    surfaceSolve: (pairs, sums) => { calls.push(["surfaceSolve", pairs, sums.length]); return { transform: Float64Array.of(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), rms: 0.25, degenerate: 0 }; },
};
// the addon's place in the module cache: HIPRenderer's loadNative() finds the stub there
const mod = new Module(nativePath, null);
mod.filename = nativePath; mod.loaded = true; mod.exports = stub;
require.cache[nativePath] = mod;
const G = require(root);
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
const MOVE = [0, -1, 0, 0.5, 1, 0, 0, 0, 0, 0, 1, -2];

const a = new HIPRenderer({ width: 64, height: 48 }, []), b = new HIPRenderer({ width: 64, height: 48 }, []);
check("constants_follow_the_header", () =>
    /#define GSR_REGISTER_DEGENERATE 3/.test(header) && /#define GSR_NORMAL_KNN 0 /.test(header) && /#define GSR_NORMAL_OWN 1 /.test(header));
check("residual_point_is_the_path_of_today", () => {
    calls.length = 0;
    const f = a.registerTo(b, 0.25), g = a.registerTo(b, 0.25, { residual: "point" });
    return eq(calls, [["registerTo", 1, 2, null, 0.25, 0, 0, 0, 32, 2 ** -40, false], ["registerTo", 1, 2, null, 0.25, 0, 0, 0, 32, 2 ** -40, false]]) &&
           eq(Object.keys(f), ["transform", "rotation", "translation", "status", "iterations", "pairs", "rms"]) && eq(Object.keys(g), Object.keys(f)) && f.status === "max_iterations";
});
check("residual_surface_defaults_and_result", () => {
    calls.length = 0;
    const f = a.registerTo(b, 0.25, { residual: "surface" });
    const g = a.registerTo(b, 0.25, { residual: "surface", normals: { source: "knn", radius: 0.15, k: 6, budget: 77 }, transform: MOVE, maxIterations: 256, tolerance: 0, history: true,
                                      scope: ["selected"], targetScope: "visible", budget: 1000 });
    a.registerTo(b, 0.25, { residual: "surface", normals: { source: "knn", radius: 0.5 } });
    return eq(calls.map((c) => c.slice(1)), [[1, 2, null, 0.25, 0, 0, 0, 1, 0, 0, 0, 32, 2 ** -40, false], [1, 2, MOVE, 0.25, 1, 2, 1000, 0, 0.15, 6, 77, 256, 0, true],
                                             [1, 2, null, 0.25, 0, 0, 0, 0, 0.5, 8, 0, 32, 2 ** -40, false]]) && calls.every((c) => c[0] === "registerSurface") &&
           eq(Object.keys(f), ["transform", "rotation", "translation", "status", "iterations", "pairs", "surfacePairs", "rms", "surfaceRms", "delta", "valid"]) &&
           f.rotation instanceof Quaternion && f.translation instanceof Vector3 && eq(f.rotation.flat(), [0, 0, 0.6, 0.8]) && f.status === "converged" &&
           f.surfacePairs === 850 && f.surfaceRms === 0.001 && f.valid === 1200 && f.stepPairs === undefined &&
           eq(Array.from(g.stepSurfacePairs), [830, 850, 850]) && eq(Array.from(g.stepSurfaceRms), [0.1, 0.01, 0.001]) && eq(Array.from(g.stepPairs), [880, 900, 900]);
});
check("status_names_follow_the_codes", () => {
    const keep = stub.registerSurface, names = [];
    for (const status of [0, 1, 2, 3]) {
        stub.registerSurface = (...args) => ({ ...keep(...args), status });
        names.push(a.registerTo(b, 0.25, { residual: "surface" }).status);
    }
    stub.registerSurface = keep;
    return eq(names, ["converged", "max_iterations", "too_few", "degenerate"]);
});
check("match_surface_defaults_and_result", () => {
    calls.length = 0;
    const m = a.matchSurface(b, 0.05);
    a.matchSurface(a, 0.5, { transform: MOVE, scope: "selected", targetScope: ["visible", "selected"], budget: 2 ** 36, normals: { source: "knn", radius: 0.2, k: 4 } });
    return eq(calls.map((c) => c.slice(1)), [[1, 2, null, 0.05, 0, 0, 0, 1, 0, 0, 0], [1, 1, MOVE, 0.5, 1, 3, 2 ** 36, 0, 0.2, 4, 0]]) &&
           eq(Object.keys(m), ["pairs", "surfacePairs", "sums", "inScope", "nonfinite", "targetIndexed", "matched", "pairBound", "d2Min", "d2Max"]) &&
           m.sums instanceof Float64Array && m.sums.length === 29 && m.pairs === 3 && m.surfacePairs === 2;
});
check("surface_solve_is_a_module_function", () => {
    calls.length = 0;
    const s = G.surfaceSolve({ surfacePairs: 12, sums: new Float64Array(29) });
    return typeof G.surfaceSolve === "function" && eq(calls, [["surfaceSolve", 12, 29]]) && s.degenerate === 0 && s.rms === 0.25 && s.transform.length === 12;
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => a.registerTo(b, 0.1, { residual: "plane" }), /residual is/], [() => a.registerTo(b, 0.1, { normals: { source: "own" } }), /normals goes with residual/],
                   [() => a.registerTo(b, 0.1, { residual: "point", normals: {} }), /normals goes with residual/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", normals: { source: "pca" } }), /must be one of/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", normals: { source: "knn" } }), /needs a radius/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", normals: { source: "knn", radius: 0.1, k: 1 } }), /normals.k must be/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", normals: { source: "knn", radius: 0.1, k: 33 } }), /normals.k must be/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", normals: { budget: -1 } }), /normals.budget must be/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", maxIterations: 0 }), /maxIterations must be/],
                   [() => a.registerTo(b, 0.1, { residual: "surface", tolerance: -1 }), /tolerance must be/], [() => a.registerTo({}, 0.1, { residual: "surface" }), /target must be/],
                   [() => a.matchSurface(null, 0.1), /target must be/], [() => a.matchSurface(b, 0.1, { transform: [1, 0, 0] }), /transform is 12 numbers/],
                   [() => a.matchSurface(b, 0.1, { targetScope: "hidden" }), /must be one of/], [() => G.surfaceSolve({ surfacePairs: 9, sums: [1, 2, 3] }), /29 values/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.registerSurface;
    stub.registerSurface = () => { throw new Error("gsr_register_surface failed (-1): gsr_register_surface: options->scope (0) is not target_scope (2)"); };
    let msg = "";
    try { a.registerTo(b, 0.3, { residual: "surface" }); } catch (e) { msg = e.message; }
    stub.registerSurface = keep;
    return /is not target_scope/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
