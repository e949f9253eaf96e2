// HIPRenderer's matching and registration methods against a stub native layer (no GPU, no addon): what reaches the addon, with what
// flags and defaults, and what comes back.  Usage: node register_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
let handles = 0;
const flat = (m) => (m === null ? null : Array.from(m));
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: ++handles }; },
    destroy: () => {},
    matchScene: (h, t, m, radius, scope, targetScope, budget, sums) => {
        calls.push(["matchScene", h.handle, t.handle, flat(m), radius, scope, targetScope, budget, sums]);
        const r = { idx: Uint32Array.of(2, 0xffffffff, 0), d2: Float64Array.of(0.25, Infinity, 0), inScope: 3, nonfinite: 0, targetIndexed: 5, matched: 2, pairBound: 40,
                    budget: budget || 2 ** 34, d2Min: 0, d2Max: 0.25 };
        if (sums) { r.pairs = 2; r.sums = new Float64Array(16).fill(1.5); }
        return r;
    },
    selectMatch: (h, t, m, radius, scope, targetScope, budget, lo, hi, op) => {
        calls.push(["selectMatch", h.handle, t.handle, flat(m), radius, scope, targetScope, budget, lo, hi, op]);
        return 7;
    },
    registerTo: (h, t, m, radius, scope, targetScope, budget, steps, tolerance, history) => {
        calls.push(["registerTo", h.handle, t.handle, flat(m), radius, scope, targetScope, budget, steps, tolerance, history]);
        const r = { transform: Float64Array.of(1, 0, 0, 0.5, 0, 1, 0, -1, 0, 0, 1, 2), q: Float64Array.of(0, 0, 0.6, 0.8), t: Float64Array.of(0.5, -1, 2), status: 0,
                    iterations: 3, pairs: 900, rms: 0.001, delta: 0 };
        if (history) { r.stepPairs = Float64Array.of(880, 900, 900); r.stepRms = Float64Array.of(0.1, 0.01, 0.001); }
        return r;
    },
    rigidDecompose: (m) => { calls.push(["rigidDecompose", flat(m)]); return { q: Float64Array.of(0.5, 0, 0, 0.75), t: Float64Array.of(m[3], m[7], m[11]) }; },
};
// the addon's place in the module cache: HIPRenderer's loadNative() finds the stub there
const mod = new Module(nativePath, null);
mod.filename = nativePath; mod.loaded = true; mod.exports = stub;
require.cache[nativePath] = mod;
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
const ID = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], MOVE = [0, -1, 0, 0.5, 1, 0, 0, 0, 0, 0, 1, -2];

const a = new HIPRenderer({ width: 64, height: 48 }, []), b = new HIPRenderer({ width: 64, height: 48 }, []);
check("constants_follow_the_header", () =>
    /#define GSR_MATCH_NONE 0xffffffffu/.test(header) && /#define GSR_REGISTER_CONVERGED {6}0/.test(header) && /#define GSR_REGISTER_MAX_ITERATIONS 1/.test(header) &&
    /#define GSR_REGISTER_TOO_FEW {8}2/.test(header) && /#define GSR_REGISTER_MAX_ITERATIONS_LIMIT 256u/.test(header) &&
    /#define GSR_SCOPE_SELECTED 1u/.test(header) && /#define GSR_SCOPE_VISIBLE  2u/.test(header));
check("match_defaults_scopes_and_result", () => {
    calls.length = 0;
    const m = a.matchScene(b, 0.05);
    const s = a.matchScene(b, 0.5, { transform: MOVE, scope: "selected", targetScope: ["visible", "selected"], budget: 2 ** 36, sums: true });
    a.matchScene(a, 1, { transform: Float64Array.from(ID), targetScope: "visible", budget: null });
    return eq(calls.map((c) => c.slice(1)), [[1, 2, null, 0.05, 0, 0, 0, false], [1, 2, MOVE, 0.5, 1, 3, 2 ** 36, true], [1, 1, ID, 1, 0, 2, 0, false]]) &&
           m.idx instanceof Uint32Array && m.d2 instanceof Float64Array && m.d2[1] === Infinity && m.sums === undefined && m.pairs === undefined &&
           eq(Object.keys(m), ["idx", "d2", "inScope", "nonfinite", "targetIndexed", "matched", "pairBound", "d2Min", "d2Max"]) &&
           m.matched === 2 && m.targetIndexed === 5 && m.pairBound === 40 && s.pairs === 2 && s.sums instanceof Float64Array && s.sums.length === 16;
});
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = a.selectMatch(b, 0.05);
    a.selectMatch(b, 0.05, { hi: 0.05, op: "add" });
    a.selectMatch(b, 0.05, { lo: 0.05, op: "subtract", scope: "visible" });
    a.selectMatch(b, 0.05, { lo: 0.01, hi: 0.02, op: "intersect", transform: MOVE, hi2: 1 });
    // (JSON has no infinities: compared apart)
    return k === 7 && eq(calls.map((c) => [c[3], c[5], c[8], c[9], c[10]]), [[null, 0, 0, null, 0], [null, 0, 0, 0.05, 1], [null, 2, 0.05, null, 2], [MOVE, 0, 0.01, 0.02, 3]]) &&
           calls[0][9] === Infinity && calls[2][9] === Infinity;
});
check("register_defaults_and_result", () => {
    calls.length = 0;
    const f = a.registerTo(b, 0.25);
    const g = a.registerTo(b, 0.25, { transform: MOVE, maxIterations: 256, tolerance: 0, history: true, scope: ["selected"], targetScope: "visible", budget: 1000 });
    return eq(calls.map((c) => c.slice(1)), [[1, 2, null, 0.25, 0, 0, 0, 32, 2 ** -40, false], [1, 2, MOVE, 0.25, 1, 2, 1000, 256, 0, true]]) &&
           eq(Object.keys(f), ["transform", "rotation", "translation", "status", "iterations", "pairs", "rms"]) && f.transform instanceof Float64Array &&
           f.rotation instanceof Quaternion && f.translation instanceof Vector3 && eq(f.rotation.flat(), [0, 0, 0.6, 0.8]) &&
           eq([f.translation.x, f.translation.y, f.translation.z], [0.5, -1, 2]) && f.status === "converged" && f.iterations === 3 && f.pairs === 900 && f.rms === 0.001 &&
           f.stepPairs === undefined && eq(Array.from(g.stepPairs), [880, 900, 900]) && eq(Array.from(g.stepRms), [0.1, 0.01, 0.001]);
});
check("status_names_follow_the_codes", () => {
    const keep = stub.registerTo, names = [];
    for (const status of [0, 1, 2]) {
        stub.registerTo = (...args) => ({ ...keep(...args), status });
        names.push(a.registerTo(b, 0.25).status);
    }
    stub.registerTo = keep;
    return eq(names, ["converged", "max_iterations", "too_few"]);
});
check("decompose_returns_a_quaternion_and_a_vector", () => {
    calls.length = 0;
    const d = a.rigidDecompose(MOVE);
    return d.rotation instanceof Quaternion && d.translation instanceof Vector3 && eq(d.rotation.flat(), [0.5, 0, 0, 0.75]) &&
           eq([d.translation.x, d.translation.y, d.translation.z], [0.5, 0, -2]) && eq(calls, [["rigidDecompose", MOVE]]);
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => a.matchScene({}, 0.1), /target must be/], [() => a.matchScene(null, 0.1), /target must be/], [() => a.selectMatch(undefined, 0.1), /target must be/],
                   [() => a.registerTo("b", 0.1), /target must be/], [() => a.matchScene(b, 0.1, { transform: [1, 0, 0] }), /transform is 12 numbers/],
                   [() => a.matchScene(b, 0.1, { scope: "hidden" }), /must be one of/], [() => a.matchScene(b, 0.1, { targetScope: ["all"] }), /must be one of/],
                   [() => a.matchScene(b, 0.1, { budget: -1 }), /budget must be/], [() => a.selectMatch(b, 0.1, { lo: 2, hi: 1 }), /lo <= hi/],
                   [() => a.selectMatch(b, 0.1, { lo: NaN }), /lo <= hi/], [() => a.selectMatch(b, 0.1, { op: "xor" }), /must be one of/],
                   [() => a.registerTo(b, 0.1, { maxIterations: 0 }), /maxIterations must be/], [() => a.registerTo(b, 0.1, { maxIterations: 257 }), /maxIterations must be/],
                   [() => a.registerTo(b, 0.1, { maxIterations: 2.5 }), /maxIterations must be/], [() => a.registerTo(b, 0.1, { tolerance: -1 }), /tolerance must be/],
                   [() => a.registerTo(b, 0.1, { tolerance: NaN }), /tolerance must be/], [() => a.rigidDecompose([1, 0, 0, 0]), /transform is 12 numbers/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("a_disposed_target_is_refused", () => {
    const c = new HIPRenderer({ width: 64, height: 48 }, []);
    c.dispose();
    calls.length = 0;
    let msg = "";
    try { a.matchScene(c, 0.1); } catch (e) { msg = e.message; }
    return /target must be a live HIPRenderer/.test(msg) && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.matchScene;
    stub.matchScene = () => { throw new Error("gsr_match failed (-1): gsr_match: the walk would make up to 9800 pair tests, above the budget of 1"); };
    let msg = "";
    try { a.matchScene(b, 0.3, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.matchScene = keep;
    return /9800 pair tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
