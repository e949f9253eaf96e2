// HIPRenderer's normal methods against a stub native layer (no GPU, no addon): what reaches the addon, with what flags and
// defaults, and what comes back.  Usage: node normal_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    normals: (h, ...a) => {
        calls.push(["normals", h.handle, ...a]);
        return { normals: new Float32Array(18), variation: new Float64Array(6), found: new Uint32Array(6).fill(3), inScope: 5, nonfinite: 1, pairBound: 2 ** 35,
                 budget: 2 ** 34, valid: 4, variationMin: 0, variationMax: 0.25 };
    },
    selectNormal: (h, ...a) => { calls.push(["selectNormal", h.handle, ...a]); return 4; },
};
// the addon's place in the module cache: HIPRenderer's loadNative() finds the stub there
const m = new Module(nativePath, null);
m.filename = nativePath; m.loaded = true; m.exports = stub;
require.cache[nativePath] = m;
const { HIPRenderer } = require(path.join(root, "renderers", "HIPRenderer.js"));

const checks = [], failed = [];
function check(name, fn) {
    checks.push(name);
    try { if (fn() === false) failed.push(name); } catch (e) { failed.push(name + ": " + e.message); }
}
const eq = (a, b) => JSON.stringify(a) === JSON.stringify(b);
const header = fs.readFileSync(path.join(__dirname, "..", "..", "include", "gsplat_hip.h"), "utf8");

const r = new HIPRenderer({ width: 64, height: 48 }, []);
check("constants_follow_the_header", () =>
    /#define GSR_NORMAL_KNN 0 /.test(header) && /#define GSR_NORMAL_OWN 1 /.test(header) && /#define GSR_NORMAL_DOT 0 /.test(header) &&
    /#define GSR_NORMAL_ABS_DOT 1 /.test(header) && /#define GSR_NORMAL_VARIATION 2 /.test(header));
// the addon's arguments behind the handle: source, radius, k, scope, budget, oriented, tx, ty, tz
check("normals_defaults_sources_scopes_and_result", () => {
    calls.length = 0;
    const a = r.splatNormals(0.05);
    r.splatNormals(0.5, { k: 2, scope: "selected", toward: [1, -2, 3.5] });
    r.splatNormals(2, { k: 32, scope: ["visible", "selected"], budget: 2 ** 36, toward: new Float64Array([0, 0, 0]) });
    r.splatNormals(undefined, { source: "own", scope: ["visible"], budget: null, k: 99 });
    return eq(calls.map((c) => c.slice(2)), [[0, 0.05, 8, 0, 0, 0, 0, 0, 0], [0, 0.5, 2, 1, 0, 1, 1, -2, 3.5], [0, 2, 32, 3, 2 ** 36, 1, 0, 0, 0], [1, 0, 0, 2, 0, 0, 0, 0, 0]]) &&
           a.normals instanceof Float32Array && a.normals.length === 18 && a.variation instanceof Float64Array && a.found instanceof Uint32Array &&
           eq(Object.keys(a), ["normals", "variation", "found", "inScope", "nonfinite", "pairBound", "valid", "variationMin", "variationMax"]) &&
           a.inScope === 5 && a.valid === 4 && a.variationMax === 0.25;
});
// .. then stat, hasAxis, ax, ay, az, lo, hi, op
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = r.selectNormal("variation", { radius: 0.05 });
    return k === 4 && eq(calls[0].slice(2), [0, 0.05, 8, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, null, null, 0]) && calls[0][16] === -Infinity && calls[0][17] === Infinity;
});
check("select_passes_the_stat_the_axis_the_range_and_the_op", () => {
    calls.length = 0;
    r.selectNormal("abs_dot", { radius: 0.05, axis: [0, 1, 0], hi: 0.2 });
    r.selectNormal("dot", { radius: 0.1, k: 16, axis: new Float32Array([0.5, 0, -2]), lo: 0.125, hi: 0.5, op: "add", scope: "visible", toward: [4, 5, 6] });
    r.selectNormal("variation", { source: "own", lo: 0.1, op: "intersect", budget: 1000 });
    r.selectNormal("variation", { radius: 0.05, lo: 0.5, hi: 0.5, op: "subtract" });
    return eq(calls.map((c) => c.slice(2)), [[0, 0.05, 8, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, null, 0.2, 0], [0, 0.1, 16, 2, 0, 1, 4, 5, 6, 0, 1, 0.5, 0, -2, 0.125, 0.5, 1],
                                             [1, 0, 0, 0, 1000, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0.1, null, 3], [0, 0.05, 8, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0.5, 0.5, 2]]) &&
           calls[0][16] === -Infinity && calls[2][17] === Infinity;
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => r.splatNormals(1, { k: 1 }), /k must be/], [() => r.splatNormals(1, { k: 33 }), /k must be/], [() => r.splatNormals(1, { k: 2.5 }), /k must be/],
                   [() => r.splatNormals(1, { source: "pca" }), /must be one of/], [() => r.splatNormals(1, { scope: "hidden" }), /must be one of/],
                   [() => r.splatNormals(1, { budget: -1 }), /budget must be/], [() => r.splatNormals(1, { toward: [1, 2] }), /toward must hold/],
                   [() => r.selectNormal("median", { radius: 1 }), /must be one of/], [() => r.selectNormal(undefined, { radius: 1 }), /must be one of/],
                   [() => r.selectNormal("dot", { radius: 1 }), /axis must hold/], [() => r.selectNormal("abs_dot", { radius: 1, axis: [1] }), /axis must hold/],
                   [() => r.selectNormal("variation", { radius: 1, op: "xor" }), /must be one of/], [() => r.selectNormal("variation", { radius: 1, lo: 3, hi: 2 }), /lo <= hi/],
                   [() => r.selectNormal("variation", { radius: 1, lo: NaN }), /lo <= hi/], [() => r.selectNormal("variation", { radius: 1, hi: NaN }), /lo <= hi/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.normals;
    stub.normals = () => { throw new Error("gsr_normals failed (-1): the count pass would make up to 262144 pair tests, above the budget of 1"); };
    let msg = "";
    try { r.splatNormals(0.01, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.normals = keep;
    return /262144 pair tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
