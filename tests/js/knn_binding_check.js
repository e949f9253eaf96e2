// HIPRenderer's k-nearest-neighbour methods against a stub native layer (no GPU, no addon): what reaches the addon, with what
// flags and defaults, and what comes back.  Usage: node knn_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
let values = new Float64Array([1, 2, 3, Infinity, NaN, 6]);
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    knn: (h, radius, k, scope, budget, stat, lists) => {
        calls.push(["knn", h.handle, radius, k, scope, budget, stat, lists]);
        const out = { found: new Uint32Array(6).fill(2), values, hist: new Uint32Array(k + 1).fill(1), inScope: 5, nonfinite: 1, pairBound: 2 ** 35, budget: budget || 2 ** 34,
                      complete: 3, finiteValues: 4, valueMin: 1, valueMax: 6 };
        if (lists) { out.idx = new Uint32Array(6 * k); out.d2 = new Float64Array(6 * k); }
        return out;
    },
    selectKnn: (h, radius, k, scope, budget, stat, lo, hi, op) => { calls.push(["selectKnn", h.handle, radius, k, scope, budget, stat, lo, hi, op]); return 4; },
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
    /#define GSR_KNN_MAX_K 32u/.test(header) && /#define GSR_KNN_NONE  0xffffffffu/.test(header) && /#define GSR_KNN_KTH  0 /.test(header) &&
    /#define GSR_KNN_MEAN 1 /.test(header));
check("knn_defaults_scopes_and_result", () => {
    calls.length = 0;
    const a = r.splatKnn(0.05);
    const b = r.splatKnn(0.5, { k: 7, stat: "kth", scope: "selected", lists: true });
    r.splatKnn(2, { k: 32, scope: ["visible", "selected"], budget: 2 ** 36 });
    r.splatKnn(1, { k: 1, stat: "mean", scope: ["visible"], budget: null });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 8, 0, 0, 1, 0], [0.5, 7, 1, 0, 0, 1], [2, 32, 3, 2 ** 36, 1, 0], [1, 1, 2, 0, 1, 0]]) &&
           a.found instanceof Uint32Array && a.values instanceof Float64Array && a.hist.length === 9 && a.idx === undefined && a.d2 === undefined &&
           eq(Object.keys(a), ["found", "values", "hist", "inScope", "nonfinite", "pairBound", "complete", "finiteValues", "valueMin", "valueMax"]) &&
           a.inScope === 5 && a.complete === 3 && a.finiteValues === 4 && a.valueMax === 6 && b.idx.length === 42 && b.d2 instanceof Float64Array;
});
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = r.selectKnn(0.05);
    return k === 4 && eq(calls[0].slice(2), [0.05, 8, 0, 0, 1, 0, null, 0]) && calls[0][8] === Infinity;      // (JSON writes Infinity as null)
});
check("select_passes_the_range_the_stat_and_the_op", () => {
    calls.length = 0;
    r.selectKnn(0.05, { lo: 0.25 });
    r.selectKnn(0.05, { lo: 0.125, hi: 0.5, k: 16, stat: "kth", op: "add", scope: "visible" });
    r.selectKnn(0.05, { lo: Infinity, k: 3, op: "intersect", budget: 1000 });
    r.selectKnn(0.05, { lo: 0.5, hi: 0.5, op: "subtract" });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 8, 0, 0, 1, 0.25, null, 0], [0.05, 16, 2, 0, 0, 0.125, 0.5, 1], [0.05, 3, 0, 1000, 1, null, null, 3],
                                             [0.05, 8, 0, 0, 1, 0.5, 0.5, 2]]) && calls[2][7] === Infinity;
});
check("outliers_read_the_mean_and_select_above_the_threshold", () => {
    calls.length = 0;
    const out = r.selectStatisticalOutliers(0.05, { k: 5, stdRatio: 2, scope: "visible", op: "add" });
    const mu = 3, sigma = Math.sqrt(14 / 3);      // of 1, 2, 3, 6: the sample standard deviation
    const few = (() => { const keep = values; values = new Float64Array([1, Infinity]); const o = r.selectStatisticalOutliers(0.05); values = keep; return o; })();
    return out.selected === 4 && Math.abs(out.threshold - (mu + 2 * sigma)) < 1e-14 && eq(calls[0].slice(2), [0.05, 5, 2, 0, 1, 0]) &&
           eq(calls[1].slice(2, 7), [0.05, 5, 2, 0, 1]) && calls[1][7] === out.threshold && calls[1][8] === Infinity && calls[1][9] === 1 &&
           few.threshold === Infinity && calls[3][7] === Infinity && eq(calls[3].slice(2, 7), [0.05, 8, 0, 0, 1]);
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => r.splatKnn(1, { k: 0 }), /k must be/], [() => r.splatKnn(1, { k: 33 }), /k must be/], [() => r.splatKnn(1, { k: 2.5 }), /k must be/],
                   [() => r.splatKnn(1, { stat: "median" }), /must be one of/], [() => r.splatKnn(1, { scope: "hidden" }), /must be one of/],
                   [() => r.splatKnn(1, { budget: -1 }), /budget must be/], [() => r.selectKnn(1, { op: "xor" }), /must be one of/],
                   [() => r.selectKnn(1, { lo: 3, hi: 2 }), /lo <= hi/], [() => r.selectKnn(1, { lo: NaN }), /lo <= hi/], [() => r.selectKnn(1, { hi: NaN }), /lo <= hi/],
                   [() => r.selectStatisticalOutliers(1, { k: 40 }), /k must be/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.knn;
    stub.knn = () => { throw new Error("gsr_knn failed (-1): the count pass would make up to 262144 pair tests, above the budget of 1"); };
    let msg = "";
    try { r.splatKnn(0.01, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.knn = keep;
    return /262144 pair tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
