// HIPRenderer's cluster methods against a stub native layer (no GPU, no addon): what reaches the addon, with what flags and
// defaults, and what comes back.  Usage: node cluster_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const LARGEST = 0xffffffff;
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    clusters: (h, radius, minPts, scope, budget) => {
        calls.push(["clusters", h.handle, radius, minPts, scope, budget]);
        return { labels: new Uint32Array(5).fill(1), sizes: new Uint32Array(5).fill(4), inScope: 5, nonfinite: 0, pairBound: 2 ** 35, budget: budget || 2 ** 34,
                 core: 3, border: 1, noise: 1, clusters: 1, largestLabel: 1, largestSize: 4 };
    },
    selectClusters: (h, radius, minPts, scope, budget, lo, hi, op) => { calls.push(["selectClusters", h.handle, radius, minPts, scope, budget, lo, hi, op]); return 4; },
    selectClusterAt: (h, radius, minPts, scope, budget, seed, op) => { calls.push(["selectClusterAt", h.handle, radius, minPts, scope, budget, seed, op]); return 3; },
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
    /#define GSR_CLUSTER_NONE    0xffffffffu/.test(header) && /#define GSR_CLUSTER_LARGEST 0xffffffffu/.test(header) && /#define GSR_NEIGHBOUR_MAX_CAP 4095u/.test(header) &&
    /#define GSR_SCOPE_SELECTED 1u/.test(header) && /#define GSR_SCOPE_VISIBLE  2u/.test(header));
check("clusters_defaults_scopes_and_result", () => {
    calls.length = 0;
    const a = r.splatClusters(0.05);
    r.splatClusters(0.5, { minPts: 7, scope: "selected" });
    r.splatClusters(2, { minPts: 4095, scope: ["visible", "selected"], budget: 2 ** 36 });
    r.splatClusters(1, { scope: ["visible"], budget: null });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 0, 0, 0], [0.5, 7, 1, 0], [2, 4095, 3, 2 ** 36], [1, 0, 2, 0]]) &&
           a.labels instanceof Uint32Array && a.sizes instanceof Uint32Array && a.labels.length === 5 &&
           eq(Object.keys(a), ["labels", "sizes", "inScope", "nonfinite", "pairBound", "core", "border", "noise", "clusters", "largestLabel", "largestSize"]) &&
           a.inScope === 5 && a.core === 3 && a.border === 1 && a.noise === 1 && a.clusters === 1 && a.largestLabel === 1 && a.largestSize === 4 && a.pairBound === 2 ** 35;
});
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = r.selectClusters(0.05);
    return k === 4 && eq(calls[0].slice(2), [0.05, 0, 0, 0, 0, LARGEST, 0]);
});
check("below_and_at_least_are_the_size_range", () => {
    calls.length = 0;
    r.selectClusters(0.05, { below: 50 });
    r.selectClusters(0.05, { atLeast: 2, below: 9, minPts: 3, op: "add", scope: "visible" });
    r.selectClusters(0.05, { atLeast: 100, op: "intersect", budget: 1000 });
    r.selectClusters(0.05, { atLeast: 5, below: 5, op: "subtract" });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 0, 0, 0, 0, 50, 0], [0.05, 3, 2, 0, 2, 9, 1], [0.05, 0, 0, 1000, 100, LARGEST, 3], [0.05, 0, 0, 0, 5, 5, 2]]);
});
check("seed_or_largest", () => {
    calls.length = 0;
    const k = r.selectClusterAt(0.05, { seed: 17 });
    r.selectClusterAt(0.05, { largest: true, minPts: 2, scope: "selected", op: "subtract" });
    r.selectClusterAt(0.1, { seed: 0, op: "add", budget: 5 });
    return k === 3 && eq(calls.map((c) => c.slice(2)), [[0.05, 0, 0, 0, 17, 0], [0.05, 2, 1, 0, LARGEST, 2], [0.1, 0, 0, 5, 0, 1]]);
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => r.splatClusters(1, { minPts: -1 }), /minPts must be/], [() => r.splatClusters(1, { minPts: 4096 }), /minPts must be/],
                   [() => r.splatClusters(1, { minPts: 2.5 }), /minPts must be/], [() => r.splatClusters(1, { scope: "hidden" }), /must be one of/],
                   [() => r.splatClusters(1, { budget: -1 }), /budget must be/], [() => r.selectClusters(1, { op: "xor" }), /must be one of/],
                   [() => r.selectClusters(1, { atLeast: 3, below: 2 }), /atLeast <= below/], [() => r.selectClusters(1, { below: 2 ** 32 }), /atLeast <= below/],
                   [() => r.selectClusters(1, { atLeast: 1.5 }), /atLeast <= below/], [() => r.selectClusterAt(1), /either seed/],
                   [() => r.selectClusterAt(1, {}), /either seed/], [() => r.selectClusterAt(1, { seed: 3, largest: true }), /either seed/],
                   [() => r.selectClusterAt(1, { seed: -1 }), /splat index/], [() => r.selectClusterAt(1, { seed: 2.5 }), /splat index/],
                   [() => r.selectClusterAt(1, { seed: 0xffffffff }), /splat index/], [() => r.selectClusterAt(1, { seed: 1, op: "xor" }), /must be one of/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.clusters;
    stub.clusters = () => { throw new Error("gsr_clusters failed (-1): the count pass would make up to 262144 pair tests, above the budget of 1"); };
    let msg = "";
    try { r.splatClusters(0.01, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.clusters = keep;
    return /262144 pair tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
