// HIPRenderer's neighbour methods against a stub native layer (no GPU, no addon): what reaches the addon, with what flags and
// defaults, and what comes back.  Usage: node neighbour_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    neighbours: (h, radius, cap, scope, budget) => {
        calls.push(["neighbours", h.handle, radius, cap, scope, budget]);
        return { counts: new Uint32Array(5).fill(2), hist: new Uint32Array(cap + 1).fill(1), inScope: 5, nonfinite: 1, pairBound: 2 ** 35, budget: budget || 2 ** 34 };
    },
    selectNeighbours: (h, radius, cap, scope, budget, lo, hi, op) => { calls.push(["selectNeighbours", h.handle, radius, cap, scope, budget, lo, hi, op]); return 4; },
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
    /#define GSR_NEIGHBOUR_MAX_CAP 4095u/.test(header) && /#define GSR_NEIGHBOUR_DEFAULT_BUDGET \(1ull << 34\)/.test(header) &&
    /#define GSR_SCOPE_SELECTED 1u/.test(header) && /#define GSR_SCOPE_VISIBLE  2u/.test(header));
check("neighbours_defaults_scopes_and_result", () => {
    calls.length = 0;
    const a = r.splatNeighbours(0.05);
    r.splatNeighbours(0.5, { cap: 7, scope: "selected" });
    r.splatNeighbours(2, { cap: 4095, scope: ["visible", "selected"], budget: 2 ** 36 });
    r.splatNeighbours(1, { scope: ["visible"], budget: null });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 64, 0, 0], [0.5, 7, 1, 0], [2, 4095, 3, 2 ** 36], [1, 64, 2, 0]]) &&
           a.counts instanceof Uint32Array && a.hist instanceof Uint32Array && a.hist.length === 65 &&
           eq(Object.keys(a), ["counts", "hist", "inScope", "nonfinite", "pairBound"]) && a.inScope === 5 && a.nonfinite === 1 && a.pairBound === 2 ** 35;
});
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = r.selectNeighbours(0.05);
    return k === 4 && eq(calls[0].slice(2), [0.05, 64, 0, 0, 0, 65, 0]);
});
check("below_is_lo_0_hi_below", () => {
    calls.length = 0;
    r.selectNeighbours(0.05, { below: 3 });
    r.selectNeighbours(0.05, { lo: 2, hi: 9, cap: 16, op: "add", scope: "visible" });
    r.selectNeighbours(0.05, { lo: 8, cap: 8, op: "intersect", budget: 1000 });
    r.selectNeighbours(0.05, { lo: 5, hi: 5, op: "subtract" });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 64, 0, 0, 0, 3, 0], [0.05, 16, 2, 0, 2, 9, 1], [0.05, 8, 0, 1000, 8, 9, 3], [0.05, 64, 0, 0, 5, 5, 2]]);
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => r.splatNeighbours(1, { cap: 0 }), /cap must be/], [() => r.splatNeighbours(1, { cap: 4096 }), /cap must be/],
                   [() => r.splatNeighbours(1, { cap: 2.5 }), /cap must be/], [() => r.splatNeighbours(1, { scope: "hidden" }), /must be one of/],
                   [() => r.splatNeighbours(1, { scope: ["selected", "all"] }), /must be one of/], [() => r.splatNeighbours(1, { budget: -1 }), /budget must be/],
                   [() => r.selectNeighbours(1, { op: "xor" }), /must be one of/], [() => r.selectNeighbours(1, { lo: 3, hi: 2 }), /lo <= hi/],
                   [() => r.selectNeighbours(1, { hi: 66 }), /lo <= hi/], [() => r.selectNeighbours(1, { cap: 8, below: 10 }), /lo <= hi/],
                   [() => r.selectNeighbours(1, { below: 3, hi: 4 }), /below goes alone/], [() => r.selectNeighbours(1, { lo: 1.5 }), /lo <= hi/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.neighbours;
    stub.neighbours = () => { throw new Error("gsr_neighbours failed (-1): the count pass would make up to 262144 pair tests, above the budget of 1"); };
    let msg = "";
    try { r.splatNeighbours(0.01, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.neighbours = keep;
    return /262144 pair tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
