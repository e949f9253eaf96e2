// HIPRenderer's cell methods against a stub native layer (no GPU, no addon): what reaches the addon, with what flags and defaults,
// and what comes back.  Usage: node merge_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const info = { inScope: 9, candidates: 8, cells: 5, mergedCells: 2, mergedMembers: 5, largest: 3, rowsAfter: 6, pairBound: 2 ** 35, budget: 2 ** 34 };
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    cells: (h, cell, cap, scope, budget, leaders) => {
        calls.push(["cells", h.handle, cell, cap, scope, budget, leaders]);
        const out = { hist: new Uint32Array(cap + 1).fill(1), ...info };
        if (leaders) out.leader = new Uint32Array(9);
        return out;
    },
    mergeCells: (h, cell, scope, budget) => { calls.push(["mergeCells", h.handle, cell, scope, budget]); return { count: 6, ...info }; },
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
const KEYS = ["inScope", "candidates", "cells", "mergedCells", "mergedMembers", "largest", "rowsAfter", "pairBound"];

const r = new HIPRenderer({ width: 64, height: 48 }, []);
check("constants_follow_the_header", () => /#define GSR_CELL_NONE 0xffffffffu/.test(header) && /#define GSR_NEIGHBOUR_MAX_CAP 4095u/.test(header));
check("cells_defaults_scopes_and_result", () => {
    calls.length = 0;
    const a = r.splatCells(0.05);
    const b = r.splatCells(0.5, { cap: 7, scope: "selected", leaders: true });
    r.splatCells(2, { cap: 4095, scope: ["visible", "selected"], budget: 2 ** 36 });
    r.splatCells(1, { cap: 1, scope: ["visible"], budget: null });
    return eq(calls.map((c) => c.slice(2)), [[0.05, 64, 0, 0, 0], [0.5, 7, 1, 0, 1], [2, 4095, 3, 2 ** 36, 0], [1, 1, 2, 0, 0]]) &&
           a.hist instanceof Uint32Array && a.hist.length === 65 && a.leader === undefined && eq(Object.keys(a), ["hist"].concat(KEYS)) &&
           a.rowsAfter === 6 && a.mergedCells === 2 && b.leader instanceof Uint32Array && b.leader.length === 9 && b.hist.length === 8;
});
check("merge_defaults_and_result", () => {
    calls.length = 0;
    const a = r.mergeCells(0.25);
    r.mergeCells(0.5, { scope: ["selected", "visible"], budget: 1000 });
    return eq(calls.map((c) => c.slice(2)), [[0.25, 0, 0], [0.5, 3, 1000]]) && eq(Object.keys(a), ["count"].concat(KEYS)) && a.count === 6 && a.rowsAfter === 6;
});
check("bad_arguments_throw_before_the_addon", () => {
    calls.length = 0;
    const tries = [[() => r.splatCells(1, { cap: 0 }), /cap must be/], [() => r.splatCells(1, { cap: 4096 }), /cap must be/], [() => r.splatCells(1, { cap: 2.5 }), /cap must be/],
                   [() => r.splatCells(1, { scope: "hidden" }), /must be one of/], [() => r.splatCells(1, { budget: -1 }), /budget must be/],
                   [() => r.mergeCells(1, { scope: "all" }), /must be one of/], [() => r.mergeCells(1, { budget: -2 }), /budget must be/]];
    let thrown = 0;
    for (const [t, re] of tries) { try { t(); } catch (e) { thrown += re.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.mergeCells;
    stub.mergeCells = () => { throw new Error("gsr_scene_merge_cells failed (-1): the walk would make up to 262144 key tests, above the budget of 1"); };
    let msg = "";
    try { r.mergeCells(0.01, { budget: 1 }); } catch (e) { msg = e.message; }
    stub.mergeCells = keep;
    return /262144 key tests/.test(msg) && /budget of 1/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
