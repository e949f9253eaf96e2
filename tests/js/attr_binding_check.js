// HIPRenderer's splat-data methods against a stub native layer (no GPU, no addon): what reaches the addon, with what codes and
// defaults, and what comes back.  Usage: node attr_binding_check.js  -> JSON { checks, failed, calls }
const fs = require("fs");
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    attrStats: (h, attr, origin, scope) => { calls.push(["attrStats", h.handle, attr, origin && Array.from(origin), scope]); return { count: 5, nan: 1, min: -2.5, max: Infinity }; },
    attrHistogram: (h, attr, origin, scope, lo, hi, bins) => {
        calls.push(["attrHistogram", h.handle, attr, origin && Array.from(origin), scope, lo, hi, bins]);
        return { counts: new Uint32Array(bins).fill(2), below: 3, above: 4, nan: 1 };
    },
    selectAttr: (h, attr, origin, lo, hi, op) => { calls.push(["selectAttr", h.handle, attr, origin && Array.from(origin), lo, hi, op]); return 9; },
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

// the header's codes, read from the header itself
const header = fs.readFileSync(path.join(__dirname, "..", "..", "include", "gsplat_hip.h"), "utf8");
const headerCodes = {};
for (const mm of header.matchAll(/#define GSR_ATTR_([A-Z_]+) (\d+)/g)) headerCodes[mm[1].toLowerCase()] = Number(mm[2]);

const r = new HIPRenderer({ width: 64, height: 48 }, []);
check("codes_follow_the_header", () => {
    calls.length = 0;
    const names = Object.keys(headerCodes);
    for (const name of names) r.splatStats(name);
    return names.length === 16 && eq(calls.map((c) => c[2]), names.map((k) => headerCodes[k])) &&
           /#define GSR_SCOPE_SELECTED 1u/.test(header) && /#define GSR_SCOPE_VISIBLE  2u/.test(header);
});
check("stats_defaults_and_scopes", () => {
    calls.length = 0;
    const s = r.splatStats("opacity");
    r.splatStats("distance", { origin: [1, 2, 3], selected: true });
    r.splatStats("distance", { origin: { x: 4, y: 5, z: 6 }, visible: true });
    r.splatStats("scale_max", { selected: true, visible: true });
    return eq(s, { count: 5, nan: 1, min: -2.5, max: null }) && s.max === Infinity &&
           eq(calls.map((c) => c.slice(2)), [[7, null, 0], [3, [1, 2, 3], 1], [3, [4, 5, 6], 2], [12, null, 3]]);
});
check("histogram_reaches_the_addon_and_returns_counts_and_edges", () => {
    calls.length = 0;
    const h = r.splatHistogram("scale_min", { lo: 0.1, hi: 1.3, bins: 7, visible: true });
    const d = r.splatHistogram("red", { lo: 0, hi: 256 });
    return eq(calls.map((c) => c.slice(2)), [[11, null, 2, 0.1, 1.3, 7], [4, null, 0, 0, 256, 64]]) &&
           h.counts instanceof Uint32Array && h.counts.length === 7 && h.below === 3 && h.above === 4 && h.nan === 1 &&
           h.edges instanceof Float64Array && h.edges.length === 8 && d.edges.length === 65 && d.edges[64] === 256;
});
check("edges_are_computed_by_the_formula", () => {
    for (const [lo, hi, bins] of [[0.1, 1.3, 7], [-3.7, 11.9, 4096], [0, 1, 1], [1e-3, 1e-3 * (1 + 2 ** -40), 257]]) {
        const e = HIPRenderer.attrEdges(lo, hi, bins), w = (hi - lo) / bins;
        if (e.length !== bins + 1 || e[0] !== lo || e[bins] !== hi) return false;
        for (let k = 0; k < bins; k++) if (e[k] !== Math.min(lo + k * w, hi) || e[k + 1] < e[k]) return false;
    }
    // the third edge of [0.1, 1.3) in 7 bins is where a rounded product shows: lo + 3 * w, not lo + (hi - lo) * 3 / 7
    return HIPRenderer.attrEdges(0.1, 1.3, 7)[3] === 0.1 + 3 * ((1.3 - 0.1) / 7);
});
check("select_defaults_are_everything_replace", () => {
    calls.length = 0;
    const k = r.selectAttribute("opacity");
    r.selectAttribute("opacity", { hi: 16 });
    r.selectAttribute("distance", { lo: 2.5, origin: [0, 0, 1], op: "add" });
    r.selectAttribute("contrib_pixels", { lo: 0, hi: 1, op: "intersect" });
    return k === 9 && calls[0][4] === -Infinity && calls[0][5] === Infinity && calls[0][6] === 0 && calls[1][4] === -Infinity && calls[1][5] === 16 &&
           eq(calls[2].slice(2), [3, [0, 0, 1], 2.5, null, 1]) && calls[2][5] === Infinity && eq(calls[3].slice(2), [15, null, 0, 1, 3]);
});
check("unknown_names_throw_before_the_addon", () => {
    calls.length = 0;
    let thrown = 0;
    const tries = [() => r.splatStats("mass"), () => r.splatStats(), () => r.splatStats(7), () => r.splatHistogram("size", { lo: 0, hi: 1, bins: 4 }),
                   () => r.selectAttribute("alpha"), () => r.selectAttribute("opacity", { op: "xor" })];
    for (const t of tries) { try { t(); } catch (e) { thrown += /must be one of/.test(e.message) ? 1 : 0; } }
    let bins = 0;
    for (const b of [0, 4097, 2.5]) { try { r.splatHistogram("opacity", { lo: 0, hi: 1, bins: b }); } catch (e) { bins += /bins must be/.test(e.message) ? 1 : 0; } }
    return thrown === tries.length && bins === 3 && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.attrStats;
    stub.attrStats = () => { throw new Error("gsr_attr_stats failed (-1): GSR_ATTR_DISTANCE needs an origin"); };
    let msg = "";
    try { r.splatStats("distance"); } catch (e) { msg = e.message; }
    stub.attrStats = keep;
    return /needs an origin/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
