// HIPRenderer's contribution methods against a stub native layer (no GPU, no addon): what reaches the addon, in what order, with
// what codes, and what comes back.  Usage: node contrib_binding_check.js  -> JSON { checks, failed, calls }
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const n = 5;
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    contribReset: (h) => { calls.push(["contribReset", h.handle]); },
    contribAccumulate: (h) => { calls.push(["contribAccumulate", h.handle]); },
    readContrib: (h) => {
        calls.push(["readContrib", h.handle]);
        return { weight: BigUint64Array.from([0n, 1n << 40n, 3n, 0n, 16777216n]), peak: Float32Array.from([0, 1, 0.5, 0, 0.25]), pixels: Uint32Array.from([0, 7, 1, 0, 2]), frames: 2 };
    },
    selectContrib: (h, stat, below, op) => { calls.push(["selectContrib", h.handle, stat, below, op]); return 2; },
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

const r = new HIPRenderer({ width: 64, height: 48 }, []);
check("reset_and_accumulate_reach_the_addon_in_order", () => {
    calls.length = 0;
    const a = r.resetContribution(), b = r.accumulateContribution();
    return a === undefined && b === undefined && eq(calls, [["contribReset", 1], ["contribAccumulate", 1]]);
});
check("read_returns_the_typed_arrays_and_frames", () => {
    const c = r.readContribution();
    return c.weight instanceof BigUint64Array && c.peak instanceof Float32Array && c.pixels instanceof Uint32Array && c.weight.length === n &&
           c.weight[1] === (1n << 40n) && c.peak[2] === 0.5 && c.pixels[1] === 7 && c.frames === 2;
});
check("select_defaults_are_weight_zero_replace", () => {
    calls.length = 0;
    return r.selectContribution() === 2 && eq(calls, [["selectContrib", 1, 0, 0, 0]]);
});
check("select_codes_follow_the_header", () => {
    calls.length = 0;
    r.selectContribution({ stat: "weight", below: 0.5, op: "add" });
    r.selectContribution({ stat: "peak", below: 0.01, op: "subtract" });
    r.selectContribution({ stat: "pixels", below: 1, op: "intersect" });
    r.selectContribution({ stat: "pixels", below: Infinity });
    return eq(calls.map((c) => c.slice(2)), [[0, 0.5, 1], [1, 0.01, 2], [2, 1, 3], [2, null, 0]]) && calls[3][3] === Infinity;
});
check("unknown_stat_or_op_throws_before_the_addon", () => {
    calls.length = 0;
    let thrown = 0;
    for (const o of [{ stat: "mass" }, { op: "xor" }, { stat: 3 }]) { try { r.selectContribution(o); } catch (e) { thrown += /must be one of/.test(e.message) ? 1 : 0; } }
    return thrown === 3 && calls.length === 0;
});
check("addon_errors_pass_through", () => {
    const keep = stub.selectContrib;
    stub.selectContrib = () => { throw new Error("gsr_select_contrib failed (-1): no pass has contributed yet (frames == 0)"); };
    let msg = "";
    try { r.selectContribution({ stat: "pixels", below: 1 }); } catch (e) { msg = e.message; }
    stub.selectContrib = keep;
    return /frames == 0/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
