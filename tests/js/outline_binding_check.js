// HIPRenderer.setSelectionOutline against a stub native layer (no GPU, no addon): what reaches the addon, with what arguments.
// Usage: node outline_binding_check.js  -> JSON { checks, failed, calls }
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const W = 64, H = 48;
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    setOverlay: (h, on, r, g, b, mix) => { calls.push(["setOverlay", h.handle, on, r, g, b, mix]); },
    setOutline: (h, on, r, g, b, alpha, threshold, width, side) => { calls.push(["setOutline", h.handle, on, r, g, b, alpha, threshold, width, side]); },
    detachBuffers: () => {},
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

const r = new HIPRenderer({ width: W, height: H }, []);
check("options_reach_the_addon_with_defaults", () => {
    calls.length = 0;
    r.setSelectionOutline({});
    r.setSelectionOutline({ color: [0.125, 7, -3], alpha: 0.5, threshold: 0.25, width: 16, side: "inner" });
    return eq(calls, [["setOutline", 1, 1, 1, 1, 1, 1, 0.5, 2, 0], ["setOutline", 1, 1, 0.125, 7, -3, 0.5, 0.25, 16, 1]]);
});
check("null_switches_it_off", () => {
    calls.length = 0;
    r.setSelectionOutline(null);
    r.setSelectionOutline();
    return eq(calls, [["setOutline", 1, 0, 0, 0, 0, 0, 0, 0, 0], ["setOutline", 1, 0, 0, 0, 0, 0, 0, 0, 0]]);
});
check("bad_options_throw_before_the_addon", () => {
    calls.length = 0;
    let thrown = 0;
    for (const [o, re] of [[{ color: [1, 2] }, /color must be/], [{ color: 3 }, /color must be/], [{ side: "both" }, /side must be one of outer, inner/],
                           [{ width: 2.5 }, /width must be an integer/]]) {
        try { r.setSelectionOutline(o); } catch (e) { thrown += re.test(e.message) ? 1 : 0; }
    }
    return thrown === 4 && calls.length === 0;
});
check("the_overlay_call_is_what_it_was", () => {
    calls.length = 0;
    r.setSelectionOverlay({});
    return eq(calls, [["setOverlay", 1, 1, 1, 0.5, 0, 0.5]]);
});
check("addon_errors_pass_through", () => {
    const keep = stub.setOutline;
    stub.setOutline = () => { throw new Error("gsr_set_overlay_outline failed (-1): gsr_set_overlay_outline: no overlay options (gsr_set_overlay first)"); };
    let msg = "";
    try { r.setSelectionOutline({}); } catch (e) { msg = e.message; }
    stub.setOutline = keep;
    return /no overlay options/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
