// HIPRenderer's selection-overlay methods against a stub native layer (no GPU, no addon): what reaches the addon, in what order,
// with what arguments, and what comes back.  Usage: node overlay_binding_check.js  -> JSON { checks, failed, calls }
const path = require("path");
const Module = require("module");

const root = path.join(__dirname, "..", "..", "gsplat.js_amd", "js");
const nativePath = path.join(root, "native", "gsplat_hip.node");
const calls = [];
const W = 64, H = 48;
let ring = 0;                                    // the open ring's format code
const stub = {
    create: (o) => { calls.push(["create", o.width, o.height]); return { handle: 1 }; },
    destroy: () => {},
    setOverlay: (h, on, r, g, b, mix) => { calls.push(["setOverlay", h.handle, on, r, g, b, mix]); },
    readOverlay: (h, w, hh) => { calls.push(["readOverlay", h.handle, w, hh]); return { rgba: new Float32Array(w * hh * 4).fill(0.25), cover: new Float32Array(w * hh).fill(0.5) }; },
    readOverlayPixels: (h, out, w, hh) => { calls.push(["readOverlayPixels", h.handle, out.length, w, hh]); out.fill(7); },
    readPixels: (h, out, w, hh) => { calls.push(["readPixels", h.handle, out.length, w, hh]); out.fill(3); },
    openDelivery: (h, n) => { calls.push(["openDelivery", h.handle, n]); ring = 0; return Array.from({ length: n }, () => new ArrayBuffer(W * H * 4)); },
    openDeliveryEx: (h, n, format) => { calls.push(["openDeliveryEx", h.handle, n, format]); ring = format; return Array.from({ length: n }, () => new ArrayBuffer(W * H * 3 / 2)); },
    deliveryLayout: () => (ring === 0 ? { format: 0, width: W, height: H, bytes: W * H * 4, planes: [{ offset: 0, stride: W * 4, rows: H }] }
                                      : { format: ring, width: W, height: H, bytes: W * H * 3 / 2, planes: [{ offset: 0, stride: W, rows: H }, { offset: W * H, stride: W, rows: H / 2 }] }),
    deliverySetOverlay: (h, on) => { calls.push(["deliverySetOverlay", h.handle, on]); },
    closeDelivery: (h) => { calls.push(["closeDelivery", h.handle]); },
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
    r.setSelectionOverlay({});
    r.setSelectionOverlay({ tint: [0, 1, 0.25], mix: 1 });
    return eq(calls, [["setOverlay", 1, 1, 1, 0.5, 0, 0.5], ["setOverlay", 1, 1, 0, 1, 0.25, 1]]);
});
check("null_switches_it_off", () => {
    calls.length = 0;
    r.setSelectionOverlay(null);
    return eq(calls, [["setOverlay", 1, 0, 0, 0, 0, 0]]);
});
check("a_bad_tint_throws_before_the_addon", () => {
    calls.length = 0;
    let thrown = 0;
    for (const o of [{ tint: [1, 2] }, { tint: 3 }]) { try { r.setSelectionOverlay(o); } catch (e) { thrown += /tint must be/.test(e.message) ? 1 : 0; } }
    return thrown === 2 && calls.length === 0;
});
check("read_returns_what_the_addon_returns", () => {
    calls.length = 0;
    const o = r.readOverlay();
    return o.rgba instanceof Float32Array && o.cover instanceof Float32Array && o.rgba.length === W * H * 4 && o.cover.length === W * H &&
           o.rgba[5] === 0.25 && o.cover[5] === 0.5 && eq(calls, [["readOverlay", 1, W, H]]);
});
check("read_pixels_takes_the_overlay_flag", () => {
    calls.length = 0;
    const a = r.readPixels({ overlay: true });
    const mine = new Uint8Array(W * H * 4);
    const b = r.readPixels({ overlay: true, out: mine });
    const c = r.readPixels(), d = r.readPixels(mine), e = r.readPixels({ overlay: false });
    return a instanceof Uint8Array && a.length === W * H * 4 && a[0] === 7 && b === mine && c[0] === 3 && d === mine && e[0] === 3 &&
           eq(calls.map((x) => x[0]), ["readOverlayPixels", "readOverlayPixels", "readPixels", "readPixels", "readPixels"]);
});
check("open_delivery_switches_the_ring", () => {
    calls.length = 0;
    r.openDelivery(2, { overlay: true });
    r.closeDelivery();
    r.openDelivery(3);
    r.closeDelivery();
    r.openDelivery(2, { format: "nv12", overlay: true });
    return eq(calls.map((x) => x[0]), ["openDelivery", "deliverySetOverlay", "closeDelivery", "openDelivery", "closeDelivery", "openDeliveryEx", "deliverySetOverlay"]) &&
           eq(calls[1], ["deliverySetOverlay", 1, 1]);
});
check("addon_errors_pass_through", () => {
    const keep = stub.readOverlay;
    stub.readOverlay = () => { throw new Error("gsr_read_overlay failed (-1): gsr_read_overlay: no overlay options (gsr_set_overlay first)"); };
    let msg = "";
    try { r.readOverlay(); } catch (e) { msg = e.message; }
    stub.readOverlay = keep;
    return /no overlay options/.test(msg);
});
process.stdout.write(JSON.stringify({ checks, failed, calls: calls.length }));
