#!/usr/bin/env node
// Driver of tests/test_gpu_hide_node.py: selectRegion -> hideSelection -> readHidden -> readPixels through the Node host, and
// Scene.setHidden on two HIPRenderers with separate device copies of one Scene (and a third that shares the first's copy).
//   node hide_device_check.js DIR   -> one JSON line { checks: [...names], failed: [...names], ... }
// and in DIR, as raw little-endian files, what the Python host needs to do the same: rows.bin, camera.bin (view, proj, viewProj as
// f32[16] each, then fx, fy), hidden.bin (the hidden words), pixels_hidden.bin and pixels_shown.bin (RGBA8 frames).
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));
const native = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js", "native", "gsplat_hip.node"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const same = (a, b) => {
    if (a.length !== b.length) return false;
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false;
    return true;
};
const throws = (f) => { try { f(); } catch (e) { return true; } return false; };
function rows(n, seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const out = new Uint8Array(32 * n), f = new Float32Array(out.buffer);
    for (let i = 0; i < n; i++) {
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 5; f[8 * i + 3 + k] = 0.01 + rnd() * 0.08; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 200, H = 120, FX = 180, N = 5000;
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const count = { setHidden: 0, setSceneArrays: 0, setScene: 0 };
for (const name of Object.keys(count)) {
    const fn = native[name];
    native[name] = function () { count[name]++; return fn.apply(this, arguments); };
}
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };

const dir = process.argv[2];
const R = rows(N, 13), s = new G.Scene();
s.setData(R);
const a = new G.HIPRenderer({ width: W, height: H }, []);
const b = new G.HIPRenderer({ width: W, height: H, throughput: true, shareSceneWith: a }, []);
const own = new G.HIPRenderer({ width: W, height: H }, []);
for (const r of [a, b, own]) { r.renderAsync(s, camera(9)); r.sync(); }
const shown = Uint8Array.from(a.readPixels());
check("nothing_hidden_at_first", popcount(a.readHidden()) === 0 && a.readHidden().length === Math.ceil(N / 32));

// hide what a rectangle's "select through" picks
const rect = { x0: 60, y0: 20, x1: 140, y1: 100 };
const picked = a.selectRegion(rect, { mode: "centre" });
const hiddenCount = a.hideSelection();
const hidden = a.readHidden();
check("hide_selection_hides_the_selection", picked > 0 && picked < N && hiddenCount === picked && same(hidden, a.readSelection()));
check("members_have_one_hidden_set", same(b.readHidden(), hidden) && popcount(own.readHidden()) === 0);
check("a_change_is_a_scene_edit", throws(() => a.pick(100, 60)));
a.renderAsync(s, camera(9)); a.sync();
const pixelsHidden = Uint8Array.from(a.readPixels());
check("the_hidden_frame_differs", !same(pixelsHidden, shown) && pixelsHidden.some((v) => v !== 0));
const index = a.readDepth().index;
let seen = 0, through = true;
for (const i of index) if (i !== 0xffffffff) { seen++; if ((hidden[i >>> 5] >>> (i & 31)) & 1) through = false; }
check("depth_sees_through", seen > 0 && through);
check("select_hidden_is_a_picker", a.selectHidden() === picked && same(a.readSelection(), hidden) && a.selectHidden({ op: "subtract" }) === 0);
check("ops", a.setHidden(hidden, { op: "subtract" }) === 0 && a.setHidden(hidden) === picked && a.setHidden(null, { op: "intersect" }) === 0 &&
      a.setHidden(hidden, { op: "add" }) === picked);
b.renderAsync(s, camera(9)); b.sync();
check("the_other_member_renders_the_hidden_frame", same(b.readPixels(), pixelsHidden));
check("show_all", a.showAll() === 0 && popcount(b.readHidden()) === 0);
a.renderAsync(s, camera(9)); a.sync();
check("shown_again_bit_for_bit", same(a.readPixels(), shown));

// Scene.setHidden: once per device copy, no upload, no "change"
let events = 0;
s.addEventListener("change", () => { events++; });
const uploads = count.setSceneArrays + count.setScene;
count.setHidden = 0;
const viaScene = s.setHidden(hidden);
check("scene_set_hidden_once_per_device_copy", count.setHidden === 2 && viaScene === picked && events === 0 && count.setSceneArrays + count.setScene === uploads);
check("reaches_both_copies", same(a.readHidden(), hidden) && same(own.readHidden(), hidden));
for (const r of [a, b, own]) { r.renderAsync(s, camera(9)); r.sync(); }
check("both_copies_render_the_hidden_frame", [a, b, own].every((r) => same(r.readPixels(), pixelsHidden)));
check("scene_show_all", s.setHidden(null) === 0 && popcount(own.readHidden()) === 0 && popcount(a.readHidden()) === 0);
if (dir) {
    const put = (name, arr) => fs.writeFileSync(path.join(dir, name), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
    const cam = camera(9);
    cam.update(W, H);
    const c = new Float32Array(50);
    c.set(cam.viewMatrix.buffer, 0); c.set(cam.projectionMatrix.buffer, 16); c.set(cam.viewProj.buffer, 32); c[48] = cam.fx; c[49] = cam.fy;
    put("rows.bin", R); put("camera.bin", c); put("hidden.bin", hidden); put("pixels_hidden.bin", pixelsHidden); put("pixels_shown.bin", shown);
}
for (const r of [a, b, own]) r.dispose();
console.log(JSON.stringify({ checks, failed, picked, width: W, height: H, rect: [rect.x0, rect.y0, rect.x1, rect.y1] }));
