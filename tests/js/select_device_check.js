#!/usr/bin/env node
// Driver of tests/test_gpu_select_node.py: selectRegion -> readSelection -> Scene.eraseSelection through the Node host, on two
// HIPRenderers that share one device copy of a Scene and a third with a copy of its own.
//   node select_device_check.js DIR   -> one JSON line { checks: [...names], failed: [...names], ... }
// and in DIR, as raw little-endian files, what the Python host needs to do the same: rows.bin, camera.bin (view, proj, viewProj as
// f32[16] each, then fx, fy), words.bin (the selection), after_{data,positions,rotations,scales}.bin (the Scene's mirrors).
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
const count = { setSelection: 0, eraseSelected: 0, setSceneArrays: 0, setScene: 0 };
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
const cam = camera(9);
for (const r of [a, b, own]) { r.renderAsync(s, camera(9)); r.sync(); }
check("two_share_one_has_its_own", a.sceneSharing().members === 2 && b.sceneSharing().members === 2 && own.sceneSharing().members === 1);

// a lasso: the disc of radius 40 about (100, 60), as bytes with rows longer than the rectangle is wide
const rect = { x0: 60, y0: 20, x1: 140, y1: 100, stride: 83 };
rect.mask = new Uint8Array(80 * rect.stride).fill(9);
for (let y = 0; y < 80; y++) for (let x = 0; x < 80; x++) rect.mask[y * rect.stride + x] = (x + 0.5 - 40) ** 2 + (y + 0.5 - 40) ** 2 <= 1600 ? 1 : 0;
const picked = a.selectRegion(rect, { mode: "centre" });
const words = a.readSelection();
check("select_region_counts_its_words", picked > 0 && picked < N && words.length === Math.ceil(N / 32) && popcount(words) === picked);
check("members_have_one_selection", same(b.readSelection(), words) && popcount(own.readSelection()) === 0);
check("own_copy_selects_the_same", own.selectRegion(rect) === picked && same(own.readSelection(), words));
const surface = b.selectRegion({ x0: 60, y0: 20, x1: 140, y1: 100 }, { mode: "hit", op: "intersect" });
const index = b.readDepth().index, hits = new Set();
for (let y = 20; y < 100; y++) for (let x = 60; x < 140; x++) if (index[y * W + x] !== 0xffffffff) hits.add(index[y * W + x]);
let both = 0;
for (const i of hits) if ((words[i >>> 5] >>> (i & 31)) & 1) both++;
check("hit_intersects_through_the_other_member", surface === both && surface > 0 && surface < picked && popcount(a.readSelection()) === surface);
check("ops_and_invert", a.invertSelection() === N - surface && a.setSelection(words, "replace") === picked && a.selectBox([-100, 100, -100, 100, -100, 100], { op: "subtract" }) === 0 &&
      a.setSelection(null, "add") === 0 && popcount(b.readSelection()) === 0);

const before = { data: Uint32Array.from(s.data), positions: Float32Array.from(s.positions), rotations: Float32Array.from(s.rotations), scales: Float32Array.from(s.scales) };
let events = 0, deviceEdits = 0;
s.addEventListener("change", () => { events++; if (s.deviceEditApplied) deviceEdits++; });
const uploads = count.setSceneArrays + count.setScene;
count.setSelection = count.eraseSelected = 0;
s.eraseSelection(words);
check("erase_once_per_device_copy", count.setSelection === 2 && count.eraseSelected === 2 && events === 1 && deviceEdits === 1 &&
      count.setSceneArrays + count.setScene === uploads);
check("count_follows", s.vertexCount === N - picked && popcount(a.readSelection()) === 0 && a.readSelection().length === Math.ceil((N - picked) / 32));
let ok = true, j = 0;
const after = { data: s.data, positions: s.positions, rotations: s.rotations, scales: s.scales };
for (let i = 0; i < N && ok; i++) {
    if ((words[i >>> 5] >>> (i & 31)) & 1) continue;
    for (let w = 0; w < 8 && ok; w++) ok = after.data[8 * j + w] === before.data[8 * i + w];
    for (let w = 0; w < 3 && ok; w++) ok = Object.is(after.positions[3 * j + w], before.positions[3 * i + w]) && Object.is(after.scales[3 * j + w], before.scales[3 * i + w]);
    for (let w = 0; w < 4 && ok; w++) ok = Object.is(after.rotations[4 * j + w], before.rotations[4 * i + w]);
    j++;
}
check("mirrors_are_the_kept_splats_in_order", ok && j === s.vertexCount);
// every renderer renders the compacted scene: equal to a renderer that is given it fresh
const free = new G.Scene();
free.setData(R);
free.eraseSelection(words);                      // (unbound: the host loop)
const fresh = new G.HIPRenderer({ width: W, height: H }, []);
fresh.render(free, camera(30));
for (const r of [a, b, own]) { r.renderAsync(s, camera(30)); r.sync(); }
check("host_loop_equals_the_devices", same(free.positions, s.positions) && same(free.data.subarray(0, 8 * s.vertexCount), s.data.subarray(0, 8 * s.vertexCount)));
check("frames_equal_a_fresh_renderer", fresh.readPixels().some((v) => v !== 0) && [a, b, own].every((r) => same(r.readPixels(), fresh.readPixels()) && same(r.lastDepthIndex(), fresh.lastDepthIndex())));
if (dir) {
    const put = (name, arr) => fs.writeFileSync(path.join(dir, name), Buffer.from(arr.buffer, arr.byteOffset, arr.byteLength));
    cam.update(W, H);
    const c = new Float32Array(50);
    c.set(cam.viewMatrix.buffer, 0); c.set(cam.projectionMatrix.buffer, 16); c.set(cam.viewProj.buffer, 32); c[48] = cam.fx; c[49] = cam.fy;
    put("rows.bin", R); put("camera.bin", c); put("words.bin", words);
    const n = s.vertexCount;
    put("after_data.bin", after.data.subarray(0, 8 * n)); put("after_positions.bin", after.positions); put("after_rotations.bin", after.rotations); put("after_scales.bin", after.scales);
}
for (const r of [a, b, own, fresh]) r.dispose();
console.log(JSON.stringify({ checks, failed, picked, width: W, height: H, rect: [rect.x0, rect.y0, rect.x1, rect.y1], stride: rect.stride }));
