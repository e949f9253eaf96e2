#!/usr/bin/env node
// Driver of tests/test_gpu_outline_node.py: setSelectionOverlay -> setSelection -> render -> setSelectionOutline -> readOverlay /
// readPixels({ overlay: true }) -> a delivered overlay frame, through the Node host.
//   node outline_device_check.js DIR   -> one JSON line { checks, failed, sha256, ... }
// and in DIR, as raw little-endian files, what the Python host needs to do the same: rows.bin, cameras.bin (view, proj, viewProj
// as f32[16] each, then fx, fy), selection.bin (the selection words).
"use strict";
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
function rows(n, seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const out = new Uint8Array(32 * n), f = new Float32Array(out.buffer);
    for (let i = 0; i < n; i++) {
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 6; f[8 * i + 3 + k] = 0.02 + rnd() * 0.2; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 200, H = 120, FX = 180, N = 5000, POSE = 9, TINT = [1, 0.5, 0], MIX = 0.5;
const OUTLINE = { color: [0.125, 7, -3], alpha: 0.5, threshold: 0.25, width: 3, side: "inner" };
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const same = (a, b) => a.length === b.length && Buffer.compare(bytes(a), bytes(b)) === 0;
const sha = (...arrays) => { const h = crypto.createHash("sha256"); for (const a of arrays) h.update(bytes(a)); return h.digest("hex"); };

const dir = process.argv[2];
const R = rows(N, 13), s = new G.Scene();
s.setData(R);
const r = new G.HIPRenderer({ width: W, height: H }, []);
const cam = camera(POSE);
r.renderAsync(s, cam); r.sync();
let refused = false;
try { r.setSelectionOutline(OUTLINE); } catch (e) { refused = /no overlay options/.test(e.message); }
check("without_overlay_options_it_is_refused", refused);
r.setSelectionOverlay({ tint: TINT, mix: MIX });
const words = new Uint32Array(Math.ceil(N / 32));
for (let i = 0; i < N; i += 3) words[i >> 5] |= 1 << (i & 31);
const selected = r.setSelection(words);
const plain = r.readOverlay();
r.setSelectionOutline(OUTLINE);
const o = r.readOverlay();
let edge = 0, inside = true;
for (let p = 0; p < W * H; p++) {
    let differs = false;
    for (let k = 0; k < 4; k++) differs = differs || !Object.is(o.rgba[4 * p + k], plain.rgba[4 * p + k]);
    if (differs) { edge++; if (!(plain.cover[p] >= OUTLINE.threshold)) inside = false; }
}
check("an_inner_outline_changes_some_inside_pixels_and_no_other", edge > 0 && edge < W * H / 2 && inside);
check("cover_is_not_changed", same(o.cover, plain.cover));
let bad = false;
try { r.setSelectionOutline({ width: 17 }); } catch (e) { bad = /width must be in 1 .. 16/.test(e.message); }
check("a_bad_width_is_refused_by_the_library", bad && same(r.readOverlay().rgba, o.rgba));
const px = r.readPixels({ overlay: true });
r.openDelivery(2, { overlay: true });
r.renderAsync(s, cam);
const serial = r.deliverFrame();
const f = r.acquireFrame(serial);
const delivered = Uint8Array.from(f.pixels);
check("a_delivered_frame_carries_the_outline", same(delivered, px));
f.release();
r.closeDelivery();
r.setSelectionOutline(null);
check("null_switches_it_off", same(r.readOverlay().rgba, plain.rgba));
if (dir) {
    cam.update(W, H);
    const cams = new Float32Array(50);
    cams.set(cam.viewMatrix.buffer, 0); cams.set(cam.projectionMatrix.buffer, 16); cams.set(cam.viewProj.buffer, 32);
    cams[48] = cam.fx; cams[49] = cam.fy;
    fs.writeFileSync(path.join(dir, "rows.bin"), bytes(R));
    fs.writeFileSync(path.join(dir, "cameras.bin"), bytes(cams));
    fs.writeFileSync(path.join(dir, "selection.bin"), bytes(words));
}
r.dispose();
console.log(JSON.stringify({ checks, failed, sha256: sha(o.rgba, o.cover), sha256_rgba8: sha(px), sha256_delivered: sha(delivered), selected, edge, width: W, height: H,
                             tint: TINT, mix: MIX, outline: OUTLINE }));
