#!/usr/bin/env node
// Driver of tests/test_gpu_contrib_node.py: resetContribution -> render / accumulateContribution over two poses -> readContribution
// -> selectContribution through the Node host.
//   node contrib_device_check.js DIR   -> one JSON line { checks, failed, frames, sha256, selected, ... }
// and in DIR, as raw little-endian files, what the Python host needs to do the same: rows.bin, cameras.bin (per pose view, proj,
// viewProj as f32[16] each, then fx, fy).
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
        // (spread far beyond what the cameras see from 8 units away: many splats are off screen or behind the camera in both poses)
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 24; f[8 * i + 3 + k] = 0.02 + rnd() * 0.2; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 200, H = 120, FX = 180, N = 5000, POSES = [9, 47];
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };

const dir = process.argv[2];
const R = rows(N, 13), s = new G.Scene();
s.setData(R);
const r = new G.HIPRenderer({ width: W, height: H }, []);
let refused = false;
r.renderAsync(s, camera(POSES[0])); r.sync();
try { r.selectContribution({ stat: "pixels", below: 1 }); } catch (e) { refused = /frames == 0/.test(e.message); }
check("an_empty_tour_is_refused", refused);
r.resetContribution();
const cams = new Float32Array(50 * POSES.length);
POSES.forEach((k, j) => {
    const cam = camera(k);
    r.renderAsync(s, cam); r.sync();
    r.accumulateContribution();
    cam.update(W, H);
    cams.set(cam.viewMatrix.buffer, 50 * j); cams.set(cam.projectionMatrix.buffer, 50 * j + 16); cams.set(cam.viewProj.buffer, 50 * j + 32);
    cams[50 * j + 48] = cam.fx; cams[50 * j + 49] = cam.fy;
});
const c = r.readContribution();
check("arrays_have_the_types_and_the_count", c.weight instanceof BigUint64Array && c.peak instanceof Float32Array && c.pixels instanceof Uint32Array &&
      c.weight.length === N && c.peak.length === N && c.pixels.length === N && c.frames === POSES.length);
let shown = 0, consistent = true;
for (let i = 0; i < N; i++) {
    if (c.pixels[i]) shown++;
    if (c.pixels[i] === 0 && !(c.weight[i] === 0n && c.peak[i] === 0)) consistent = false;
}
check("some_splats_show_and_some_never_do", shown > 0 && shown < N && consistent);
const sha256 = crypto.createHash("sha256").update(bytes(c.weight)).update(bytes(c.peak)).update(bytes(c.pixels)).digest("hex");
const never = r.selectContribution({ stat: "pixels", below: 1 });
check("never_shown_is_selected", never === N - shown && popcount(r.readSelection()) === never);
let heavy = 0;
for (let i = 0; i < N; i++) if (Number(c.weight[i]) / 16777216 < 2.5) heavy++;
const light = r.selectContribution({ stat: "weight", below: 2.5, op: "replace" });
check("weight_threshold_matches_the_arrays", light === heavy && light > never);
const faint = r.selectContribution({ stat: "peak", below: 0.05, op: "intersect" });
let both = 0;
for (let i = 0; i < N; i++) if (Number(c.weight[i]) / 16777216 < 2.5 && c.peak[i] < 0.05) both++;
check("ops_fold_like_the_selection_calls", faint === both);
if (dir) {
    fs.writeFileSync(path.join(dir, "rows.bin"), bytes(R));
    fs.writeFileSync(path.join(dir, "cameras.bin"), bytes(cams));
}
r.dispose();
console.log(JSON.stringify({ checks, failed, frames: c.frames, sha256, never, light, faint, width: W, height: H, poses: POSES.length }));
