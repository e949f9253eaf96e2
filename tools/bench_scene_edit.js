#!/usr/bin/env node
"use strict";
// Wall time of an edit per frame through the reference's Scene API -- scene.rotate(q); renderer.render(scene, camera) and
// scene.scale(s); renderer.render(scene, camera) -- with the scene attached (the edit runs as a kernel on the renderer's
// context, nothing is uploaded) against the host path in the same process (the JavaScript loop over all splats and a full
// upload, forced by a host-only device scene beside the renderer), and the cost of one refresh of the Scene's arrays.
//   node tools/bench_scene_edit.js <splats> [iterations] [W] [H] [fx] [--sh]
// prints one JSON line.  --sh: the scene carries degree-3 SH on every splat and scene.shFollowsTransforms is on, so the per-frame
// edits keep the SH frame up and render through it; and limitBox (a box that keeps every splat: the whole scene and, with the
// option on, 96 bytes of SH per splat move) is timed with the option on and, on a second scene, off.  The scene is seeded noise in a 6-unit cube (.splat rows from a generator of its own).
const path = require("path");
const G = require(path.join(__dirname, "..", "gsplat.js_amd", "js"));
const withSh = process.argv.includes("--sh");
const [nArg, itArg, W, H, fx] = process.argv.slice(2).filter((v) => v !== "--sh");
const n = +(nArg || 1000000), iters = +(itArg || 20), width = +(W || 1920), height = +(H || 1080), focal = +(fx || 1132);
const now = () => Number(process.hrtime.bigint()) * 1e-6;   // ms

function rows(count, seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const out = new Uint8Array(32 * count), f = new Float32Array(out.buffer);
    for (let i = 0; i < count; i++) {
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 6; f[8 * i + 3 + k] = 0.004 + rnd() * 0.02; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const cam = new G.Camera(undefined, undefined, focal, focal);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
const half = Math.PI / 360, dq = new G.Quaternion(0, Math.sin(half), 0, Math.cos(half));
const up = new G.Vector3(1.001, 1.001, 1.001), down = new G.Vector3(1 / 1.001, 1 / 1.001, 1 / 1.001);

function shScene(follow) {     // every splat degree 3; small seeded coefficients
    const s = new G.Scene();
    if (!withSh) { s.setData(rows(n, 5)); return s; }
    const shs = new Float32Array(48 * n);
    let v = 12345;
    for (let i = 0; i < shs.length; i++) { v = (Math.imul(v, 1664525) + 1013904223) >>> 0; shs[i] = (v / 4294967296 - 0.5) * 0.5; }
    s.bandsIndices = new Int32Array([-1, -1, -1]);
    s.setData(rows(n, 5), shs);
    s.shFollowsTransforms = follow;
    return s;
}
// limitBox that keeps everything, attached: ms per call (the call waits for its count)
function limitBoxMs(follow) {
    const s = shScene(follow), rr = new G.HIPRenderer({ width, height }, []);
    rr.render(s, cam);
    const count = Math.max(3, Math.min(iters, 10));
    s.limitBox(-100, 100, -100, 100, -100, 100);
    const t = now();
    for (let k = 0; k < count; k++) s.limitBox(-100, 100, -100, 100, -100, 100);
    const ms = (now() - t) / count;
    const kept = s.vertexCount, shKept = s.shHeight > 0 && !s.shDroppedOnDevice;
    rr.dispose();
    return { ms, kept, shKept };
}
const scene = shScene(true);
const r = new G.HIPRenderer({ width, height }, []);
const perFrame = (edit, count) => {
    for (let k = 0; k < 2; k++) { edit(k); r.render(scene, cam); }
    const t0 = now();
    for (let k = 0; k < count; k++) { edit(k); r.render(scene, cam); }
    return (now() - t0) / count;
};
r.render(scene, cam);
const frameMs = perFrame(() => {}, iters);
const attachedRotate = perFrame(() => scene.rotate(dq), iters);
const attachedScale = perFrame((k) => scene.scale(k & 1 ? down : up), iters);
scene.rotate(dq);
let t0 = now();
const words = scene.data.length;                     // one refresh of all four arrays
const refreshMs = now() - t0;
// the host path: a host-only device scene beside the renderer sends every edit through the JavaScript loop and the upload
const hostOnly = { hostOnly: true };
scene.attachDevice(hostOnly);
const hostIters = Math.max(2, Math.min(iters, Math.ceil(4e6 / Math.max(n, 1))));
const hostRotate = perFrame(() => scene.rotate(dq), hostIters);
const hostScale = perFrame((k) => scene.scale(k & 1 ? down : up), hostIters);
scene.detachDevice(hostOnly);
const info = r.deviceInfo ? r.deviceInfo() : null;
r.dispose();
const boxOn = withSh ? limitBoxMs(true) : null, boxOff = withSh ? limitBoxMs(false) : null;
console.log(JSON.stringify({
    caller: "Node (tools/bench_scene_edit.js)", splats: n, width, height, iterations: iters, host_iterations: hostIters,
    ms_per_frame_no_edit: +frameMs.toFixed(4),
    ms_per_rotate_and_frame_attached: +attachedRotate.toFixed(4), ms_per_rotate_and_frame_host: +hostRotate.toFixed(3),
    ms_per_scale_and_frame_attached: +attachedScale.toFixed(4), ms_per_scale_and_frame_host: +hostScale.toFixed(3),
    speedup_rotate: +(hostRotate / attachedRotate).toFixed(1), speedup_scale: +(hostScale / attachedScale).toFixed(1),
    ms_mirror_refresh: +refreshMs.toFixed(3), data_words: words, device: info, sh: withSh,
    ms_per_limit_box_sh_follow_on: boxOn ? +boxOn.ms.toFixed(4) : undefined, ms_per_limit_box_sh_follow_off: boxOff ? +boxOff.ms.toFixed(4) : undefined,
    limit_box_kept: boxOn ? boxOn.kept : undefined, limit_box_sh_kept_on: boxOn ? boxOn.shKept : undefined, limit_box_sh_kept_off: boxOff ? boxOff.shKept : undefined,
}));
