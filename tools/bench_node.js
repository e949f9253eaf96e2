#!/usr/bin/env node
"use strict";
// Frames per second through the JavaScript host -- the reference's own calling convention, renderer.render(scene, camera)
// (WebGLRenderer.ts:241-296), one synchronous frame after the other -- and with three renderers used round-robin
// (renderAsync / sync, what bench.py's default measures through ctypes).  The scene is a .splat file (32-byte rows);
// scripts/final_lines.sh writes the synthetic C3 scene with the Python generator first.
//   node tools/bench_node.js <scene.splat> <W> <H> <fx> [frames] [warmup]
// prints one JSON line.
const path = require("path");
const G = require(path.join(__dirname, "..", "gsplat.js_amd", "js"));
const [file, W, H, fx, framesArg, warmArg] = process.argv.slice(2);
const frames = framesArg ? +framesArg : 240, warm = warmArg ? +warmArg : 20;

function orbitCamera(k) {
    const cam = new G.Camera(undefined, undefined, +fx, +fx);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * (k % 120)) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const now = () => Number(process.hrtime.bigint()) * 1e-6;   // ms

const scene = new G.Scene();
G.Loader.LoadSync(file, scene);
const cams = [];
for (let k = 0; k < 120; k++) cams.push(orbitCamera(k));

// (1) the reference's contract: render() returns when the frame is done
const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
for (let k = 0; k < warm; k++) r.render(scene, cams[k % 120]);
let t0 = now();
for (let k = 0; k < frames; k++) r.render(scene, cams[(warm + k) % 120]);
const syncMs = (now() - t0) / frames;
// with the pixels read back as RGBA8 every frame (what a consumer without a display does)
t0 = now();
let sink = 0;
const nread = Math.min(frames, 120);
for (let k = 0; k < nread; k++) { r.render(scene, cams[k % 120]); sink += r.readPixels()[1]; }
const readMs = (now() - t0) / nread;
const pixels = new Uint8Array(+W * +H * 4);   // reused, like the destination of gl.readPixels
r.render(scene, cams[0]); r.readPixels(pixels);
t0 = now();
for (let k = 0; k < nread; k++) { r.render(scene, cams[k % 120]); sink += r.readPixels(pixels)[1]; }
const readReuseMs = (now() - t0) / nread;
r.dispose();

// (2) three renderers, frames in flight
const rs = [0, 1, 2].map(() => new G.WebGLRenderer({ width: +W, height: +H, throughput: true }, []));
for (let k = 0; k < warm; k++) rs[k % 3].renderAsync(scene, cams[k % 120]);
rs.forEach((x) => x.sync());
t0 = now();
for (let k = 0; k < frames; k++) rs[k % 3].renderAsync(scene, cams[(warm + k) % 120]);
rs.forEach((x) => x.sync());
const asyncMs = (now() - t0) / frames;
const info = rs[0].deviceInfo ? rs[0].deviceInfo() : null;
rs.forEach((x) => x.dispose());

// (3) every frame delivered to the host as RGBA8 through the library's pinned ring (openDelivery(3) / deliverFrame /
// acquireFrame): `pixels` views the slot, nothing is allocated or copied per frame; a renderer's oldest frame is picked up
// when its ring is full.  One default renderer, then three throughput renderers with a ring each.
function delivered(renderers, count) {
    const pending = renderers.map(() => []);
    const pickUp = (c) => { const f = renderers[c].acquireFrame(pending[c].shift()); sink += f.pixels[1]; f.release(); };
    const t = now();
    for (let k = 0; k < count; k++) {
        const c = k % renderers.length;
        if (pending[c].length === 3) pickUp(c);
        renderers[c].renderAsync(scene, cams[(warm + k) % 120]);
        pending[c].push(renderers[c].deliverFrame());
    }
    for (let c = 0; c < renderers.length; c++) while (pending[c].length) pickUp(c);
    return (now() - t) / count;
}
const d1 = new G.WebGLRenderer({ width: +W, height: +H }, []);
d1.openDelivery(3);
delivered([d1], warm);
const deliver1Ms = delivered([d1], frames);
// the last delivered frame against readPixels() of the same pose
d1.renderAsync(scene, cams[5]);
const last = d1.acquireFrame(d1.deliverFrame());
d1.readPixels(pixels);
const deliveredEqual = Buffer.compare(Buffer.from(last.pixels.buffer, last.pixels.byteOffset, last.pixels.byteLength), Buffer.from(pixels.buffer)) === 0;
last.release();
d1.dispose();
const d3 = [0, 1, 2].map(() => new G.WebGLRenderer({ width: +W, height: +H, throughput: true }, []));
d3.forEach((x) => x.openDelivery(3));
delivered(d3, warm);
const deliver3Ms = delivered(d3, frames);
d3.forEach((x) => x.dispose());

console.log(JSON.stringify({
    host: "node " + process.version + ", gsplat.js_amd/js (N-API addon over libgsplat_hip.so)",
    scene: path.basename(file), splats: scene.vertexCount, width: +W, height: +H, frames: frames, warmup: warm,
    render_sync: { frames_per_sec: 1000 / syncMs, ms_per_frame: syncMs, note: "renderer.render(scene, camera), one frame at a time" },
    render_sync_with_readPixels: { frames_per_sec: 1000 / readMs, ms_per_frame: readMs, note: "fresh Uint8Array per frame" },
    render_sync_with_readPixels_reused_array: { frames_per_sec: 1000 / readReuseMs, ms_per_frame: readReuseMs },
    render_async_3_renderers: { frames_per_sec: 1000 / asyncMs, ms_per_frame: asyncMs },
    render_async_deliver: { frames_per_sec: 1000 / deliver1Ms, ms_per_frame: deliver1Ms, slots: 3, delivered_equals_readPixels: deliveredEqual,
                            note: "one renderer; every frame acquired as a Uint8Array view of its pinned slot, no allocation per frame" },
    render_async_deliver_3_renderers: { frames_per_sec: 1000 / deliver3Ms, ms_per_frame: deliver3Ms, slots: 3 },
    device: info, sink: sink & 1,
}));
