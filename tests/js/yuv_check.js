#!/usr/bin/env node
// Driver used by tests/test_js_yuv_delivery.py: the JavaScript host's Y'CbCr delivery (openDelivery(slots, { format, ... })).
"use strict";
const crypto = require("crypto");
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const [, , mode, ...a] = process.argv;

function orbitCamera(k, fx) {
    const cam = new G.Camera(undefined, undefined, fx, fx);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const sha = (x) => crypto.createHash("sha256").update(Buffer.from(x.buffer, x.byteOffset, x.byteLength)).digest("hex");

if (mode === "payload") {                  // payload <splat> <out.json> <W> <H> <fx> <pose>
    const [file, out, W, H, fx, pose] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
    const res = {};
    for (const [name, options] of [["nv12", { format: "nv12" }], ["i420", { format: "i420" }],
                                   ["nv12_full_bg", { format: "nv12", fullRange: true, background: [255, 128, 7] }]]) {
        r.openDelivery(2, options);
        const layout = r.deliveryLayout();
        r.renderAsync(scene, orbitCamera(+pose, +fx));
        const f = r.acquireFrame(r.deliverFrame());
        res[name] = {
            sha256: sha(f.pixels), bytes: f.pixels.length, format: f.format, layout,
            planes: f.planes.map((p) => ({ offset: p.byteOffset, length: p.length, stride: p.stride, rows: p.rows, sameBuffer: p.buffer === f.pixels.buffer })),
            planesCoverPayload: Buffer.concat(f.planes.map((p) => Buffer.from(p.buffer, p.byteOffset, p.byteLength))).equals(Buffer.from(f.pixels.buffer, 0, f.pixels.length)),
        };
        f.release();
        r.closeDelivery();
    }
    r.openDelivery(2);                     // and the ring as it was: RGBA8, one plane
    r.renderAsync(scene, orbitCamera(+pose, +fx));
    const f = r.acquireFrame(r.deliverFrame());
    const want = new Uint8Array(+W * +H * 4);
    r.readPixels(want);
    res.rgba8 = { format: f.format, planes: f.planes.length, stride: f.planes[0].stride, equal: sha(f.pixels) === sha(want) && sha(f.planes[0]) === sha(want) };
    f.release();
    try { r.openDelivery(2, { format: "yuv9" }); res.unknownRefused = false; } catch (e) { res.unknownRefused = true; }
    try { r.openDelivery(2, { format: "nv12" }); res.openWhileOpenRefused = false; } catch (e) { res.openWhileOpenRefused = /\(-1\)/.test(e.message); }
    r.dispose();
    fs.writeFileSync(out, JSON.stringify(res));
} else {
    console.error("usage: yuv_check.js payload ...");
    process.exit(2);
}
