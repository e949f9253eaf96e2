#!/usr/bin/env node
// Driver used by tests/test_js_depth_delivery.py: the JavaScript host's depth ring (openDelivery(slots, { format, depth: { format, step, near } })).
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

if (mode === "planes") {                   // planes <splat> <out.json> <W> <H> <fx> <pose>
    const [file, out, W, H, fx, pose] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
    const res = {};
    for (const [name, options] of [["u16_2_nv12", { format: "nv12", depth: { format: "u16", step: 2, near: 0.5 } }],
                                   ["f32_1_rgba8", { depth: { format: "f32" } }],
                                   ["u16_1_i420", { format: "i420", depth: {} }]]) {
        r.openDelivery(2, options);
        r.renderAsync(scene, orbitCamera(+pose, +fx));
        const f = r.acquireFrame(r.deliverFrame());
        res[name] = {
            depthSha256: sha(f.depth), pixelsSha256: sha(f.pixels), samples: f.depth.length, kind: f.depth.constructor.name,
            depthLayout: f.depthLayout, sameLayout: JSON.stringify(f.depthLayout) === JSON.stringify(r.depthLayout()),
            offset: f.depth.byteOffset, sameBuffer: f.depth.buffer === f.pixels.buffer, pixelBytes: f.pixels.length, layoutBytes: r.deliveryLayout().bytes,
        };
        f.release();
        r.closeDelivery();
    }
    r.openDelivery(2, { format: "nv12" });  // a ring without depth: no plane, no layout
    r.renderAsync(scene, orbitCamera(+pose, +fx));
    const f = r.acquireFrame(r.deliverFrame());
    res.plain = { depth: f.depth === undefined, depthLayout: f.depthLayout === undefined, wholeBuffer: f.pixels.length === f.pixels.buffer.byteLength };
    try { r.depthLayout(); res.plain.layoutRefused = false; } catch (e) { res.plain.layoutRefused = /\(-1\)/.test(e.message); }
    f.release();
    r.closeDelivery();
    try { r.openDelivery(2, { depth: { format: "u8" } }); res.unknownRefused = false; } catch (e) { res.unknownRefused = true; }
    try { r.openDelivery(2, { depth: { step: 4 } }); res.stepRefused = false; } catch (e) { res.stepRefused = /\(-1\)/.test(e.message); }
    r.dispose();
    fs.writeFileSync(out, JSON.stringify(res));
} else {
    console.error("usage: depth_delivery_check.js planes ...");
    process.exit(2);
}
