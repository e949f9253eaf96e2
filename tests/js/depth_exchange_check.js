#!/usr/bin/env node
// Driver used by tests/test_js_depth_exchange.py: depth in a group through the JavaScript host, in a world of one
// (joinGroup({ ..., depth }) / setGroupDepth, readFrameDepth, openDelivery(n, { depth }) in the group).
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

if (mode === "world1") {                   // world1 <splat> <out.json> <W> <H> <fx> <pose>
    const [file, out, W, H, fx, pose] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
    const res = {};
    try { r.setGroupDepth({ format: "u16" }); res.outsideRefused = false; } catch (e) { res.outsideRefused = /\(-1\)/.test(e.message); }
    const group = { id: G.HIPRenderer.createGroupId(), rank: 0, world: 1, edges: [[0, +W]] };
    r.joinGroup(Object.assign({ depth: { format: "u16", step: 2, near: 0.5 } }, group));
    for (const [name, depth, format] of [["u16_2_rgba8", { format: "u16", step: 2, near: 0.5 }, "rgba8"], ["f32_1_nv12", { format: "f32" }, "nv12"]]) {
        r.setGroupDepth(depth);
        r.openDelivery(2, { format, depth });
        r.renderAsync(scene, orbitCamera(+pose, +fx));     // in a group: the frame and its all-gather
        const f = r.acquireFrame(r.deliverFrame());
        const plane = r.readFrameDepth();
        res[name] = {
            frameDepthSha256: sha(plane), depthSha256: sha(f.depth), pixelsSha256: sha(f.pixels), kind: plane.constructor.name, samples: plane.length,
            ringKind: f.depth.constructor.name, layout: r.frameDepthLayout(), ringLayout: f.depthLayout,
        };
        f.release();
        r.closeDelivery();
    }
    try { r.openDelivery(2, { depth: { format: "u16", step: 2, near: 0.5 } }); res.mismatchRefused = false; } catch (e) { res.mismatchRefused = /\(-1\)/.test(e.message); }
    r.setGroupDepth(null);
    try { r.readFrameDepth(); res.offRefused = false; } catch (e) { res.offRefused = /\(-1\)/.test(e.message); }
    r.leaveGroup();
    r.dispose();
    fs.writeFileSync(out, JSON.stringify(res));
} else {
    console.error("usage: depth_exchange_check.js world1 ...");
    process.exit(2);
}
