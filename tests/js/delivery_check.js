#!/usr/bin/env node
// Driver used by tests/test_js_delivery.py: the JavaScript host's frame delivery (openDelivery / deliverFrame / acquireFrame).
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const [, , mode, ...a] = process.argv;

function orbitCamera(k, fx) {
    const cam = new G.Camera(undefined, undefined, fx, fx);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const same = (x, y) => x.length === y.length && Buffer.compare(Buffer.from(x.buffer, x.byteOffset, x.byteLength), Buffer.from(y.buffer, y.byteOffset, y.byteLength)) === 0;

if (mode === "surface") {                  // the delivery methods of a renderer, read off the class source without constructing one
    const src = fs.readFileSync(path.join(__dirname, "..", "..", "gsplat.js_amd", "js", "renderers", "HIPRenderer.js"), "utf8");
    const names = ["openDelivery", "closeDelivery", "deliverFrame", "frameReady", "acquireFrame"];
    console.log(JSON.stringify({ exported: typeof G.WebGLRenderer === "function" && G.WebGLRenderer === G.HIPRenderer,
                                 methods: names.filter((n) => new RegExp("this\\." + n + "\\s*=").test(src)) }));
} else if (mode === "deliver") {           // deliver <splat> <out.json> <W> <H> <fx>
    const [file, out, W, H, fx] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
    const res = { frames: 0, equal: true, sameBuffer: true, serials: [] };
    r.openDelivery(3);
    const want = new Uint8Array(+W * +H * 4);
    const buffers = new Map();             // slot identity: the ArrayBuffer behind every view ever handed out
    let first = null;
    // one at a time: the delivered frame against readPixels(out) of the same frame; three laps of the ring
    for (let k = 0; k < 9; k++) {
        r.renderAsync(scene, orbitCamera(7 * k, +fx));
        const s = r.deliverFrame();
        const f = r.acquireFrame(s);
        r.readPixels(want);
        res.equal = res.equal && f.serial === s && same(f.pixels, want);
        const slot = k % 3;
        if (buffers.has(slot)) res.sameBuffer = res.sameBuffer && buffers.get(slot) === f.pixels.buffer;
        else buffers.set(slot, f.pixels.buffer);
        if (!first) first = f.pixels;
        res.serials.push(s);
        f.release();
        res.frames++;
    }
    res.distinctBuffers = new Set(buffers.values()).size;
    // pipelined: three frames enqueued before the first is picked up
    const poses = [3, 33, 63, 93, 13, 43], pending = [], got = [];
    for (const k of poses) {
        if (pending.length === 3) { const f = r.acquireFrame(pending.shift()); got.push(Uint8Array.from(f.pixels)); f.release(); }
        r.renderAsync(scene, orbitCamera(k, +fx));
        pending.push(r.deliverFrame());
    }
    while (pending.length) { const f = r.acquireFrame(); res.oldestFirst = (res.oldestFirst !== false) && f.serial === pending.shift(); got.push(Uint8Array.from(f.pixels)); f.release(); }
    poses.forEach((k, i) => { r.render(scene, orbitCamera(k, +fx)); r.readPixels(want); res.equal = res.equal && same(got[i], want); });
    // a full ring throws and the renderer stays usable; a held frame blocks setSize / closeDelivery
    const hold = [];
    for (let k = 0; k < 3; k++) { r.renderAsync(scene, orbitCamera(k, +fx)); hold.push(r.acquireFrame(r.deliverFrame())); }
    try { r.deliverFrame(); res.busy = false; } catch (e) { res.busy = /\(-7\)/.test(e.message); }
    try { r.setSize(320, 240); res.resizeRefused = false; } catch (e) { res.resizeRefused = true; }
    try { r.closeDelivery(); res.closeRefused = false; } catch (e) { res.closeRefused = true; }
    hold.forEach((f) => f.release());
    // an idle ring follows setSize: new blocks, the old views are detached
    const old = first;
    r.setSize(322, 241);
    res.detachedAfterResize = old.length === 0 && old.buffer.byteLength === 0;
    r.renderAsync(scene, orbitCamera(5, +fx / 2));
    const f2 = r.acquireFrame(r.deliverFrame());
    const want2 = r.readPixels();
    res.resized = f2.pixels.length === 322 * 241 * 4 && same(f2.pixels, want2) && want2.some((v) => v !== 0);
    const keep = f2.pixels;
    f2.release();
    r.renderAsync(scene, orbitCamera(6, +fx / 2)); r.deliverFrame();   // a copy in flight
    r.dispose();
    res.detachedAfterDispose = keep.length === 0;
    let sum = 0; for (let i = 0; i < keep.length; i++) sum += keep[i];   // reading a detached view touches no memory
    res.safeRead = sum === 0;
    fs.writeFileSync(out, JSON.stringify(res));
} else if (mode === "group") {             // group <splat> <out.json> <W> <H> <fx>: renderAsync + deliverFrame after joinGroup (one rank)
    const [file, out, W, H, fx] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
    r.joinGroup({ id: G.WebGLRenderer.createGroupId(), rank: 0, world: 1, edges: [[0, +W]] });
    r.openDelivery(2);
    const ref = new G.WebGLRenderer({ width: +W, height: +H }, []);
    const res = { equal: true, frames: 0 };
    const pending = [];
    const poses = [4, 44, 84, 24];
    const got = [];
    for (const k of poses) {
        if (pending.length === 2) { const f = r.acquireFrame(pending.shift()); got.push(Uint8Array.from(f.pixels)); f.release(); }
        r.renderAsync(scene, orbitCamera(k, +fx));
        pending.push(r.deliverFrame());
    }
    while (pending.length) { const f = r.acquireFrame(pending.shift()); got.push(Uint8Array.from(f.pixels)); f.release(); }
    res.equalsReadFrame = same(got[got.length - 1], r.readPixels());
    poses.forEach((k, i) => { ref.render(scene, orbitCamera(k, +fx)); res.equal = res.equal && same(got[i], ref.readPixels()); res.frames++; });
    r.dispose(); ref.dispose();
    fs.writeFileSync(out, JSON.stringify(res));
} else {
    console.error("unknown mode " + mode);
    process.exit(2);
}
