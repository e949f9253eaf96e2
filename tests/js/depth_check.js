#!/usr/bin/env node
// Driver used by tests/test_js_depth.py: the JavaScript host's depth planes and picking (readDepth / pick / setHitAlpha).
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

if (mode === "surface") {                  // the depth methods of a renderer, read off the class source without constructing one
    const src = fs.readFileSync(path.join(__dirname, "..", "..", "gsplat.js_amd", "js", "renderers", "HIPRenderer.js"), "utf8");
    const names = ["setHitAlpha", "depthAsync", "readDepth", "pick"];
    console.log(JSON.stringify({ methods: names.filter((n) => new RegExp("this\\." + n + "\\s*=").test(src)) }));
} else if (mode === "planes") {            // planes <splat> <out.json> <W> <H> <fx> <pose> <x,y;x,y;...>
    const [file, out, W, H, fx, pose, pts] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: +W, height: +H }, []);
    r.render(scene, orbitCamera(+pose, +fx));
    const np = +W * +H;
    const mine = { mean: new Float32Array(np), hit: new Float32Array(np), index: new Uint32Array(np) };
    const back = r.readDepth(mine);        // the caller's arrays, filled
    const fresh = r.readDepth();
    const res = { filled: back === mine && sha(fresh.index) === sha(mine.index), mean: sha(mine.mean), hit: sha(mine.hit), index: sha(mine.index), picks: [] };
    const only = r.readDepth({ index: new Uint32Array(np) });
    res.partial = only.mean === undefined && sha(only.index) === res.index;
    const bits = new Float32Array(1), u = new Uint32Array(bits.buffer);
    for (const p of pts.split(";")) {
        const [x, y] = p.split(",").map(Number);
        const k = r.pick(x, y);
        const word = (v) => { bits[0] = v; return u[0]; };
        res.picks.push([k.index, word(k.depth), word(k.mean), word(k.alpha), k.point === null]);
    }
    try { r.pick(-1, 0); res.refused = false; } catch (e) { res.refused = /\(-1\)/.test(e.message); }
    try { r.setHitAlpha(0); res.alphaRefused = false; } catch (e) { res.alphaRefused = /\(-1\)/.test(e.message); }
    r.dispose();
    fs.writeFileSync(out, JSON.stringify(res));
} else if (mode === "point") {             // point <splat> <out.json>: one opaque splat at the orbit target, an odd-sized image
    const [file, out] = a;
    const scene = new G.Scene();
    G.Loader.LoadSync(file, scene);
    const r = new G.WebGLRenderer({ width: 641, height: 481 }, []);
    const res = [];
    for (const k of [0, 17, 50]) {
        r.render(scene, orbitCamera(k, 1132));
        const p = r.pick(320, 240);          // the image centre is the centre of this pixel
        res.push({ index: p.index, depth: p.depth, alpha: p.alpha, point: p.point && p.point.flat() });
    }
    const none = r.pick(0, 0);
    res.push({ index: none.index, depth: none.depth === Infinity, point: none.point });
    r.dispose();
    fs.writeFileSync(out, JSON.stringify(res));
} else {
    console.error("usage: depth_check.js surface | planes ... | point ...");
    process.exit(2);
}
