#!/usr/bin/env node
// Driver of tests/test_gpu_share_scene_node.py: two HIPRenderers, the second created with { shareSceneWith: first }, render one
// Scene from one device copy.  Comparisons are bit for bit and made here, against an unshared renderer.
//   node share_scene_device_check.js   -> one JSON line { checks: [...names], failed: [...names] }
"use strict";
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
const W = 200, H = 120, FX = 180;
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
// counts through wrappers on the addon's methods (the renderers call them through the same module object)
const count = { sceneTransform: 0, setSceneArrays: 0, setScene: 0, shareScene: 0 };
for (const name of Object.keys(count)) {
    const fn = native[name];
    native[name] = function () { count[name]++; return fn.apply(this, arguments); };
}

const R = rows(5000, 13), s = new G.Scene(), free = new G.Scene();
s.setData(R); free.setData(R);
const a = new G.HIPRenderer({ width: W, height: H, throughput: true }, []);
const b = new G.HIPRenderer({ width: W, height: H, throughput: true, shareSceneWith: a }, []);
const cam = camera(9);
a.renderAsync(s, cam); b.renderAsync(s, camera(9));
a.sync(); b.sync();
check("second_renderer_shared_instead_of_uploading", count.setSceneArrays === 1 && count.setScene === 0 && count.shareScene === 1);
check("two_members_same_bytes", a.sceneSharing().members === 2 && b.sceneSharing().members === 2 &&
      a.sceneSharing().sceneBytes === b.sceneSharing().sceneBytes && a.sceneSharing().sceneBytes === 5000 * 60);
const unshared = new G.HIPRenderer({ width: W, height: H, throughput: true }, []);
unshared.render(free, camera(9));
const first = unshared.readPixels();
check("frames_equal_unshared_before_the_edit", first.some((v) => v !== 0) && same(a.readPixels(), first) && same(b.readPixels(), first));

const dq = G.Quaternion.FromEuler(new G.Vector3(0.1, -0.7, 0.3));
let events = 0;
s.addEventListener("change", () => events++);
count.sceneTransform = 0;
const uploads = count.setSceneArrays + count.setScene;
s.rotate(dq);
check("rotate_is_one_native_transform", count.sceneTransform === 1 && events === 1 && count.setSceneArrays + count.setScene === uploads);
const before = count.sceneTransform;
free.rotate(dq);                                // (the unshared renderer's own transform)
check("unshared_renderer_makes_its_own", count.sceneTransform === before + 1);
a.renderAsync(s, camera(9)); b.renderAsync(s, camera(9));
a.sync(); b.sync();
unshared.render(free, camera(9));
const second = unshared.readPixels();
check("frames_equal_unshared_after_the_rotate", !same(first, second) && same(a.readPixels(), second) && same(b.readPixels(), second));
check("orders_equal_unshared_after_the_rotate", same(a.lastDepthIndex(), unshared.lastDepthIndex()) && same(b.lastDepthIndex(), unshared.lastDepthIndex()));
s.limitBox(0, 100, -100, 100, -100, 100); free.limitBox(0, 100, -100, 100, -100, 100);
a.renderAsync(s, camera(30)); b.renderAsync(s, camera(30));
a.sync(); b.sync();
unshared.render(free, camera(30));
check("limitbox_reaches_both", s.vertexCount === free.vertexCount && s.vertexCount > 1000 && s.vertexCount < 4000 &&
      same(a.readPixels(), unshared.readPixels()) && same(b.readPixels(), unshared.readPixels()) && same(s.positions, free.positions));
// a "change" that makes the renderers upload (setData): one upload, by the first renderer; the second shares again
{
    const before = count.setSceneArrays + count.setScene, shares = count.shareScene, R2 = rows(4001, 17);
    s.setData(R2); free.setData(R2);
    const made = count.setSceneArrays + count.setScene - before;   // (one for `s`, one for the unshared renderer's `free`)
    a.renderAsync(s, camera(30)); b.renderAsync(s, camera(30));
    a.sync(); b.sync();
    unshared.render(free, camera(30));
    check("reupload_once_and_shared_again", made === 2 && count.shareScene === shares + 1 && a.sceneSharing().members === 2 &&
          b.sceneSharing().members === 2 && same(a.readPixels(), unshared.readPixels()) && same(b.readPixels(), unshared.readPixels()));
    count.sceneTransform = 0;
    s.rotate(dq); free.rotate(dq);
    check("one_transform_after_the_reupload", count.sceneTransform === 2);
}
a.dispose();
b.renderAsync(s, camera(31)); b.sync();
unshared.render(free, camera(31));
check("first_renderer_disposed_second_renders_on", b.sceneSharing().members === 1 && same(b.readPixels(), unshared.readPixels()));
b.dispose(); unshared.dispose();
console.log(JSON.stringify({ checks, failed }));
