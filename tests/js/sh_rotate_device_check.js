#!/usr/bin/env node
// Driver of tests/test_gpu_sh_rotate_node.py: an SH scene attached to a real renderer, its coefficients rotated through
// renderer.rotateSH / rotateSelection(q, { sh: true }) / bakeSHFrame.  After every step: SHA-256 of the Scene's shs_rgb mirrors (marked
// stale by the call, read back from the device on this read) and of the device copy's four arrays.  The Python host, given the same
// input and the same walk, must hold the same bytes.
//   node sh_rotate_device_check.js <rows> <shs> <W> <H> <band0> <band1> <band2>   -> one JSON line { steps: [...] }
"use strict";
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));
const native = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js", "native", "gsplat_hip.node"));

const a = process.argv.slice(2);
const [W, H, b0, b1, b2] = a.slice(2).map(Number);
const bytes = fs.readFileSync(a[0]), shBytes = fs.readFileSync(a[1]);
const rows = new Uint8Array(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.length));
const shs = new Float32Array(shBytes.buffer.slice(shBytes.byteOffset, shBytes.byteOffset + shBytes.length));
const sha = (t) => crypto.createHash("sha256").update(Buffer.from(t.buffer, t.byteOffset, t.byteLength)).digest("hex");
const throws = (f, word) => { try { f(); } catch (e) { return String(e.message).includes(word); } return false; };

const QUAT = [0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214], QUAT2 = [-0.5, 0.5, 0.5, 0.5];
const QUAT3 = [0.6, 0.0, -1.6, 0.4], PIVOT = [0.25, -0.5, 0.125];
const cam = new G.Camera(new G.Vector3(0, 0, -6), new G.Quaternion(0, 0, 0, 1), 40, 40);   // (no trigonometry: the same bits on every host)

const scene = new G.Scene();
scene.bandsIndices = new Int32Array([b0, b1, b2]);
scene.setData(rows, shs);
const n = scene.vertexCount;
const mask = new Uint32Array(Math.ceil(n / 32));
for (let i = 0; i < n; i++) if ((7 * i + 3) % 10 < 3) mask[i >>> 5] |= 1 << (i & 31);
const r = new G.HIPRenderer({ width: W, height: H }, []);
r.render(scene, cam);

const geometry = () => {
    const data = new Uint32Array(8 * n), pos = new Float32Array(3 * n), rot = new Float32Array(4 * n), scl = new Float32Array(3 * n);
    native.readSceneArrays(r._h, data, pos, rot, scl);
    return [data, pos, rot, scl].map(sha);
};
const steps = [];
const keep = (name, extra) => steps.push(Object.assign({ name, shs_rgb: scene.shs_rgb.map(sha), shHeight: scene.shHeight, geometry: geometry() }, extra || {}));

keep("start");
keep("all", { rows: r.rotateSH(QUAT) });
r.setSelection(mask);
keep("selected", { rows: r.rotateSH(new G.Quaternion(QUAT2[0], QUAT2[1], QUAT2[2], QUAT2[3]), { selected: true }) });
r.rotateSelection(QUAT3, { pivot: PIVOT, sh: true });
keep("selection_with_sh");
r.rotateSelection(new Float64Array(QUAT2), { sh: true });
keep("selection_with_sh_no_pivot");
r.rotateSelection(QUAT, { pivot: PIVOT });                 // sh defaults to false: today's path, the coefficients stay
keep("selection_without_sh");
scene.shFollowsTransforms = true;
scene.rotate(new G.Quaternion(QUAT[0], QUAT[1], QUAT[2], QUAT[3]));          // (a device edit: the context keeps the frame)
r.setSelection(mask);
keep("refused", { refused: throws(() => r.rotateSelection(QUAT2, { pivot: PIVOT, sh: true }), "gsr_scene_bake_sh_frame"), shFrame: Array.from(scene.shFrame) });
const q = r.bakeSHFrame();
keep("baked", { q: [q.x, q.y, q.z, q.w], shFrame: Array.from(scene.shFrame) });
r.rotateSelection(QUAT2, { pivot: PIVOT, sh: true });
keep("selection_with_sh_after_the_bake");
r.render(scene, cam);
const out = { steps, pixels: sha(r.readPixels()), drawn: r.readPixels().some((v, k) => (k & 3) === 3 && v !== 0) };
r.dispose();
console.log(JSON.stringify(out));
