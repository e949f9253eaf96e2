#!/usr/bin/env node
// Driver of tests/test_gpu_sh_follow.py::test_node_host_equals_the_python_host: an SH scene with shFollowsTransforms on a real
// renderer, rotated and cropped through the Scene API, once before its first frame (the edits run in JavaScript, the upload hands
// textures, thresholds and frame to the context) and once attached (the edits run as kernels, shs_rgb / bandsIndices are read
// back from the context).  Prints one JSON line of SHA-256 digests; the Python host's must equal them.
//   node sh_follow_device_check.js <rows> <shs> <W> <H> <fx> <band0> <band1> <band2> <qx> <qy> <qz> <qw> <box x 6>
"use strict";
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const a = process.argv.slice(2);
const [rowsFile, shsFile] = a, num = a.slice(2).map(Number);
const [W, H, fx, b0, b1, b2, qx, qy, qz, qw, ...box] = num;
const bytes = fs.readFileSync(rowsFile), shBytes = fs.readFileSync(shsFile);
const rows = new Uint8Array(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.length));
const shs = new Float32Array(shBytes.buffer.slice(shBytes.byteOffset, shBytes.byteOffset + shBytes.length));
const sha = (t) => crypto.createHash("sha256").update(Buffer.from(t.buffer, t.byteOffset, t.byteLength)).digest("hex");
const cam = new G.Camera(new G.Vector3(0, 0, -6), new G.Quaternion(0, 0, 0, 1), fx, fx);   // (no trigonometry: the same bits on every host)
const q = new G.Quaternion(qx, qy, qz, qw);

function run(attachFirst) {
    const scene = new G.Scene();
    scene.bandsIndices = new Int32Array([b0, b1, b2]);
    scene.setData(rows, shs);
    const r = new G.HIPRenderer({ width: W, height: H }, []);
    if (attachFirst) r.render(scene, cam);
    scene.shFollowsTransforms = true;
    scene.rotate(q);
    scene.limitBox(box[0], box[1], box[2], box[3], box[4], box[5]);
    r.render(scene, cam);
    const out = { pixels: sha(r.readPixels()), shs_rgb: scene.shs_rgb.map(sha), bandsIndices: Array.from(scene.bandsIndices), shHeight: scene.shHeight,
                  vertexCount: scene.vertexCount, shFrame: Array.from(scene.shFrame), shDroppedOnDevice: scene.shDroppedOnDevice };
    // a change the caller dispatches: mirrors are read back, everything is uploaded again with the frame, and the frame is the same
    scene.dispatchEvent({ type: "change" });
    r.render(scene, cam);
    out.pixelsAfterUpload = sha(r.readPixels());
    r.dispose();
    return out;
}
console.log(JSON.stringify({ hostPath: run(false), devicePath: run(true) }));
