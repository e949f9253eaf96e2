#!/usr/bin/env node
// Driver of tests/test_gpu_normals_node.py: splatNormals / selectNormal through the Node host on the scenes the Python test wrote
// into DIR as raw little-endian rows (32 bytes per splat): cluster.bin and sphere.bin.
//   node normal_device_check.js DIR RADIUS_CLUSTER K_CLUSTER RADIUS_SPHERE K_SPHERE   -> one JSON line { checks, failed, scenes }
// f32 and f64 results travel as their bit patterns, so that the comparison is bit for bit.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const W = 128, H = 96;
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };
const bits = (a) => Array.from(new BigUint64Array(a.buffer, a.byteOffset, a.length), (v) => v.toString());
const bits32 = (a) => Array.from(new Uint32Array(a.buffer, a.byteOffset, a.length));

const dir = process.argv[2];
const r = new G.HIPRenderer({ width: W, height: H }, []);
const cam = new G.Camera(undefined, undefined, 120, 120);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
const scenes = {};
const toward = [0.3, -2, 0.7], up = [0.1, 1, -0.2];
for (const [name, radius, k] of [["cluster", Number(process.argv[3]), Number(process.argv[4])], ["sphere", Number(process.argv[5]), Number(process.argv[6])]]) {
    const R = new Uint8Array(fs.readFileSync(path.join(dir, name + ".bin"))), n = R.length / 32, s = new G.Scene();
    s.setData(R);
    r.renderAsync(s, cam); r.sync();     // the scene reaches the device with its first frame
    r.setHidden(null);
    const plain = r.splatNormals(radius, { k }), facing = r.splatNormals(radius, { k, toward }), own = r.splatNormals(undefined, { source: "own" });
    check(name + "_results_have_the_types_and_the_sizes", plain.normals instanceof Float32Array && plain.normals.length === 3 * n && plain.variation instanceof Float64Array &&
          plain.variation.length === n && plain.found instanceof Uint32Array && plain.found.length === n && plain.inScope === n && own.pairBound === 0);
    let valid = 0, faces = 0, firstPositive = 0;
    for (let i = 0; i < n; i++) {
        if (Number.isNaN(plain.variation[i])) continue;
        valid++;
        const a = plain.normals, f = facing.normals, p = 3 * i;
        firstPositive += (a[p] !== 0 ? a[p] : a[p + 1] !== 0 ? a[p + 1] : a[p + 2]) > 0 ? 1 : 0;
        faces += Math.abs(f[p]) === Math.abs(a[p]) && Math.abs(f[p + 1]) === Math.abs(a[p + 1]) && Math.abs(f[p + 2]) === Math.abs(a[p + 2]) ? 1 : 0;
    }
    check(name + "_valid_rows_are_counted_and_oriented", valid === plain.valid && firstPositive === valid && faces === valid && facing.valid === valid);
    // the consistency guarantee, on this host's own arrays
    let walls = 0, flat = 0;
    const mid = (plain.variationMin + plain.variationMax) / 2;
    for (let i = 0; i < n; i++) {
        const a = plain.normals, p = 3 * i, v = Math.abs((a[p] * up[0] + a[p + 1] * up[1]) + a[p + 2] * up[2]);
        walls += v >= 0 && v <= 0.25 ? 1 : 0;
        flat += plain.variation[i] >= 0 && plain.variation[i] <= mid ? 1 : 0;
    }
    const wallsSelected = r.selectNormal("abs_dot", { radius, k, axis: up, hi: 0.25 }), wallWords = Array.from(r.readSelection());
    const flatSelected = r.selectNormal("variation", { radius, k, lo: 0, hi: mid, op: "intersect" }), flatWords = Array.from(r.readSelection());
    check(name + "_the_picker_is_the_rule_on_the_returned_arrays", wallsSelected === walls && popcount(wallWords) === walls && flatSelected <= Math.min(walls, flat) &&
          popcount(flatWords) === flatSelected);
    const hidden = new Uint32Array(Math.ceil(n / 32));
    for (let i = 0; i < n; i += 5) hidden[i >>> 5] |= 1 << (i & 31);
    r.setHidden(hidden);
    const vis = r.splatNormals(radius, { k, scope: "visible" });
    const ownSelected = r.selectNormal("dot", { source: "own", axis: up, lo: 0, scope: ["visible"], op: "add" }), ownWords = Array.from(r.readSelection());
    check(name + "_a_hidden_splat_has_no_normal", vis.inScope === n - Math.ceil(n / 5) && Number.isNaN(vis.variation[0]) && Number.isNaN(vis.normals[0]) && vis.found[0] === 0);
    scenes[name] = { n, radius, k, normals: bits32(plain.normals), variation: bits(plain.variation), found: Array.from(plain.found), facing: bits32(facing.normals),
                     own: bits32(own.normals), ownVariation: bits(own.variation),
                     info: [plain.inScope, plain.nonfinite, plain.pairBound, plain.valid, own.valid], range: bits(new Float64Array([plain.variationMin, plain.variationMax])),
                     walls: wallsSelected, wallWords, flat: flatSelected, flatWords, visNormals: bits32(vis.normals), visFound: Array.from(vis.found),
                     ownSelected, ownWords };
}
let refused = 0;
try { r.splatNormals(0.15, { budget: 1 }); } catch (e) { refused += /pair tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { r.splatNormals(0); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { r.selectNormal("variation", { radius: 0.15, budget: 2 ** 39 }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
try { r.selectNormal("dot", { radius: 0.15, axis: [0, 0, 0] }); } catch (e) { refused += /axis is zero/.test(e.message) ? 1 : 0; }
check("the_library_refusals_reach_the_caller", refused === 4);
r.dispose();
console.log(JSON.stringify({ checks, failed, width: W, height: H, scenes }));
