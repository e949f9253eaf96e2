#!/usr/bin/env node
// Driver of tests/test_gpu_knn_node.py: splatKnn / selectKnn / selectStatisticalOutliers through the Node host on the scenes the
// Python test wrote into DIR as raw little-endian rows (32 bytes per splat): cluster.bin and coincident.bin.
//   node knn_device_check.js DIR RADIUS_CLUSTER K_CLUSTER RADIUS_COINCIDENT K_COINCIDENT   -> one JSON line { checks, failed, scenes }
// f64 results travel as their 64-bit patterns (decimal strings), so that the comparison is bit for bit.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const W = 128, H = 96;
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };
const sum = (a) => { let t = 0; for (const v of a) t += v; return t; };
const bits = (a) => Array.from(new BigUint64Array(a.buffer, a.byteOffset, a.length), (v) => v.toString());

const dir = process.argv[2];
const r = new G.HIPRenderer({ width: W, height: H }, []);
const cam = new G.Camera(undefined, undefined, 120, 120);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
const scenes = {};
for (const [name, radius, k] of [["cluster", Number(process.argv[3]), Number(process.argv[4])], ["coincident", Number(process.argv[5]), Number(process.argv[6])]]) {
    const R = new Uint8Array(fs.readFileSync(path.join(dir, name + ".bin"))), n = R.length / 32, s = new G.Scene();
    s.setData(R);
    r.renderAsync(s, cam); r.sync();     // the scene reaches the device with its first frame
    r.setHidden(null);
    const mean = r.splatKnn(radius, { k, lists: true }), kth = r.splatKnn(radius, { k, stat: "kth" });
    check(name + "_results_have_the_types_and_the_sizes", mean.found instanceof Uint32Array && mean.found.length === n && mean.values instanceof Float64Array &&
          mean.values.length === n && mean.hist.length === k + 1 && mean.idx instanceof Uint32Array && mean.idx.length === n * k && mean.d2 instanceof Float64Array &&
          mean.d2.length === n * k && kth.idx === undefined && kth.d2 === undefined);
    check(name + "_the_histogram_sums_to_the_scope", sum(mean.hist) === mean.inScope && mean.inScope === n && kth.complete === mean.hist[k]);
    const everything = r.selectKnn(radius, { k, stat: "kth" });
    const full = r.selectKnn(radius, { k, stat: "kth", hi: 1e300 }), fullWords = Array.from(r.readSelection());
    check(name + "_infinite_values_follow_the_upper_end", everything === n && full === kth.complete && popcount(fullWords) === full);
    const hidden = new Uint32Array(Math.ceil(n / 32));
    for (let i = 0; i < n; i += 5) hidden[i >>> 5] |= 1 << (i & 31);
    r.setHidden(hidden);
    const vis = r.splatKnn(radius, { k, scope: "visible" });
    const out = r.selectStatisticalOutliers(radius, { k, stdRatio: 1.5, scope: ["visible"], op: "add" }), outWords = Array.from(r.readSelection());
    let atOrAbove = 0;
    for (let i = 0; i < n; i++) atOrAbove += vis.values[i] >= out.threshold && !(fullWords[i >>> 5] >>> (i & 31) & 1) ? 1 : 0;
    check(name + "_outliers_are_the_values_at_or_above_the_threshold", out.selected === full + atOrAbove && popcount(outWords) === out.selected);
    scenes[name] = { n, radius, k, found: Array.from(mean.found), idx: Array.from(mean.idx), d2: bits(mean.d2), mean: bits(mean.values), kth: bits(kth.values),
                     hist: Array.from(mean.hist), info: [mean.inScope, mean.nonfinite, mean.pairBound, mean.complete, mean.finiteValues],
                     range: bits(new Float64Array([mean.valueMin, mean.valueMax, kth.valueMin, kth.valueMax])), full, fullWords, visFound: Array.from(vis.found),
                     visMean: bits(vis.values), threshold: bits(new Float64Array([out.threshold]))[0], outliers: out.selected, outWords };
}
let refused = 0;
try { r.splatKnn(0.15, { budget: 1 }); } catch (e) { refused += /pair tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { r.splatKnn(0); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { r.selectKnn(0.15, { budget: 2 ** 39 }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
check("the_library_refusals_reach_the_caller", refused === 3);
r.dispose();
console.log(JSON.stringify({ checks, failed, width: W, height: H, scenes }));
