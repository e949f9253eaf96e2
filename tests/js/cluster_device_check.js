#!/usr/bin/env node
// Driver of tests/test_gpu_clusters_node.py: splatClusters / selectClusters / selectClusterAt through the Node host on a seeded scene.
//   node cluster_device_check.js DIR   -> one JSON line { checks, failed, ... }
// and in DIR, as a raw little-endian file, what the Python host needs to do the same: rows.bin.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
function rows(n, seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const out = new Uint8Array(32 * n), f = new Float32Array(out.buffer);
    for (let i = 0; i < n; i++) {
        const wide = i % 16 === 0 ? 12 : 1.5;      // one splat in sixteen is scattered far out: islands of one
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * wide; f[8 * i + 3 + k] = 0.02 + rnd() * 0.1; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 128, H = 96, N = 3001, RADIUS = 0.1, MIN_PTS = 3, NONE = 0xffffffff;
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };
const countIf = (a, f) => { let c = 0; for (let i = 0; i < a.length; i++) if (f(a[i], i)) c++; return c; };

const dir = process.argv[2];
const R = rows(N, 41), s = new G.Scene();
s.setData(R);
const r = new G.HIPRenderer({ width: W, height: H }, []);
const cam = new G.Camera(undefined, undefined, 120, 120);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
r.renderAsync(s, cam); r.sync();     // the scene reaches the device with its first frame
const hidden = new Uint32Array(Math.ceil(N / 32));
for (let i = 0; i < N; i += 5) hidden[i >>> 5] |= 1 << (i & 31);
r.setHidden(hidden);
const all = r.splatClusters(RADIUS, { minPts: MIN_PTS }), vis = r.splatClusters(RADIUS, { minPts: MIN_PTS, scope: "visible" }), cc = r.splatClusters(RADIUS);
check("results_have_the_types_and_the_sizes", all.labels instanceof Uint32Array && all.labels.length === N && all.sizes instanceof Uint32Array && all.sizes.length === N);
check("the_kinds_sum_to_the_scope", all.inScope === N && all.core + all.border + all.noise === N && vis.inScope === N - popcount(hidden) &&
      vis.core + vis.border + vis.noise === vis.inScope && countIf(all.labels, (l) => l === NONE) === all.noise && cc.noise === 0 && cc.border === 0 && cc.core === N);
const small = r.selectClusters(RADIUS, { below: 10, minPts: MIN_PTS }), words = Array.from(r.readSelection());
check("what_the_sizes_show_is_what_the_range_selects", small === countIf(all.sizes, (v) => v < 10) && popcount(words) === small);
const largest = r.selectClusterAt(RADIUS, { largest: true, minPts: MIN_PTS }), largestWords = Array.from(r.readSelection());
check("the_largest_cluster_has_its_size", largest === all.largestSize && largest === countIf(all.labels, (l) => l === all.largestLabel));
let seed = 0;
while (all.labels[seed] === NONE || all.labels[seed] === all.largestLabel) seed++;
const at = r.selectClusterAt(RADIUS, { seed, minPts: MIN_PTS, op: "add" });
check("ops_fold_like_the_selection_calls", at === largest + all.sizes[seed]);
let refused = 0;
try { r.splatClusters(RADIUS, { budget: 1 }); } catch (e) { refused += /pair tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { r.splatClusters(0); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { r.selectClusterAt(RADIUS, { seed: N }); } catch (e) { refused += /seed/.test(e.message) ? 1 : 0; }
check("the_library_refusals_reach_the_caller", refused === 3 && popcount(r.readSelection()) === at);
if (dir) fs.writeFileSync(path.join(dir, "rows.bin"), bytes(R));
r.dispose();
console.log(JSON.stringify({ checks, failed, n: N, width: W, height: H, radius: RADIUS, minPts: MIN_PTS, labels: Array.from(all.labels), sizes: Array.from(all.sizes),
                             visLabels: Array.from(vis.labels), visSizes: Array.from(vis.sizes),
                             info: [all.inScope, all.nonfinite, all.pairBound, all.core, all.border, all.noise, all.clusters, all.largestLabel, all.largestSize],
                             small, words, largest, largestWords, seed, at }));
