#!/usr/bin/env node
// Driver of tests/test_gpu_neighbours_node.py: splatNeighbours / selectNeighbours through the Node host on a seeded scene.
//   node neighbour_device_check.js DIR   -> one JSON line { checks, failed, ... }
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
        const wide = i % 16 === 0 ? 12 : 1.5;      // one splat in sixteen is scattered far out: the floaters
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * wide; f[8 * i + 3 + k] = 0.02 + rnd() * 0.1; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 128, H = 96, N = 3001, RADIUS = 0.15, CAP = 8;
const bytes = (a) => Buffer.from(a.buffer, a.byteOffset, a.byteLength);
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };
const sum = (a, from, to) => { let t = 0; for (let k = from; k < to; k++) t += a[k]; return t; };

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
const all = r.splatNeighbours(RADIUS, { cap: CAP }), vis = r.splatNeighbours(RADIUS, { cap: CAP, scope: "visible" });
check("results_have_the_types_and_the_sizes", all.counts instanceof Uint32Array && all.counts.length === N && all.hist instanceof Uint32Array && all.hist.length === CAP + 1);
check("the_histogram_sums_to_the_scope", sum(all.hist, 0, CAP + 1) === all.inScope && all.inScope === N && sum(vis.hist, 0, CAP + 1) === vis.inScope && vis.inScope === N - popcount(hidden));
const few = r.selectNeighbours(RADIUS, { below: 3, cap: CAP }), words = Array.from(r.readSelection());
check("what_the_histogram_shows_is_what_the_range_selects", few === sum(all.hist, 0, 3) && popcount(words) === few);
const added = r.selectNeighbours(RADIUS, { lo: CAP, cap: CAP, op: "add", scope: ["visible"] });
check("ops_fold_like_the_selection_calls", added === few + vis.hist[CAP]);
let refused = 0;
try { r.splatNeighbours(RADIUS, { cap: CAP, budget: 1 }); } catch (e) { refused += /pair tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { r.splatNeighbours(0); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { r.selectNeighbours(RADIUS, { budget: 2 ** 39 }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
check("the_library_refusals_reach_the_caller", refused === 3 && popcount(r.readSelection()) === added);
if (dir) fs.writeFileSync(path.join(dir, "rows.bin"), bytes(R));
r.dispose();
console.log(JSON.stringify({ checks, failed, n: N, width: W, height: H, radius: RADIUS, cap: CAP, counts: Array.from(all.counts), hist: Array.from(all.hist),
                             visCounts: Array.from(vis.counts), visHist: Array.from(vis.hist), info: [all.inScope, all.nonfinite, all.pairBound], few, words, added }));
