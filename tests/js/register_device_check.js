#!/usr/bin/env node
// Driver of tests/test_gpu_match_node.py: matchScene / selectMatch / registerTo / rigidDecompose through the Node host, and
// Scene.rotate / Scene.translate applying the result to the device copy, on the rows the test wrote.
//   node register_device_check.js DIR   (DIR/source.bin, DIR/target.bin: .splat rows)  -> one JSON line { checks, failed, ... }
// Doubles travel as the decimal strings of their 64-bit patterns: JSON has no infinities and no NaN.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const W = 128, H = 96, RADIUS = 0.25, STEPS = 12;
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };
const bits = (a) => Array.from(new BigUint64Array(Float64Array.from(a).buffer), String);

const dir = process.argv[2];
const load = (name) => {
    const file = fs.readFileSync(path.join(dir, name));
    const rows = new Uint8Array(file.buffer, file.byteOffset, file.byteLength);
    const s = new G.Scene();
    s.setData(rows);
    return s;
};
const sa = load("source.bin"), sb = load("target.bin"), N = sa.vertexCount;
const ra = new G.HIPRenderer({ width: W, height: H }, []), rb = new G.HIPRenderer({ width: W, height: H }, []);
const cam = new G.Camera(undefined, undefined, 120, 120);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
ra.renderAsync(sa, cam); ra.sync();     // the scenes reach the device with their first frames
rb.renderAsync(sb, cam); rb.sync();

const m = ra.matchScene(rb, RADIUS, { sums: true });
check("the_match_has_the_types_and_the_sizes", m.idx instanceof Uint32Array && m.idx.length === N && m.d2 instanceof Float64Array && m.d2.length === N &&
      m.sums instanceof Float64Array && m.sums.length === 16 && m.pairs === m.matched && m.inScope === N && m.targetIndexed === sb.vertexCount);
check("unmatched_rows_hold_none_and_infinity", m.idx.every((j, i) => (j === 0xffffffff) === (m.d2[i] === Infinity)) && m.idx.filter((j) => j !== 0xffffffff).length === m.matched);
const has = ra.selectMatch(rb, RADIUS, { hi: RADIUS }), hasWords = Array.from(ra.readSelection());
const lacks = ra.selectMatch(rb, RADIUS, { lo: RADIUS });
check("has_and_lacks_cover_the_scene", has === m.matched && popcount(hasWords) === has && has + lacks === N);
const fit = ra.registerTo(rb, RADIUS, { maxIterations: STEPS, history: true });
check("the_registration_converged", fit.status === "converged" && fit.iterations <= STEPS && fit.transform instanceof Float64Array && fit.transform.length === 12 &&
      fit.stepPairs.length === fit.iterations && fit.stepRms.length === fit.iterations && fit.pairs === fit.stepPairs[fit.iterations - 1]);
const dec = ra.rigidDecompose(fit.transform);
check("rotation_and_translation_are_the_decomposition", fit.rotation instanceof G.Quaternion && fit.translation instanceof G.Vector3 &&
      JSON.stringify(dec.rotation.flat()) === JSON.stringify(fit.rotation.flat()) && dec.translation.x === fit.transform[3] && dec.translation.y === fit.transform[7] &&
      dec.translation.z === fit.transform[11] && fit.translation.x === dec.translation.x &&
      Math.abs(fit.rotation.x ** 2 + fit.rotation.y ** 2 + fit.rotation.z ** 2 + fit.rotation.w ** 2 - 1) < 1e-12);
const again = ra.matchScene(rb, RADIUS);
check("the_scene_was_not_written", JSON.stringify(Array.from(again.idx)) === JSON.stringify(Array.from(m.idx)));
sa.rotate(fit.rotation); sa.translate(fit.translation);     // on every device copy
const after = ra.matchScene(rb, 2 ** -17);
check("applied_once_the_partners_coincide", after.matched === fit.pairs);
let refused = 0;
try { ra.matchScene(rb, RADIUS, { budget: 1 }); } catch (e) { refused += /pair tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { ra.matchScene(rb, -1); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { ra.selectMatch(rb, RADIUS, { transform: [NaN, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] }); } catch (e) { refused += /must be finite/.test(e.message) ? 1 : 0; }
try { ra.registerTo(rb, RADIUS, { budget: 2 ** 39 }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
try { ra.registerTo(rb, RADIUS, { tolerance: -1 }); } catch (e) { refused += /tolerance/.test(e.message) ? 1 : 0; }
check("the_refusals_reach_the_caller", refused === 5);
ra.dispose(); rb.dispose();
console.log(JSON.stringify({ checks, failed, n: N, width: W, height: H, radius: RADIUS, steps: STEPS, idx: Array.from(m.idx), d2: bits(m.d2), sums: bits(m.sums), pairs: m.pairs,
                             info: [m.inScope, m.nonfinite, m.targetIndexed, m.matched, m.pairBound], d2MinMax: bits([m.d2Min, m.d2Max]), has, hasWords, lacks,
                             transform: bits(fit.transform), status: fit.status, iterations: fit.iterations, fitPairs: fit.pairs, rms: bits([fit.rms]),
                             stepPairs: Array.from(fit.stepPairs), stepRms: bits(fit.stepRms), q: bits(fit.rotation.flat()),
                             t: bits([fit.translation.x, fit.translation.y, fit.translation.z]), afterIdx: Array.from(after.idx), afterMatched: after.matched }));
