#!/usr/bin/env node
// Driver of tests/test_gpu_surface_node.py: registerTo with residual "surface", matchSurface and SPLAT.surfaceSolve through the Node
// host, on the rows the test wrote.
//   node surface_device_check.js DIR   (DIR/source.bin, DIR/target.bin: .splat rows)  -> one JSON line { checks, failed, ... }
// Doubles travel as the decimal strings of their 64-bit patterns: JSON has no infinities and no NaN.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const W = 128, H = 96, RADIUS = 0.25, STEPS = 16, TOLERANCE = 2 ** -30, KNN = { source: "knn", k: 8, radius: 0.15 };
const bits = (a) => Array.from(new BigUint64Array(Float64Array.from(a).buffer), String);
const same = (a, b) => JSON.stringify(bits(a)) === JSON.stringify(bits(b));

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

const before = ra.matchScene(rb, RADIUS);
const today = ra.registerTo(rb, RADIUS, { maxIterations: STEPS, tolerance: TOLERANCE, history: true });
const point = ra.registerTo(rb, RADIUS, { residual: "point", maxIterations: STEPS, tolerance: TOLERANCE, history: true });
check("residual_point_is_the_call_without_it", same(today.transform, point.transform) && today.status === point.status && today.iterations === point.iterations &&
      same(today.stepRms, point.stepRms) && point.surfacePairs === undefined);
const fit = ra.registerTo(rb, RADIUS, { residual: "surface", normals: { source: "own" }, maxIterations: STEPS, tolerance: TOLERANCE, history: true });
check("the_surface_registration_converged_in_fewer_steps", fit.status === "converged" && fit.iterations < STEPS && fit.transform instanceof Float64Array &&
      fit.transform.length === 12 && ["stepPairs", "stepSurfacePairs", "stepRms", "stepSurfaceRms"].every((k) => fit[k] instanceof Float64Array && fit[k].length === fit.iterations) &&
      fit.surfacePairs === fit.stepSurfacePairs[fit.iterations - 1] && fit.valid === sb.vertexCount && (point.status !== "converged" || fit.iterations < point.iterations));
const dec = ra.rigidDecompose(fit.transform);
check("rotation_and_translation_are_the_decomposition", fit.rotation instanceof G.Quaternion && fit.translation instanceof G.Vector3 &&
      JSON.stringify(dec.rotation.flat()) === JSON.stringify(fit.rotation.flat()) && fit.translation.x === fit.transform[3] && fit.translation.y === fit.transform[7] &&
      fit.translation.z === fit.transform[11]);
const plain = ra.registerTo(rb, RADIUS, { residual: "surface", maxIterations: STEPS, tolerance: TOLERANCE });
check("own_normals_are_the_default_and_the_same_call_gives_the_same_bits", same(plain.transform, fit.transform) && plain.stepPairs === undefined);
const knn = ra.registerTo(rb, RADIUS, { residual: "surface", normals: KNN, maxIterations: STEPS, tolerance: TOLERANCE, history: true });
check("knn_normals_converge_too", knn.status === "converged" && knn.valid > 0);
const ms = ra.matchSurface(rb, RADIUS, { normals: { source: "own" } });
check("one_step_as_data", ms.sums instanceof Float64Array && ms.sums.length === 29 && ms.pairs === ms.matched && ms.surfacePairs === fit.stepSurfacePairs[0] && ms.inScope === N);
const solved = G.surfaceSolve(ms);
const composed = ra.registerTo(rb, RADIUS, { residual: "surface", maxIterations: 1, tolerance: TOLERANCE });
check("the_pure_solve_is_the_first_step", solved.degenerate === 0 && same(solved.transform, composed.transform) && same([solved.rms], [fit.stepSurfaceRms[0]]));
const again = ra.matchScene(rb, RADIUS);
check("the_scene_was_not_written", JSON.stringify(Array.from(again.idx)) === JSON.stringify(Array.from(before.idx)) && again.matched === ms.matched);
let refused = 0;
try { ra.registerTo(rb, RADIUS, { residual: "surface", budget: 1 }); } catch (e) { refused += /pair tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { ra.registerTo(rb, -1, { residual: "surface" }); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { ra.matchSurface(rb, RADIUS, { normals: { source: "knn", radius: 1e-200, k: 8 } }); } catch (e) { refused += /radius/.test(e.message) ? 1 : 0; }
try { ra.matchSurface(rb, RADIUS, { normals: { budget: 2 ** 39 } }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
try { G.surfaceSolve({ surfacePairs: 5, sums: ms.sums }); } catch (e) { refused += /at least 6/.test(e.message) ? 1 : 0; }
check("the_refusals_reach_the_caller", refused === 5);
ra.dispose(); rb.dispose();
console.log(JSON.stringify({ checks, failed, n: N, width: W, height: H, radius: RADIUS, steps: STEPS, knn: KNN,
                             pointTransform: bits(point.transform), pointStatus: point.status, pointIterations: point.iterations,
                             transform: bits(fit.transform), status: fit.status, iterations: fit.iterations, pairs: fit.pairs, surfacePairs: fit.surfacePairs, valid: fit.valid,
                             rms: bits([fit.rms, fit.surfaceRms, fit.delta]), stepPairs: Array.from(fit.stepPairs), stepSurfacePairs: Array.from(fit.stepSurfacePairs),
                             stepRms: bits(fit.stepRms), stepSurfaceRms: bits(fit.stepSurfaceRms), q: bits(fit.rotation.flat()),
                             knnTransform: bits(knn.transform), knnIterations: knn.iterations, knnValid: knn.valid,
                             sums: bits(ms.sums), sumPairs: [ms.pairs, ms.surfacePairs], info: [ms.inScope, ms.nonfinite, ms.targetIndexed, ms.matched, ms.pairBound],
                             solved: bits(solved.transform) }));
