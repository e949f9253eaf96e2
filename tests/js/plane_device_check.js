#!/usr/bin/env node
// Driver of tests/test_gpu_plane_node.py: fitPlane / selectPlane / planeAlignment / planeInliers through the Node host, and
// Scene.rotate / Scene.translate acting on the device copy, on the rows the test wrote.
//   node plane_device_check.js DIR   (DIR/rows.bin: .splat rows)  -> one JSON line { checks, failed, ... }
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const W = 128, H = 96, THRESHOLD = 0.01, HYPOTHESES = 256;
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };

const dir = process.argv[2];
const file = fs.readFileSync(path.join(dir, "rows.bin"));
const R = new Uint8Array(file.buffer, file.byteOffset, file.byteLength), N = R.length / 32;
const s = new G.Scene();
s.setData(R);
const r = new G.HIPRenderer({ width: W, height: H }, []);
const cam = new G.Camera(undefined, undefined, 120, 120);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
r.renderAsync(s, cam); r.sync();     // the scene reaches the device with its first frame

const fit = r.fitPlane(THRESHOLD, { hypotheses: HYPOTHESES, scores: true });
check("the_fit_has_the_types_and_the_sizes", fit.found === true && fit.plane instanceof Float64Array && fit.plane.length === 4 && fit.triple instanceof Uint32Array &&
      fit.scores instanceof Uint32Array && fit.scores.length === HYPOTHESES && fit.inScope === N && fit.tests === HYPOTHESES * N && fit.hypotheses === HYPOTHESES);
check("the_winner_has_the_largest_score_and_the_smallest_index", fit.scores[fit.best] === fit.inliers && fit.scores.every((v, h) => v < fit.inliers || (v === fit.inliers && h >= fit.best)));
const within = r.selectPlane(fit.plane, { within: THRESHOLD }), words = Array.from(r.readSelection());
check("what_the_fit_counted_is_what_the_interval_selects", within === fit.inliers && popcount(words) === within);
const under = r.selectPlane(fit.plane, { hi: -THRESHOLD }), over = r.selectPlane(fit.plane, { lo: THRESHOLD, op: "add" });
const off = (() => { let k = 0; for (const a of [-THRESHOLD, THRESHOLD]) k += r.selectPlane(fit.plane, { lo: a, hi: a }); return k; })();   // splats at exactly +-threshold are in both
check("the_three_intervals_cover_the_scene", under + within + (over - under) - off === N);
const own = Array.from(r.planeInliers([fit.plane, [0, 1, 0, 0]], THRESHOLD));
check("the_scoring_pass_alone_agrees", own[0] === fit.inliers);
const { rotation, translation } = r.planeAlignment(fit.plane);
check("the_alignment_is_a_unit_quaternion", rotation instanceof G.Quaternion && translation instanceof G.Vector3 &&
      Math.abs(rotation.x * rotation.x + rotation.y * rotation.y + rotation.z * rotation.z + rotation.w * rotation.w - 1) < 1e-15);
s.rotate(rotation); s.translate(translation);     // on every device copy
const after = r.planeInliers([[0, 1, 0, 0]], THRESHOLD + 2 ** -19)[0];
check("the_floor_lies_at_y_0", after >= fit.inliers);
let refused = 0;
try { r.fitPlane(THRESHOLD, { budget: 1 }); } catch (e) { refused += /tests .*above the budget of 1/.test(e.message) ? 1 : 0; }
try { r.fitPlane(-1); } catch (e) { refused += /threshold/.test(e.message) ? 1 : 0; }
try { r.selectPlane([0, 0, 0, 1]); } catch (e) { refused += /zero normal/.test(e.message) ? 1 : 0; }
try { r.planeAlignment([0, 0, 0, 1]); } catch (e) { refused += /normal is zero/.test(e.message) ? 1 : 0; }
try { r.planeInliers([[0, 1, 0, 0]], THRESHOLD, { budget: 2 ** 39 }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
check("the_library_refusals_reach_the_caller", refused === 5);
r.dispose();
console.log(JSON.stringify({ checks, failed, n: N, width: W, height: H, threshold: THRESHOLD, hypotheses: HYPOTHESES, plane: Array.from(fit.plane), best: fit.best,
                             triple: Array.from(fit.triple), inliers: fit.inliers, degenerate: fit.degenerate, nonfinite: fit.nonfinite, scores: Array.from(fit.scores),
                             within, words, under, over, own, q: rotation.flat(), t: [translation.x, translation.y, translation.z], after }));
