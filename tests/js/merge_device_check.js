#!/usr/bin/env node
// Driver of tests/test_gpu_merge_node.py: splatCells / mergeCells through the Node host on the scene the Python test wrote into DIR
// as raw little-endian rows (32 bytes per splat): cluster.bin.
//   node merge_device_check.js DIR CELL   -> one JSON line { checks, failed, report, merged }
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const W = 128, H = 96;
const popcount = (w) => { let c = 0; for (let v of w) for (; v; v &= v - 1) c++; return c; };
const sum = (a) => { let t = 0; for (const v of a) t += v; return t; };

const dir = process.argv[2], cell = Number(process.argv[3]);
const r = new G.HIPRenderer({ width: W, height: H }, []);
const cam = new G.Camera(undefined, undefined, 120, 120);
G.OrbitControls.applyPose(cam, 0.4, 0.3, 8, new G.Vector3(0, 0, 0));
const R = new Uint8Array(fs.readFileSync(path.join(dir, "cluster.bin"))), n = R.length / 32, s = new G.Scene();
s.setData(R);
r.renderAsync(s, cam); r.sync();     // the scene reaches the device with its first frame
const rep = r.splatCells(cell, { cap: 16, leaders: true }), plain = r.splatCells(cell);
check("the_report_has_the_types_and_the_sizes", rep.hist instanceof Uint32Array && rep.hist.length === 17 && rep.leader instanceof Uint32Array && rep.leader.length === n &&
      plain.leader === undefined && plain.hist.length === 65);
check("the_histogram_sums_to_the_cells", sum(rep.hist) === rep.cells && rep.hist[0] === 0 && rep.inScope === n && rep.rowsAfter === n - rep.mergedMembers + rep.mergedCells);
const before = r.readSceneData();
const out = r.mergeCells(cell);
const words = Array.from(r.readSelection());
check("the_edit_does_what_the_report_announced", out.count === rep.rowsAfter && out.mergedCells === rep.mergedCells && before.vertexCount === n);
check("the_selection_is_the_merged_rows", popcount(words) === rep.mergedCells);
const after = r.readSceneData();
check("the_device_copy_has_the_new_count", after.vertexCount === out.count && after.data.length === out.count * 8);
r.renderDeviceScene(cam); r.sync();
check("the_merged_scene_renders", r.lastDepthIndex().length === out.count);
const again = r.splatCells(cell);
let refused = 0;
try { r.splatCells(cell, { budget: 1 }); } catch (e) { refused += /key tests, above the budget of 1/.test(e.message) ? 1 : 0; }
try { r.mergeCells(0); } catch (e) { refused += /cell/.test(e.message) ? 1 : 0; }
try { r.mergeCells(cell, { budget: 2 ** 39 }); } catch (e) { refused += /GSR_NEIGHBOUR_MAX_BUDGET/.test(e.message) ? 1 : 0; }
check("the_library_refusals_reach_the_caller", refused === 3);
r.dispose();
const info = (o) => [o.inScope, o.candidates, o.cells, o.mergedCells, o.mergedMembers, o.largest, o.rowsAfter, o.pairBound];
console.log(JSON.stringify({ checks, failed, width: W, height: H, n, cell, report: { leader: Array.from(rep.leader), hist: Array.from(rep.hist), info: info(rep) },
                             merged: { count: out.count, info: info(out), words, data: Array.from(after.data), positions: Array.from(new Uint32Array(after.positions.buffer)),
                                       again: info(again) } }));
