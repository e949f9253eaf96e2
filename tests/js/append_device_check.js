#!/usr/bin/env node
// Driver of tests/test_gpu_append_node.py: a Scene bound to two real HIPRenderers that do NOT share a scene (two device copies), grown
// through Scene.duplicateSelection(mask) and Scene.append(other); both copies must follow, the renderers of either copy must render
// the frame a fresh renderer renders from the Scene's arrays, and the Scene's four arrays, read back, go to OUT for the Python
// reference to compare.  renderer.duplicateSelection() / appendSelectionFrom() / reserveScene() / sceneCapacity() on one copy.
//   node append_device_check.js ROWS OTHER OUT   -> one JSON line { checks: [...names], failed: [...names], ... }
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));
const native = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js", "native", "gsplat_hip.node"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const same = (a, b) => {
    if (a.length !== b.length) return false;
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false;
    return true;
};
const throws = (f, word) => { try { f(); } catch (e) { return String(e.message).includes(word); } return false; };
const W = 200, H = 120, FX = 180;
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const count = { setSelection: 0, duplicateSelected: 0, appendArrays: 0, setSceneArrays: 0, setScene: 0 };
for (const name of Object.keys(count)) {
    const fn = native[name];
    native[name] = function () { count[name]++; return fn.apply(this, arguments); };
}
const Q0 = new G.Quaternion(0.1, -0.3, 0.2, 0.9273618495495703), S0 = new G.Vector3(1.25, 0.8, 1.1);
const make = (file) => { const s = new G.Scene(); s.setData(new Uint8Array(fs.readFileSync(file))); s.rotate(Q0); s.scale(S0); return s; };
const bound = make(process.argv[2]), other = make(process.argv[3]);
const N = bound.vertexCount, M = other.vertexCount;
const mask = new Uint32Array(Math.ceil(N / 32));
let K = 0;
for (let i = 0; i < N; i++) if ((7 * i + 3) % 5 < 2) { mask[i >>> 5] |= 1 << (i & 31); K++; }

const a = new G.HIPRenderer({ width: W, height: H }, []), b = new G.HIPRenderer({ width: W, height: H }, []);
const fresh = new G.HIPRenderer({ width: W, height: H }, []);
const frame = (r, s) => { r.renderAsync(s, camera(9)); r.sync(); return Uint8Array.from(r.readPixels()); };
const copyOf = (s) => { const v = new G.Scene(); v.vertexCount = s.vertexCount; v.height = s.height; v.data = Uint32Array.from(s.data); v.positions = Float32Array.from(s.positions); return v; };
for (const r of [a, b]) frame(r, bound);
let before = frame(fresh, copyOf(bound));
let events = 0, deviceEdits = 0;
bound.addEventListener("change", () => { events++; if (bound.deviceEditApplied) deviceEdits++; });
const uploads = count.setSceneArrays + count.setScene;
const out = [];
const keep = () => { const k = bound.vertexCount; for (const x of [bound.data.subarray(0, 8 * k), bound.positions, bound.rotations, bound.scales]) out.push(Buffer.from(new Uint8Array(x.buffer, x.byteOffset, x.byteLength))); };

const dup = bound.duplicateSelection(mask);
check("duplicate_reaches_both_device_copies", count.setSelection === 2 && count.duplicateSelected === 2 && dup.first === N && dup.count === K);
check("vertex_count_follows_the_duplicate", bound.vertexCount === N + K && bound.positions.length === 3 * (N + K));
keep();
{
    const want = frame(fresh, copyOf(bound));
    check("both_copies_render_the_grown_scene", !same(want, before) && same(frame(a, bound), want) && same(frame(b, bound), want));
    before = want;
}
// the copies are the selection of either copy
{
    const tail = new Uint32Array(Math.ceil((N + K) / 32));
    for (let i = N; i < N + K; i++) tail[i >>> 5] |= 1 << (i & 31);
    check("the_copies_are_the_selection_on_both_copies", same(a.readSelection(), tail) && same(b.readSelection(), tail));
}
const app = bound.append(other);
check("append_reaches_both_device_copies", count.appendArrays === 2 && app.first === N + K && app.count === M && bound.vertexCount === N + K + M);
keep();
{
    const want = frame(fresh, copyOf(bound));
    check("both_copies_render_the_appended_scene", !same(want, before) && same(frame(a, bound), want) && same(frame(b, bound), want));
}
check("change_fired_as_a_device_edit_and_nothing_was_uploaded", events === 2 && deviceEdits === 2 && count.setSceneArrays + count.setScene === uploads + 2);
// (the two uploads counted above are `fresh`'s: a new Scene every time)

// the renderer's own calls: this copy only
{
    const n0 = N + K + M;
    const cap = a.sceneCapacity();
    a.reserveScene(n0 + 2 * M);
    check("reserve_raises_the_capacity", cap >= n0 && a.sceneCapacity() === n0 + 2 * M && b.sceneCapacity() !== a.sceneCapacity());
    frame(a, bound);
    const r = a.duplicateSelection();            // the selection is the appended rows: M of them
    check("renderer_duplicate_returns_first_and_count", r.first === n0 && r.count === M && a.sceneCapacity() === n0 + 2 * M);
    check("a_renderer_duplicate_is_a_scene_edit", throws(() => a.pick(100, 60), "no frame"));
    const r2 = b.appendSelectionFrom(a);         // a's selection: its M copies, device to device into the other copy
    check("append_selection_from_another_renderer", r2.first === n0 && r2.count === M);
    check("both_copies_hold_the_same_scene_again", same(frame(a, bound), frame(b, bound)));
    a.setSelection(null);
    const none = a.duplicateSelection();
    let ok = true;
    try { a.pick(100, 60); } catch (e) { ok = false; }
    check("nothing_selected_adds_nothing_and_keeps_the_frame", none.count === 0 && none.first === n0 + M && ok);
}
for (const r of [a, b, fresh]) r.dispose();
fs.writeFileSync(process.argv[4], Buffer.concat(out));
console.log(JSON.stringify({ checks, failed, n: N, m: M, k: K }));
