#!/usr/bin/env node
// Driver of tests/test_gpu_edit_node.py: a Scene attached to real HIPRenderers -- two that share one device copy and one with a copy
// of its own -- edited through Scene.translateSelection / rotateSelection / scaleSelection / paintSelection; after every step its
// four arrays must equal, bit for bit, those of an unbound Scene (the host loops) given the same input, and the renderers of either
// copy must render the frame a fresh renderer renders from those arrays.  renderer.selectionBounds() against a JavaScript min / max.
//   node edit_device_check.js   -> one JSON line { checks: [...names], failed: [...names] }
"use strict";
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));
const native = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js", "native", "gsplat_hip.node"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const bits = (a) => new Uint32Array(a.buffer, a.byteOffset, a.byteLength / 4);
const same = (a, b) => {
    if (a.length !== b.length) return false;
    for (let i = 0; i < a.length; i++) if (a[i] !== b[i]) return false;
    return true;
};
const throws = (f, word) => { try { f(); } catch (e) { return String(e.message).includes(word); } return false; };
function rows(n, seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const out = new Uint8Array(32 * n), f = new Float32Array(out.buffer);
    for (let i = 0; i < n; i++) {
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 5; f[8 * i + 3 + k] = 0.01 + rnd() * 0.08; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 200, H = 120, FX = 180, N = 5000;
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
const count = { setSelection: 0, editSelected: 0, paintSelected: 0, setSceneArrays: 0, setScene: 0 };
for (const name of Object.keys(count)) {
    const fn = native[name];
    native[name] = function () { count[name]++; return fn.apply(this, arguments); };
}
const Q0 = new G.Quaternion(0.1, -0.3, 0.2, 0.9273618495495703), S0 = new G.Vector3(1.25, 0.8, 1.1);
const T = new G.Vector3(0.25, -0.5, 1.0), Q = new G.Quaternion(-0.2, 0.5, 0.1, 0.8366600265340756), S = new G.Vector3(0.9, 1.2, 1.05);
const PIVOT = [0.3, -0.7, 1.9];
const mask = new Uint32Array(Math.ceil(N / 32));
for (let i = 0; i < N; i++) if ((7 * i + 3) % 5 < 2) mask[i >>> 5] |= 1 << (i & 31);

const R = rows(N, 13);
const make = () => { const s = new G.Scene(); s.setData(R); s.rotate(Q0); s.scale(S0); return s; };
const bound = make(), host = make();
const a = new G.HIPRenderer({ width: W, height: H }, []);
const b = new G.HIPRenderer({ width: W, height: H, throughput: true, shareSceneWith: a }, []);
const own = new G.HIPRenderer({ width: W, height: H }, []);
const fresh = new G.HIPRenderer({ width: W, height: H }, []), freshT = new G.HIPRenderer({ width: W, height: H, throughput: true }, []);
const frame = (r, s) => { r.renderAsync(s, camera(9)); r.sync(); return Uint8Array.from(r.readPixels()); };
// `host` stays unattached, so its edits are the host loops: `fresh` renders a copy of its data and positions in a Scene of its own
const copyOf = (s) => { const v = new G.Scene(); v.vertexCount = s.vertexCount; v.height = s.height; v.data = Uint32Array.from(s.data); v.positions = Float32Array.from(s.positions); return v; };
for (const r of [a, b, own]) frame(r, bound);
let before = frame(fresh, copyOf(host));
let events = 0, deviceEdits = 0;
bound.addEventListener("change", () => { events++; if (bound.deviceEditApplied) deviceEdits++; });
const uploads = count.setSceneArrays + count.setScene;

const steps = [
    ["translate", (s) => s.translateSelection(mask, T)],
    ["rotate", (s) => s.rotateSelection(mask, Q)],
    ["rotate_pivot", (s) => s.rotateSelection(mask, Q, { pivot: PIVOT })],
    ["scale", (s) => s.scaleSelection(mask, S)],
    ["scale_pivot", (s) => s.scaleSelection(mask, S, { pivot: new G.Vector3(PIVOT[0], PIVOT[1], PIVOT[2]) })],
    ["paint_opacity", (s) => s.paintSelection(mask, { a: 0x60 })],
    ["paint_colour", (s) => s.paintSelection(mask, { r: 0x20, g: 0xc0, b: 0x40 })],
];
for (const [name, step] of steps) {
    count.setSelection = count.editSelected = count.paintSelected = 0;
    step(bound);
    step(host);
    const calls = count.editSelected + count.paintSelected;
    check(name + "_once_per_device_copy", count.setSelection === 2 && calls === 2);
    check(name + "_arrays_equal_the_host_loop", same(bound.data.subarray(0, 8 * N), host.data.subarray(0, 8 * N)) && same(bits(bound.positions), bits(host.positions)) &&
          same(bits(bound.rotations), bits(host.rotations)) && same(bits(bound.scales), bits(host.scales)) && bound.vertexCount === N);
    const want = frame(fresh, copyOf(host));
    // (a throughput context cuts its work items differently, so its bytes are compared with a fresh throughput context's)
    check(name + "_every_renderer_renders_the_edited_scene", !same(want, before) && [a, own].every((r) => same(frame(r, bound), want)) &&
          same(frame(b, bound), frame(freshT, copyOf(host))));
    before = want;
}
check("change_fired_as_a_device_edit_and_nothing_was_uploaded", events === steps.length && deviceEdits === steps.length && count.setSceneArrays + count.setScene === uploads + 2 * steps.length);
// (the uploads counted above are `fresh`'s and `freshT`'s, one per step each: a new Scene every time)
check("the_selection_is_the_mask_on_both_copies", same(a.readSelection(), mask) && same(b.readSelection(), mask) && same(own.readSelection(), mask));

// selectionBounds against a JavaScript min / max over the Scene's positions
{
    const p = bound.positions, mn = [Infinity, Infinity, Infinity], mx = [-Infinity, -Infinity, -Infinity];
    let n = 0;
    for (let i = 0; i < N; i++) {
        if (!((mask[i >>> 5] >>> (i & 31)) & 1)) continue;
        n++;
        for (let k = 0; k < 3; k++) { const v = p[3 * i + k]; if (v < mn[k]) mn[k] = v; if (v > mx[k]) mx[k] = v; }
    }
    const got = own.selectionBounds(), shared = b.selectionBounds();
    check("selection_bounds_equal_a_javascript_min_max", got.count === n && [0, 1, 2].every((k) => got.min[k] === mn[k] && got.max[k] === mx[k]) &&
          shared.count === n && [0, 1, 2].every((k) => shared.min[k] === mn[k] && shared.max[k] === mx[k]));
    own.setSelection(null);
    const none = own.selectionBounds();
    check("selection_bounds_of_nothing", none.count === 0 && none.min.every((v) => v === Infinity) && none.max.every((v) => v === -Infinity));
}
// the renderer's own edits: this copy only; a scene edit
{
    own.setSelection(mask);
    frame(own, bound);
    own.rotateSelection(Q, { pivot: PIVOT });
    check("a_renderer_edit_is_a_scene_edit", throws(() => own.pick(100, 60), "no frame"));
    host.rotateSelection(mask, Q, { pivot: PIVOT });
    own.paintSelection({ a: 0x30 });
    host.paintSelection(mask, { a: 0x30 });
    own.translateSelection([T.x, T.y, T.z]);
    host.translateSelection(mask, T);
    own.scaleSelection(S);
    host.scaleSelection(mask, S);
    check("renderer_edits_equal_the_host_loop", same(frame(own, bound), frame(fresh, copyOf(host))));
    check("non_finite_scale_is_refused", throws(() => own.scaleSelection([1, NaN, 1]), "finite"));
}
for (const r of [a, b, own, fresh, freshT]) r.dispose();
console.log(JSON.stringify({ checks, failed }));
