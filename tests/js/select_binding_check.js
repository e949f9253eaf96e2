#!/usr/bin/env node
// Driver of tests/test_select_binding.py: Scene.eraseSelection against stub device scenes.  Two of them carry the same `share`
// token and stand in front of ONE twin (one device copy); the third has no token and a twin of its own.  The mask must reach each
// distinct copy once, set before erase; without devices (or with one that cannot take a selection) the same loop runs on the host.
//   node select_binding_check.js [DIR]   -> one JSON line { checks: [...names], failed: [...names] }
// With DIR: the host loop's inputs and results as raw little-endian files there (before_*.bin, mask.bin, erased_*.bin,
// kept_*.bin; * = data, positions, rotations, scales), for the numpy compaction of the Python side.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const same = (a, b, len) => {
    if (len === undefined) { if (a.length !== b.length) return false; len = a.length; }
    const bytes = len * a.BYTES_PER_ELEMENT, x = new Uint8Array(a.buffer, a.byteOffset, bytes), y = new Uint8Array(b.buffer, b.byteOffset, bytes);
    for (let i = 0; i < bytes; i++) if (x[i] !== y[i]) return false;
    return true;
};
function rows(n, seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const out = new Uint8Array(32 * n), f = new Float32Array(out.buffer);
    for (let i = 0; i < n; i++) {
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 6; f[8 * i + 3 + k] = 0.01 + rnd() * 0.2; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const sceneOf = (r) => { const s = new G.Scene(); s.setData(r); return s; };
const equalScenes = (a, b) => a.vertexCount === b.vertexCount && a.height === b.height && a.data.length === b.data.length &&
    same(a.data, b.data, 8 * a.vertexCount) && same(a.positions, b.positions) && same(a.rotations, b.rotations) && same(a.scales, b.scales);
// the test's selection: splat i is selected iff (7 i + 3) mod 5 < 2; every bit at and above n set, which nobody may read as a splat
function maskOf(n) {
    const m = new Uint32Array(Math.ceil(n / 32) + 1).fill(0xffffffff);
    for (let i = 0; i < n; i++) if (!((7 * i + 3) % 5 < 2)) m[i >>> 5] &= ~(1 << (i & 31));
    return m;
}
const selected = (n) => { let c = 0; for (let i = 0; i < n; i++) if ((7 * i + 3) % 5 < 2) c++; return c; };

const log = [];                               // [device name, call] in the order the Scene made them
function copyOf(r) { return { twin: sceneOf(r), words: null }; }
function deviceScene(name, copy, share, bare) {
    const twin = copy.twin;
    const dev = {
        hostOnly: false,
        transform: (kind) => { log.push([name, "transform" + kind]); return twin.vertexCount; },
        read: (out) => {
            log.push([name, "read"]);
            const n = twin.vertexCount;
            out.data.set(twin.data.subarray(0, 8 * n));
            out.positions.set(twin.positions.subarray(0, 3 * n));
            out.rotations.set(twin.rotations.subarray(0, 4 * n));
            out.scales.set(twin.scales.subarray(0, 3 * n));
        },
    };
    if (!bare) {
        dev.setSelection = (words) => { log.push([name, "setSelection"]); copy.words = Uint32Array.from(words); };
        dev.eraseSelected = (keep) => {
            log.push([name, keep ? "eraseKept" : "eraseSelected"]);
            twin.eraseSelection(copy.words, { keep: keep });   // (the twin has no devices: the host loop)
            copy.words = null;
            return twin.vertexCount;
        };
    }
    if (share !== undefined) dev.share = share;
    return dev;
}
const order = () => log.map((e) => e[0] + ":" + e[1]).join(",");

const N = 3000;
{
    const R = rows(N, 11), s = sceneOf(R), free = sceneOf(R), m = maskOf(N);
    const token = {}, shared = copyOf(R), single = copyOf(R);
    const a = deviceScene("a", shared, token), x = deviceScene("x", single), b = deviceScene("b", shared, token);
    s.attachDevice(a); s.attachDevice(x); s.attachDevice(b);
    let changes = 0, applied = 0;
    s.addEventListener("change", () => { changes++; if (s.deviceEditApplied) applied++; });
    log.length = 0;
    s.eraseSelection(m); free.eraseSelection(m);
    check("erase_once_per_distinct_copy_set_before_erase", order() === "a:setSelection,a:eraseSelected,x:setSelection,x:eraseSelected");
    check("erase_count_from_the_calls", s.vertexCount === N - selected(N) && s.vertexCount === free.vertexCount && s.height === free.height);
    check("erase_reached_both_copies", equalScenes(shared.twin, free) && equalScenes(single.twin, free));
    check("change_fires_as_a_device_edit", changes === 1 && applied === 1);
    log.length = 0;
    check("mirrors_refresh_from_a_member", equalScenes(s, free) && order() === "a:read");
    check("sh_marked_dropped_like_limitbox", s.shDroppedOnDevice === true);
    // keep: the unselected go; the mask is for the new count
    const n1 = s.vertexCount, m1 = maskOf(n1);
    log.length = 0;
    s.eraseSelection(m1, { keep: true }); free.eraseSelection(m1, { keep: true });
    check("keep_once_per_distinct_copy", order() === "a:setSelection,a:eraseKept,x:setSelection,x:eraseKept" && s.vertexCount === selected(n1));
    check("keep_arrays_equal_unbound", equalScenes(s, free));
    // nothing to remove: the devices are still told (they change nothing), the count stays, "change" fires
    const n2 = s.vertexCount, none = new Uint32Array(Math.ceil(n2 / 32));
    changes = 0;
    s.eraseSelection(none); free.eraseSelection(none);
    check("nothing_selected_changes_nothing", s.vertexCount === n2 && equalScenes(s, free) && changes === 1);
    let threw = false;
    try { s.eraseSelection(new Uint32Array(Math.ceil(n2 / 32) - 1)); } catch (e) { threw = /at least/.test(e.message); }
    check("short_mask_throws", threw && s.vertexCount === n2);
}
{   // a device scene that cannot take a selection: the edit runs here, and "change" makes the renderers upload
    const R = rows(N, 12), s = sceneOf(R), free = sceneOf(R), m = maskOf(N), c = copyOf(R);
    s.attachDevice(deviceScene("old", c, undefined, true));
    let uploads = 0;
    s.addEventListener("change", () => { if (!s.deviceEditApplied) uploads++; });
    log.length = 0;
    s.eraseSelection(m); free.eraseSelection(m);
    check("device_without_selection_runs_on_the_host", uploads === 1 && equalScenes(s, free) && s.vertexCount === N - selected(N) && c.twin.vertexCount === N);
}
{   // the host loop, unbound: what numpy indexing gives (compared on the Python side too), and SH rows that follow
    const R = rows(N, 13), m = maskOf(N);
    const dump = (dir, tag, s) => {
        if (!dir) return;
        const n = s.vertexCount;
        for (const [k, per] of [["data", 8], ["positions", 3], ["rotations", 4], ["scales", 3]])
            fs.writeFileSync(path.join(dir, tag + "_" + k + ".bin"), Buffer.from(s[k].buffer, s[k].byteOffset, per * n * 4));
    };
    const dir = process.argv[2];
    const before = sceneOf(R), erased = sceneOf(R), kept = sceneOf(R);
    let changes = 0;
    erased.addEventListener("change", () => changes++);
    erased.eraseSelection(m);
    kept.eraseSelection(m, { keep: true });
    dump(dir, "before", before); dump(dir, "erased", erased); dump(dir, "kept", kept);
    if (dir) fs.writeFileSync(path.join(dir, "mask.bin"), Buffer.from(m.buffer));
    let ok = erased.vertexCount === N - selected(N) && kept.vertexCount === selected(N) && changes === 1;
    for (let i = 0, e = 0, k = 0; i < N && ok; i++) {
        const sel = (7 * i + 3) % 5 < 2, dst = sel ? kept : erased, j = sel ? k++ : e++;
        for (let w = 0; w < 8 && ok; w++) ok = dst.data[8 * j + w] === before.data[8 * i + w];
        for (let w = 0; w < 3 && ok; w++) ok = dst.positions[3 * j + w] === before.positions[3 * i + w] && dst.scales[3 * j + w] === before.scales[3 * i + w];
        for (let w = 0; w < 4 && ok; w++) ok = dst.rotations[4 * j + w] === before.rotations[4 * i + w];
    }
    check("host_loop_keeps_order_and_fires_change", ok);
    // SH rows follow with shFollowsTransforms, exactly as a limitBox that keeps the same splats leaves them
    const shs = new Float32Array(48 * (N - 100));
    for (let i = 0; i < shs.length; i++) shs[i] = ((i * 37) % 101) / 101 - 0.5;
    const mk = () => { const s = new G.Scene(); s.bandsIndices = new Int32Array([99, 1200, 2100]); s.setData(R, shs); s.shFollowsTransforms = true; return s; };
    const viaMask = mk(), viaBox = mk(), p = viaBox.positions, inBox = new Uint32Array(Math.ceil(N / 32));
    for (let i = 0; i < N; i++) if (p[3 * i] >= -1 && p[3 * i] <= 2 && p[3 * i + 1] >= -2 && p[3 * i + 1] <= 2.5 && p[3 * i + 2] >= -3 && p[3 * i + 2] <= 1) inBox[i >>> 5] |= 1 << (i & 31);
    viaMask.eraseSelection(inBox, { keep: true });
    viaBox.limitBox(-1, 2, -2, 2.5, -3, 1);
    check("sh_follows_like_limitbox", equalScenes(viaMask, viaBox) && viaMask.vertexCount > 0 && viaMask.vertexCount < N && viaMask.shHeight === viaBox.shHeight &&
          same(viaMask.bandsIndices, viaBox.bandsIndices) && [0, 1, 2].every((c) => same(viaMask.shs_rgb[c], viaBox.shs_rgb[c])));
}
console.log(JSON.stringify({ checks, failed }));
