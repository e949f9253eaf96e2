#!/usr/bin/env node
// Driver of tests/test_sh_follow_binding.py: Scene.shFollowsTransforms without a GPU.  One Scene runs its edits in JavaScript, a
// second one through the device-scene interface with a plain Scene behind it (as tests/js/scene_binding_check.js does); both
// must leave the same shs_rgb, bandsIndices, shFrame and shHeight.
//   node sh_follow_check.js protocol   -> one JSON line { checks: [...names], failed: [...names] }
"use strict";
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const same = (a, b) => {
    if (a.length !== b.length) return false;
    const x = new Uint8Array(a.buffer, a.byteOffset, a.byteLength), y = new Uint8Array(b.buffer, b.byteOffset, b.byteLength);
    for (let i = 0; i < x.length; i++) if (x[i] !== y[i]) return false;
    return true;
};

const N = 3089, BAND = [1023, 1500, 2600];
function material(seed) {
    let s = seed >>> 0;
    const rnd = () => ((s = (Math.imul(s, 1664525) + 1013904223) >>> 0) / 4294967296);
    const rows = new Uint8Array(32 * N), f = new Float32Array(rows.buffer);
    for (let i = 0; i < N; i++) {
        f[8 * i] = -2 + (4 * i) / (N - 1);                         // x grows with the index
        for (let k = 1; k < 3; k++) f[8 * i + k] = (rnd() - 0.5) * 4;
        for (let k = 0; k < 3; k++) f[8 * i + 3 + k] = 0.01 + rnd() * 0.2;
        for (let k = 24; k < 32; k++) rows[32 * i + k] = Math.floor(rnd() * 256);
    }
    const shs = new Float32Array(48 * (N - BAND[0] - 1));
    for (let i = 0; i < shs.length; i++) shs[i] = (rnd() - 0.5) * 1.4;
    return { rows, shs };
}
function sceneOf(m, follow) {
    const s = new G.Scene();
    s.bandsIndices = new Int32Array(BAND);
    s.setData(m.rows, m.shs);
    s.shFollowsTransforms = follow;
    return s;
}

// the renderer's part with a plain Scene as the device: uploads on attach and on foreign changes (SH textures, thresholds, frame
// and the option included), runs the transforms through the twin's own loops, and hands the twin's SH state back
function stubRenderer() {
    const twin = new G.Scene();
    const calls = { readSh: 0, upload: 0, setShFollow: 0 };
    let scene = null;
    const dev = {
        hostOnly: false,
        transform: (kind, a) => {
            if (kind === 0) twin.translate(new G.Vector3(a[0], a[1], a[2]));
            else if (kind === 1) twin.rotate(new G.Quaternion(a[0], a[1], a[2], a[3]));
            else if (kind === 2) twin.scale(new G.Vector3(a[0], a[1], a[2]));
            else {
                const had = twin.shHeight > 0;
                twin.limitBox(a[0], a[1], a[2], a[3], a[4], a[5]);
                if (had && !twin.shFollowsTransforms) { twin.shHeight = 0; twin.bandsIndices = new Int32Array([-1, -1, -1]); }   // gsr_scene_limit_box drops it
            }
            return twin.vertexCount;
        },
        read: (out) => {
            const n = twin.vertexCount;
            out.data.set(twin.data.subarray(0, 8 * n)); out.positions.set(twin.positions.subarray(0, 3 * n));
            out.rotations.set(twin.rotations.subarray(0, 4 * n)); out.scales.set(twin.scales.subarray(0, 3 * n));
        },
        setShFollow: (on) => { calls.setShFollow++; twin.shFollowsTransforms = on; },
        readSh: (textures, band) => {
            calls.readSh++;
            const count = twin.shHeight ? twin.vertexCount - (twin.bandsIndices[0] + 1) : 0;
            band.set(twin.bandsIndices);
            if (textures) for (let c = 0; c < 3; c++) textures[c].set(twin.shs_rgb[c].subarray(0, 8 * count));
            return count;
        },
    };
    const upload = () => {
        calls.upload++;
        const sh = scene.shs_rgb;
        twin.vertexCount = scene.vertexCount; twin.height = scene.height;
        twin.data = scene.data.slice(); twin.positions = scene.positions.slice();
        twin.rotations = scene.rotations.slice(); twin.scales = scene.scales.slice();
        twin.shs_rgb = sh.map((t) => t.slice()); twin.shHeight = scene.shHeight; twin.bandsIndices = scene.bandsIndices.slice();
    };
    const onChange = () => { if (!scene.deviceEditApplied) upload(); };
    return {
        calls, twin,
        attach: (s) => { scene = s; s.addEventListener("change", onChange); upload(); s.attachDevice(dev); },
        detach: () => { scene.removeEventListener("change", onChange); scene.detachDevice(dev); scene = null; },
    };
}

const sameSh = (a, b) => a.shHeight === b.shHeight && same(a.bandsIndices, b.bandsIndices) && same(a.shFrame, b.shFrame) &&
    [0, 1, 2].every((c) => same(a.shs_rgb[c], b.shs_rgb[c]));
const bruteBands = (band, keep) => band.map((b) => { let c = 0; for (let i = 0; i < keep.length && i <= b; i++) if (keep[i]) c++; return c - 1; });

if (process.argv[2] === "protocol") {
    const m = material(11);
    const q = G.Quaternion.FromEuler(new G.Vector3(0.1, -0.7, 0.3)), sc = new G.Vector3(1.25, 0.75, 1.5);
    const xAt = (i) => new Float32Array(m.rows.buffer)[8 * i];
    const edits = (s) => {
        s.rotate(q); s.translate(new G.Vector3(0.25, 0, -0.5)); s.scale(sc);
        s.limitBox(-100, 100, -100, 100, -100, 100);
        s.limitBox(-100, 100, -1.2, 0.9, -100, 100);
        s.rotate(q);
    };

    // the JavaScript path alone: frame, compaction, recount
    const js = sceneOf(m, true);
    check("frame_identity_after_setData", same(js.shFrame, new Float64Array([1, 0, 0, 0, 1, 0, 0, 0, 1])));
    const before = { pos: js.positions.slice(), tex: js.shs_rgb.map((t) => t.slice()) };
    js.limitBox(xAt(700), xAt(2800), -100, 100, -100, 100);
    const keep = []; for (let i = 0; i < N; i++) keep.push(before.pos[3 * i] >= xAt(700) && before.pos[3 * i] <= xAt(2800));
    check("js_recount_is_brute_force", same(js.bandsIndices, new Int32Array(bruteBands(BAND, keep))));
    let rowsOk = true, row = 0;
    for (let i = BAND[0] + 1; i < N; i++) if (keep[i]) {
        for (let c = 0; c < 3; c++) for (let w = 0; w < 8; w++) rowsOk = rowsOk && js.shs_rgb[c][8 * row + w] === before.tex[c][8 * (i - BAND[0] - 1) + w];
        row++;
    }
    check("js_rows_move_in_order", rowsOk && row === js.vertexCount - (js.bandsIndices[0] + 1));
    check("js_zeros_behind_and_height", js.shHeight === Math.ceil((2 * row) / js.width) && js.shs_rgb.every((t) => t.length === js.width * js.shHeight * 4 && t.subarray(8 * row).every((v) => v === 0)));

    // the same edits through the device-scene interface
    const plain = sceneOf(m, true), bound = sceneOf(m, true), r = stubRenderer();
    r.attach(bound);
    check("attach_tells_the_device", r.calls.setShFollow === 1 && r.twin.shFollowsTransforms === true);
    edits(plain); edits(bound);
    check("no_sh_read_until_asked", r.calls.readSh === 0 && r.calls.upload === 1);
    check("not_dropped_with_follow", bound.shDroppedOnDevice === false);
    check("interface_path_equals_js_path", sameSh(plain, bound) && plain.vertexCount === bound.vertexCount);
    const reads = r.calls.readSh;
    void bound.shs_rgb; void bound.bandsIndices; void bound.shHeight;
    check("second_read_pulls_nothing", r.calls.readSh === reads && reads > 0);
    // no SH splat survives: the cleared state on both paths
    plain.limitBox(-100, 100, -100, 100, 50, 60); bound.limitBox(-100, 100, -100, 100, 50, 60);
    check("nothing_kept_clears_both", sameSh(plain, bound) && bound.shHeight === 0 && bound.bandsIndices[0] === -1 && bound.shs_rgb[0].length === 0);
    r.detach();

    // detach hands the SH state back; a foreign change re-uploads it with the frame
    const b2 = sceneOf(m, true), p2 = sceneOf(m, true), r2 = stubRenderer();
    r2.attach(b2);
    b2.scale(sc); b2.limitBox(-100, 100, -1.2, 0.9, -100, 100); p2.scale(sc); p2.limitBox(-100, 100, -1.2, 0.9, -100, 100);
    b2.dispatchEvent({ type: "change" });
    check("foreign_change_uploads_compacted_sh", r2.calls.upload === 2 && same(r2.twin.shs_rgb[1], p2.shs_rgb[1]) && same(r2.twin.bandsIndices, p2.bandsIndices));
    b2.limitBox(xAt(900), xAt(2700), -100, 100, -100, 100); p2.limitBox(xAt(900), xAt(2700), -100, 100, -100, 100);
    r2.detach();
    check("detach_last_refreshes_sh", sameSh(b2, p2));
    let threw = false;
    try { p2.scale(new G.Vector3(1, 0, 1)); } catch (e) { threw = true; }
    check("zero_scale_refused_with_follow", threw && sameSh(b2, p2));

    // option off: exactly as before
    const off = sceneOf(m, false), offPlain = sceneOf(m, false), r3 = stubRenderer();
    r3.attach(off);
    off.rotate(q); offPlain.rotate(q);
    check("off_frame_stays_identity", same(off.shFrame, new Float64Array([1, 0, 0, 0, 1, 0, 0, 0, 1])) && same(offPlain.shFrame, off.shFrame));
    const texBefore = off.shs_rgb.map((t) => t.slice());
    off.limitBox(-100, 100, -1.2, 0.9, -100, 100); offPlain.limitBox(-100, 100, -1.2, 0.9, -100, 100);
    check("off_limitbox_sets_shDroppedOnDevice", off.shDroppedOnDevice === true && r3.calls.readSh === 0);
    check("off_sh_untouched", [0, 1, 2].every((c) => same(off.shs_rgb[c], texBefore[c]) && same(offPlain.shs_rgb[c], texBefore[c])) &&
          same(off.bandsIndices, new Int32Array(BAND)) && same(offPlain.bandsIndices, new Int32Array(BAND)));
    off.scale(new G.Vector3(1, 0, 1));
    check("off_zero_scale_accepted", true);
    r3.detach();
    // a device scene that knows nothing of SH: with the option on it counts as host-only
    const old = sceneOf(m, true), oldPlain = sceneOf(m, true), r4 = stubRenderer();
    r4.attach(old);
    const legacy = { hostOnly: false, transform: () => { throw new Error("must not be asked"); }, read: () => {} };
    old.attachDevice(legacy);
    old.rotate(q); old.limitBox(-100, 100, -1.2, 0.9, -100, 100); oldPlain.rotate(q); oldPlain.limitBox(-100, 100, -1.2, 0.9, -100, 100);
    check("device_without_readSh_forces_js_path", sameSh(old, oldPlain) && r4.calls.upload === 3 && r4.calls.readSh === 0);
    old.detachDevice(legacy); r4.detach();
    process.stdout.write(JSON.stringify({ checks, failed }) + "\n");
}
