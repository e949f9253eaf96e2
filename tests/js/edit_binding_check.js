#!/usr/bin/env node
// Driver of tests/test_edit_binding.py: Scene.translateSelection / rotateSelection / scaleSelection / paintSelection.
//   node edit_binding_check.js protocol              -> one JSON line { checks: [...names], failed: [...names] }
//     against stub device scenes: two carry the same `share` token and stand in front of ONE device copy, the third has a copy of
//     its own.  The mask must reach each distinct copy once, before the edit; "change" fires as a device edit; the mirrors are
//     refreshed from a member; a short mask throws; a device scene without the methods sends the edit to the host loop; the
//     SH-follow refusal throws.
//   node edit_binding_check.js host ROWS OUT         -> the unbound host loops: ROWS (.splat rows) pre-rotated and pre-scaled, then
//     the walk below on the mask (7 i + 3) % 5 < 2; after every step data (8n words), positions, rotations, scales go to OUT.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const Q0 = new G.Quaternion(0.1, -0.3, 0.2, 0.9273618495495703), S0 = new G.Vector3(1.25, 0.8, 1.1);
const T = new G.Vector3(0.25, -0.5, 1.0), Q = new G.Quaternion(-0.2, 0.5, 0.1, 0.8366600265340756), S = new G.Vector3(0.9, 1.2, 1.05);
const PIVOT = [0.3, -0.7, 1.9];
const maskOf = (n) => {
    const m = new Uint32Array(Math.ceil(n / 32));
    for (let i = 0; i < n; i++) if ((7 * i + 3) % 5 < 2) m[i >>> 5] |= 1 << (i & 31);
    return m;
};

if (process.argv[2] === "host") {
    const rows = new Uint8Array(fs.readFileSync(process.argv[3]));
    const s = new G.Scene();
    s.setData(rows);
    s.rotate(Q0);
    s.scale(S0);
    const n = s.vertexCount, mask = maskOf(n), out = [];
    // (Buffer.from(Uint8Array) copies: the arrays go on changing)
    const keep = () => { for (const a of [s.data.subarray(0, 8 * n), s.positions, s.rotations, s.scales]) out.push(Buffer.from(new Uint8Array(a.buffer, a.byteOffset, a.byteLength))); };
    const steps = [
        () => s.translateSelection(mask, T), () => s.rotateSelection(mask, Q), () => s.rotateSelection(mask, Q, { pivot: PIVOT }),
        () => s.scaleSelection(mask, S), () => s.scaleSelection(mask, S, { pivot: new G.Vector3(PIVOT[0], PIVOT[1], PIVOT[2]) }),
        () => s.paintSelection(mask, { a: 0x60 }), () => s.paintSelection(mask, { r: 0x20, g: 0xc0, b: 0x40 }),
    ];
    let changes = 0;
    s.addEventListener("change", () => { changes++; });
    for (const step of steps) { step(); keep(); }
    fs.writeFileSync(process.argv[4], Buffer.concat(out));
    process.stdout.write(JSON.stringify({ n, steps: steps.length, changes }) + "\n");
    process.exit(0);
}

const checks = [], failed = [];
const check = (name, ok) => { checks.push(name); if (!ok) failed.push(name); };
const throws = (f, word) => { try { f(); } catch (e) { return String(e.message).includes(word); } return false; };
function rows(n) {
    const out = new Uint8Array(32 * n), f = new Float32Array(out.buffer);
    for (let i = 0; i < n; i++) {
        for (let k = 0; k < 3; k++) { f[8 * i + k] = ((i * 7 + k * 3) % 11) - 5; f[8 * i + 3 + k] = 0.05; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = (i + k) & 255;
    }
    return out;
}
const N = 3000, WORDS = Math.ceil(N / 32);
const log = [];
function deviceScene(name, copy, share, bare) {
    const dev = { hostOnly: false, transform: () => N, read: () => { log.push(name + ":read"); } };
    dev.setSelection = (words) => { log.push(name + ":setSelection"); copy.words = Uint32Array.from(words); };
    dev.eraseSelected = () => N;
    if (!bare) {
        dev.editSelected = (kind, args, pivot) => { log.push(name + ":edit" + kind); copy.edit = { kind, args: Array.from(args), pivot: pivot === null ? null : Array.from(pivot), f64: args instanceof Float64Array && (pivot === null || pivot instanceof Float64Array) }; };
        dev.paintSelected = (rgba, byteMask) => { log.push(name + ":paint"); copy.paint = [rgba, byteMask]; };
    }
    if (share !== undefined) dev.share = share;
    return dev;
}
{
    const s = new G.Scene();
    s.setData(rows(N));
    const mask = maskOf(N);
    const token = {}, shared = {}, single = {};
    s.attachDevice(deviceScene("a", shared, token)); s.attachDevice(deviceScene("x", single)); s.attachDevice(deviceScene("b", shared, token));
    let changes = 0, asDeviceEdit = 0;
    s.addEventListener("change", () => { changes++; if (s.deviceEditApplied) asDeviceEdit++; });
    log.length = 0;
    s.rotateSelection(mask, Q, { pivot: PIVOT });
    check("mask_reaches_each_distinct_copy_once_before_the_edit", log.join(",") === "a:setSelection,a:edit1,x:setSelection,x:edit1");
    check("both_copies_hold_the_mask", [shared, single].every((c) => c.words.length === WORDS && c.words.every((w, k) => w === mask[k])));
    check("rotate_passes_xyzw_and_the_pivot_as_f64", [shared, single].every((c) => c.edit.f64 && c.edit.kind === 1 && String(c.edit.args) === String([Q.x, Q.y, Q.z, Q.w]) && String(c.edit.pivot) === String(PIVOT)));
    check("change_fires_as_a_device_edit", changes === 1 && asDeviceEdit === 1 && !s.deviceEditApplied);
    log.length = 0;
    void s.positions;
    check("mirrors_refresh_from_a_member", log.join(",") === "a:read");
    log.length = 0;
    void s.data;
    check("mirrors_refresh_once", log.length === 0);
    log.length = 0;
    s.translateSelection(mask, T);
    check("translate_has_no_pivot", log.join(",") === "a:setSelection,a:edit0,x:setSelection,x:edit0" && shared.edit.pivot === null && String(shared.edit.args) === String([T.x, T.y, T.z]));
    s.scaleSelection(mask, S);
    check("no_pivot_is_null_not_zero", shared.edit.kind === 2 && shared.edit.pivot === null && String(single.edit.args) === String([S.x, S.y, S.z]));
    s.scaleSelection(mask, S, { pivot: new G.Vector3(1, 2, 3) });
    check("a_vector3_pivot_passes", String(shared.edit.pivot) === "1,2,3");
    log.length = 0;
    s.paintSelection(mask, { a: 0x60 });
    check("paint_sends_the_word_and_the_byte_mask", log.join(",") === "a:setSelection,a:paint,x:setSelection,x:paint" && shared.paint[0] === 0x60000000 && shared.paint[1] === 0xff000000);
    s.paintSelection(mask, { r: 0x20, g: 0xc0, b: 0x40 });
    check("absent_channels_are_left_alone", single.paint[0] === 0x0040c020 && single.paint[1] === 0x00ffffff);
    check("every_edit_fired_change_as_a_device_edit", changes === 6 && asDeviceEdit === 6 && s.vertexCount === N);
    log.length = 0;
    check("short_mask_throws", ["translateSelection", "rotateSelection", "scaleSelection", "paintSelection"].every((m) =>
        throws(() => s[m](new Uint32Array(WORDS - 1), m === "rotateSelection" ? Q : m === "paintSelection" ? { a: 1 } : T), "at least " + WORDS)) && log.length === 0);
    check("not_a_mask_throws", throws(() => s.translateSelection([1, 2, 3], T), "Uint32Array"));
    check("non_finite_scale_throws", throws(() => s.scaleSelection(mask, new G.Vector3(1, Infinity, 1)), "finite") && log.length === 0);
    check("a_bad_channel_throws", throws(() => s.paintSelection(mask, { r: 256 }), "0..255") && log.length === 0);
}
{
    // a device scene without the methods: the edit runs in the host loop and "change" makes the renderers upload
    const s = new G.Scene();
    s.setData(rows(N));
    const mask = maskOf(N);
    s.attachDevice(deviceScene("bare", {}, undefined, true));
    let plain = 0;
    s.addEventListener("change", () => { if (!s.deviceEditApplied) plain++; });
    const before = Float32Array.from(s.positions);
    log.length = 0;
    s.translateSelection(mask, T);
    const p = s.positions;
    let ok = plain === 1 && !log.includes("bare:setSelection");
    for (let i = 0; i < N && ok; i++) {
        const sel = (mask[i >>> 5] >>> (i & 31)) & 1;
        for (let k = 0; k < 3; k++) ok = ok && p[3 * i + k] === (sel ? Math.fround(before[3 * i + k] + [T.x, T.y, T.z][k]) : before[3 * i + k]);
    }
    check("device_without_the_methods_falls_back_to_the_host_loop", ok);
}
{
    // SH follows the transforms and the scene has SH rows: a selection cannot be rotated or scaled; translate and paint pass
    const n = 64, s = new G.Scene();
    s.setData(rows(n), new Float32Array(48 * n).fill(0.25));
    const mask = maskOf(n);
    s.shFollowsTransforms = true;
    const before = Float32Array.from(s.positions);
    check("sh_follow_refusal_throws", throws(() => s.rotateSelection(mask, Q), "SH frame") && throws(() => s.scaleSelection(mask, S, { pivot: PIVOT }), "SH frame") &&
          s.positions.every((v, k) => v === before[k]));
    let ok = true;
    try { s.translateSelection(mask, T); s.paintSelection(mask, { a: 7 }); } catch (e) { ok = false; }
    check("translate_and_paint_pass_under_sh_follow", ok && s.positions.some((v, k) => v !== before[k]));
    s.shFollowsTransforms = false;
    try { s.rotateSelection(mask, Q); } catch (e) { ok = false; }
    check("rotate_passes_with_sh_follow_off", ok);
    const flat = new G.Scene();
    flat.setData(rows(n));
    flat.shFollowsTransforms = true;
    try { flat.rotateSelection(mask, Q); } catch (e) { ok = false; }
    check("rotate_passes_without_sh_rows", ok);
}
process.stdout.write(JSON.stringify({ checks, failed }) + "\n");
