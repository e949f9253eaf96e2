#!/usr/bin/env node
// Driver of tests/test_append_binding.py: Scene.duplicateSelection / Scene.append.
//   node append_binding_check.js protocol            -> one JSON line { checks: [...names], failed: [...names] }
//     against recording stub device scenes: two carry the same `share` token and stand in front of ONE device copy, the third has a
//     copy of its own.  The call must reach each distinct copy once (the mask before the duplicate), vertexCount follows the devices,
//     "change" fires as a device edit, the mirrors go stale and are refreshed from a member; a short mask throws; a device scene
//     without the methods sends the call to the host loop; both throw while the scene has SH rows.
//   node append_binding_check.js host ROWS OTHER OUT -> the unbound host loops: ROWS (.splat rows) pre-rotated and pre-scaled, a NaN
//     and a -0.0 put into two masked rows; duplicateSelection on the mask (7 i + 3) % 5 < 2, then append of OTHER's scene; after
//     either step data (8n words), positions, rotations, scales go to OUT.
"use strict";
const fs = require("fs");
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

const Q0 = new G.Quaternion(0.1, -0.3, 0.2, 0.9273618495495703), S0 = new G.Vector3(1.25, 0.8, 1.1);
const maskOf = (n) => {
    const m = new Uint32Array(Math.ceil(n / 32));
    for (let i = 0; i < n; i++) if ((7 * i + 3) % 5 < 2) m[i >>> 5] |= 1 << (i & 31);
    return m;
};

if (process.argv[2] === "host") {
    const make = (file) => { const s = new G.Scene(); s.setData(new Uint8Array(fs.readFileSync(file))); s.rotate(Q0); s.scale(S0); return s; };
    const s = make(process.argv[3]), other = make(process.argv[4]);
    const n = s.vertexCount, mask = maskOf(n), out = [];
    // rows 1 and 4 are masked: a NaN with a payload into y of row 1, -0.0 into x of row 4, in data as in positions
    const p = new Uint32Array(s.positions.buffer), d = s.data;
    p[3 * 1 + 1] = d[8 * 1 + 1] = 0x7fc01234;
    p[3 * 4] = d[8 * 4] = 0x80000000;
    const keep = () => { const k = s.vertexCount; for (const a of [s.data.subarray(0, 8 * k), s.positions, s.rotations, s.scales]) out.push(Buffer.from(new Uint8Array(a.buffer, a.byteOffset, a.byteLength))); };
    let changes = 0;
    s.addEventListener("change", () => { changes++; });
    const dup = s.duplicateSelection(mask);
    keep();
    const app = s.append(other);
    keep();
    fs.writeFileSync(process.argv[5], Buffer.concat(out));
    process.stdout.write(JSON.stringify({ n, m: other.vertexCount, dup, app, count: s.vertexCount, height: s.height, dataLength: s.data.length, changes }) + "\n");
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
const N = 3000, M = 257, WORDS = Math.ceil(N / 32);
const log = [];
// a recording fake device: its copy's count grows by the bits of the mask it was handed, or by m
function deviceScene(name, copy, share, bare) {
    copy.count = N;
    const dev = { hostOnly: false, transform: () => copy.count, read: () => { log.push(name + ":read"); } };
    dev.setSelection = (words) => { log.push(name + ":setSelection"); copy.words = Uint32Array.from(words); };
    dev.eraseSelected = () => copy.count;
    dev.editSelected = () => {};
    dev.paintSelected = () => {};
    if (!bare) {
        dev.duplicateSelected = () => {
            log.push(name + ":duplicate");
            let k = 0;
            for (const w of copy.words) for (let b = 0; b < 32; b++) k += (w >>> b) & 1;
            return (copy.count += k);
        };
        dev.appendArrays = (data, positions, rotations, scales, m) => {
            log.push(name + ":append");
            copy.appended = { m, typed: data instanceof Uint32Array && [positions, rotations, scales].every((a) => a instanceof Float32Array),
                              lengths: [data.length >= 8 * m, positions.length === 3 * m, rotations.length === 4 * m, scales.length === 3 * m] };
            return (copy.count += m);
        };
    }
    if (share !== undefined) dev.share = share;
    return dev;
}
const other = new G.Scene();
other.setData(rows(M));
{
    const s = new G.Scene();
    s.setData(rows(N));
    const mask = maskOf(N);
    let K = 0;
    for (let i = 0; i < N; i++) K += (mask[i >>> 5] >>> (i & 31)) & 1;
    const token = {}, shared = {}, single = {};
    s.attachDevice(deviceScene("a", shared, token)); s.attachDevice(deviceScene("x", single)); s.attachDevice(deviceScene("b", shared, token));
    let changes = 0, asDeviceEdit = 0;
    s.addEventListener("change", () => { changes++; if (s.deviceEditApplied) asDeviceEdit++; });
    log.length = 0;
    const dup = s.duplicateSelection(mask);
    check("mask_reaches_each_distinct_copy_once_before_the_duplicate", log.join(",") === "a:setSelection,a:duplicate,x:setSelection,x:duplicate");
    check("both_copies_hold_the_mask", [shared, single].every((c) => c.words.length === WORDS && c.words.every((w, k) => w === mask[k])));
    check("duplicate_returns_first_and_count", dup.first === N && dup.count === K);
    check("vertex_count_and_height_follow", s.vertexCount === N + K && s.height === Math.ceil((2 * (N + K)) / s.width));
    check("change_fires_as_a_device_edit", changes === 1 && asDeviceEdit === 1 && !s.deviceEditApplied);
    log.length = 0;
    const p = s.positions;
    check("mirrors_went_stale_and_refresh_from_a_member", log.join(",") === "a:read" && p.length === 3 * (N + K) && s.rotations.length === 4 * (N + K) && s.data.length === s.width * s.height * 4);
    log.length = 0;
    const app = s.append(other);
    check("append_reaches_each_distinct_copy_once", log.join(",") === "a:append,x:append");
    check("append_hands_over_the_four_arrays", [shared, single].every((c) => c.appended.m === M && c.appended.typed && c.appended.lengths.every(Boolean)));
    check("append_returns_first_and_count", app.first === N + K && app.count === M && s.vertexCount === N + K + M);
    check("every_call_fired_change_as_a_device_edit", changes === 2 && asDeviceEdit === 2);
    log.length = 0;
    check("short_mask_throws", throws(() => s.duplicateSelection(new Uint32Array(1)), "at least") && log.length === 0);
    check("not_a_mask_throws", throws(() => s.duplicateSelection([1, 2, 3]), "Uint32Array") && log.length === 0);
    check("append_needs_another_scene", throws(() => s.append(s), "another Scene") && throws(() => s.append({}), "another Scene") && log.length === 0);
    const empty = s.duplicateSelection(new Uint32Array(Math.ceil(s.vertexCount / 32)));
    check("an_empty_mask_adds_nothing", empty.count === 0 && empty.first === N + K + M && s.vertexCount === N + K + M);
}
{
    // a device scene without the methods: the call runs in the host loop and "change" makes the renderers upload
    const s = new G.Scene();
    s.setData(rows(N));
    const mask = maskOf(N);
    s.attachDevice(deviceScene("bare", {}, undefined, true));
    let plain = 0;
    s.addEventListener("change", () => { if (!s.deviceEditApplied) plain++; });
    const before = Float32Array.from(s.positions);
    log.length = 0;
    const dup = s.duplicateSelection(mask);
    const p = s.positions;
    let ok = plain === 1 && !log.includes("bare:setSelection") && p.length === 3 * (N + dup.count), j = 0;
    for (let i = 0; i < N && ok; i++) {
        for (let k = 0; k < 3; k++) ok = ok && p[3 * i + k] === before[3 * i + k];
        if ((mask[i >>> 5] >>> (i & 31)) & 1) { for (let k = 0; k < 3; k++) ok = ok && p[3 * (N + j) + k] === before[3 * i + k]; j++; }
    }
    check("device_without_the_methods_falls_back_to_the_host_loop", ok && j === dup.count);
}
{
    // a scene with SH rows refuses both, attached or not, and nothing changes
    const n = 64, s = new G.Scene();
    s.setData(rows(n), new Float32Array(48 * n).fill(0.25));
    const mask = maskOf(n);
    const before = Float32Array.from(s.positions);
    check("sh_rows_refuse_duplicate_and_append", throws(() => s.duplicateSelection(mask), "SH rows") && throws(() => s.append(other), "SH rows") &&
          s.vertexCount === n && s.positions.every((v, k) => v === before[k]));
    const copy = {};
    s.attachDevice(deviceScene("sh", copy));
    log.length = 0;
    check("sh_rows_refuse_before_any_device_call", throws(() => s.duplicateSelection(mask), "SH rows") && throws(() => s.append(other), "SH rows") && log.length === 0);
    const flat = new G.Scene();
    flat.setData(rows(n));
    let ok = true;
    try { flat.append(s); } catch (e) { ok = false; }      // the OTHER scene may have SH rows: they are not carried
    check("the_other_scenes_sh_rows_are_not_carried", ok && flat.vertexCount === 2 * n && flat.shHeight === 0);
}
process.stdout.write(JSON.stringify({ checks, failed }) + "\n");
