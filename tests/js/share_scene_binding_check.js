#!/usr/bin/env node
// Driver of tests/test_share_scene_binding.py: a Scene attached to three stub device scenes.  Two of them carry the same `share`
// token and stand in front of ONE twin (one device copy, as renderers whose contexts share a scene); the third has no token and
// a twin of its own.  An edit applied twice to the shared twin would show in its arrays.
//   node share_scene_binding_check.js   -> one JSON line { checks: [...names], failed: [...names] }
"use strict";
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

const log = [];                               // [device name, call] in the order the Scene made them
// a device copy: a plain Scene behind the calls; `holders` device scenes may stand in front of one
function copyOf(r) { return { twin: sceneOf(r), follow: false }; }
function deviceScene(name, copy, share) {
    const twin = copy.twin;
    const dev = {
        hostOnly: false,
        transform: (kind, a) => {
            log.push([name, "transform" + kind]);
            if (kind === 0) twin.translate(new G.Vector3(a[0], a[1], a[2]));
            else if (kind === 1) twin.rotate(new G.Quaternion(a[0], a[1], a[2], a[3]));
            else if (kind === 2) twin.scale(new G.Vector3(a[0], a[1], a[2]));
            else twin.limitBox(a[0], a[1], a[2], a[3], a[4], a[5]);
            return twin.vertexCount;
        },
        read: (out) => {
            log.push([name, "read"]);
            const n = twin.vertexCount;
            out.data.set(twin.data.subarray(0, 8 * n));
            out.positions.set(twin.positions.subarray(0, 3 * n));
            out.rotations.set(twin.rotations.subarray(0, 4 * n));
            out.scales.set(twin.scales.subarray(0, 3 * n));
        },
        setShFollow: (on) => { log.push([name, "setShFollow"]); copy.follow = on; },
        readSh: (textures, band) => { band.set([-1, -1, -1]); return 0; },
    };
    if (share !== undefined) dev.share = share;
    return dev;
}
const calls = (what) => log.filter((e) => e[1] === what).map((e) => e[0]).join(",");
const q = G.Quaternion.FromEuler(new G.Vector3(0.1, -0.7, 0.3));

{
    const R = rows(3000, 11), s = sceneOf(R), free = sceneOf(R);
    const token = {}, shared = copyOf(R), single = copyOf(R);
    const a = deviceScene("a", shared, token), x = deviceScene("x", single), b = deviceScene("b", shared, token);
    s.attachDevice(a); s.attachDevice(x); s.attachDevice(b);         // the single one between the two members
    log.length = 0;
    s.rotate(q); free.rotate(q);
    check("rotate_once_per_distinct_share_in_attach_order", calls("transform1") === "a,x" && log.length === 2);
    check("rotate_reached_both_copies", same(shared.twin.positions, free.positions) && same(single.twin.positions, free.positions) &&
          same(shared.twin.rotations, free.rotations));
    log.length = 0;
    s.limitBox(-2, 2, -2.5, 2.5, -1, 3); free.limitBox(-2, 2, -2.5, 2.5, -1, 3);
    check("limitbox_once_per_distinct_share_in_attach_order", calls("transform3") === "a,x" && log.length === 2);
    check("limitbox_count_from_the_calls", s.vertexCount === free.vertexCount && s.vertexCount > 0 && s.vertexCount < 3000 && s.height === free.height);
    log.length = 0;
    s.shFollowsTransforms = true;
    check("set_sh_follow_once_per_distinct_share", calls("setShFollow") === "a,x" && log.length === 2 && shared.follow === true && single.follow === true);
    s.shFollowsTransforms = false;
    log.length = 0;
    const p = s.positions;
    check("mirrors_refresh_from_a_member", calls("read") === "a" && same(p, free.positions));
    check("arrays_equal_unbound", equalScenes(s, free));
    // after the shared pair is detached, the Scene goes on with the third
    s.detachDevice(a); s.detachDevice(b);
    log.length = 0;
    s.rotate(q); free.rotate(q);
    const alone = calls("transform1") === "x" && log.length === 1;
    check("without_tokens_every_device_is_called", (() => {   // two device scenes without tokens count singly, as they always did
        const s2 = sceneOf(R), c1 = copyOf(R), c2 = copyOf(R), n0 = log.length;
        s2.attachDevice(deviceScene("u", c1)); s2.attachDevice(deviceScene("v", c2, null));
        s2.rotate(q);
        const made = log.slice(n0).filter((e) => e[1] === "transform1").map((e) => e[0]).join(",");
        log.length = n0;
        return made === "u,v";
    })());
    check("third_alone_still_works", alone && same(single.twin.positions, free.positions));
    check("third_alone_arrays_equal_unbound", equalScenes(s, free) && calls("read") === "x");
}
console.log(JSON.stringify({ checks, failed }));
