#!/usr/bin/env node
// Driver of tests/test_scene_binding.py: the Scene's binding to device scenes, run against a stub device scene (a second
// plain Scene behind the interface { transform, read, hostOnly }), so the whole protocol is checked without a GPU.
//   node scene_binding_check.js protocol   -> one JSON line { checks: [...names], failed: [...names] }
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

function rows(n, seed) {                   // .splat rows from a small generator of its own
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

// A renderer's part of the protocol with a plain Scene as the "device": upload on attach and on a "change" that is not a device
// edit's, the transforms through the twin's own loops.
function stubRenderer(opts) {
    const twin = new G.Scene();
    const calls = { transform: 0, read: 0, upload: 0 };
    let scene = null;
    const dev = {
        hostOnly: !!(opts && opts.hostOnly),
        transform: (kind, a) => {
            calls.transform++;
            if (kind === 0) twin.translate(new G.Vector3(a[0], a[1], a[2]));
            else if (kind === 1) twin.rotate(new G.Quaternion(a[0], a[1], a[2], a[3]));
            else if (kind === 2) twin.scale(new G.Vector3(a[0], a[1], a[2]));
            else twin.limitBox(a[0], a[1], a[2], a[3], a[4], a[5]);
            return twin.vertexCount + (opts && opts.lie ? 1 : 0);
        },
        read: (out) => {
            calls.read++;
            const n = twin.vertexCount;
            out.data.set(twin.data.subarray(0, 8 * n));
            out.positions.set(twin.positions.subarray(0, 3 * n));
            out.rotations.set(twin.rotations.subarray(0, 4 * n));
            out.scales.set(twin.scales.subarray(0, 3 * n));
        },
    };
    const upload = () => {
        calls.upload++;
        twin.vertexCount = scene.vertexCount; twin.height = scene.height;
        twin.data = scene.data.slice(); twin.positions = scene.positions.slice();
        twin.rotations = scene.rotations.slice(); twin.scales = scene.scales.slice();
    };
    const onChange = () => { if (!scene.deviceEditApplied) upload(); };
    return {
        calls, twin, dev,
        attach: (s) => { scene = s; s.addEventListener("change", onChange); upload(); s.attachDevice(dev); },
        detach: () => { scene.removeEventListener("change", onChange); scene.detachDevice(dev); scene = null; },
    };
}
const raw = (s) => ({ data: s._data, positions: s._positions, rotations: s._rotations, scales: s._scales });
const equalScenes = (a, b) => a.vertexCount === b.vertexCount && a.height === b.height && a.data.length === b.data.length &&
    same(a.data, b.data, 8 * a.vertexCount) && same(a.positions, b.positions) && same(a.rotations, b.rotations) && same(a.scales, b.scales);

const q = G.Quaternion.FromEuler(new G.Vector3(0.1, -0.7, 0.3)), t = new G.Vector3(0.25, -0.5, 1), sc = new G.Vector3(1.1, 0.9, 1.3);

if (process.argv[2] === "protocol") {
    const R = rows(3000, 7);
    {   // a transform calls every attached device scene once, runs no loop here, and the arrays wait until they are read
        const s = sceneOf(R), free = sceneOf(R), a = stubRenderer(), b = stubRenderer();
        let events = 0, seenInEvent = null;
        s.addEventListener("change", () => { events++; });
        a.attach(s); b.attach(s);
        const before = { p: s._positions.slice(), d: s._data.slice(), p0: s._positions };
        s.rotate(q); free.rotate(q);
        check("transform_once_per_device", a.calls.transform === 1 && b.calls.transform === 1 && a.calls.upload === 1 && b.calls.upload === 1);
        check("no_js_loop_until_read", same(s._positions, before.p) && same(s._data, before.d) && a.calls.read === 0);
        check("change_once_per_edit", events === 1);
        const d1 = s.data;
        check("first_read_pulls_once", a.calls.read === 1 && b.calls.read === 0 && same(d1, free.data));
        const p1 = s.positions, r1 = s.rotations, s1 = s.scales, d2 = s.data;
        check("second_read_pulls_nothing", a.calls.read === 1 && d2 === d1 && p1 === before.p0);
        check("arrays_equal_unbound_after_rotate", equalScenes(s, free) && same(r1, free.rotations) && same(s1, free.scales));
        // limitBox: count and height at once, shapes of the arrays as the loop leaves them
        s.limitBox(-2, 2, -2.5, 2.5, -1, 3); free.limitBox(-2, 2, -2.5, 2.5, -1, 3);
        check("limitbox_count_at_once", s.vertexCount === free.vertexCount && s.height === free.height && s.vertexCount > 0 && s.vertexCount < 3000 &&
              a.calls.read === 1 && s.shDroppedOnDevice === true);
        check("limitbox_shapes", equalScenes(s, free) && !s.data.subarray(8 * s.vertexCount).some((w) => w !== 0));
        // a third-party listener that reads scene.data inside "change" sees the edit
        const onEdit = () => { seenInEvent = s.data.slice(0, 8 * s.vertexCount); };
        s.addEventListener("change", onEdit);
        s.translate(t); free.translate(t);
        s.removeEventListener("change", onEdit);
        check("listener_reads_edited_words", seenInEvent !== null && same(seenInEvent, free.data, 8 * free.vertexCount));
        check("toSplatBytes_refreshes", (s.scale(sc), free.scale(sc), same(s.toSplatBytes(), free.toSplatBytes())));
        // a foreign "change" (the caller wrote into positions and said so) uploads everywhere
        const up = a.calls.upload;
        s.positions[0] += 1; free.positions[0] += 1;
        s.dispatchEvent({ type: "change" });
        check("foreign_change_uploads", a.calls.upload === up + 1 && b.calls.upload === up + 1 && same(a.twin.positions, s.positions));
        // ... also while the mirrors are stale: refresh, then upload
        s.scale(sc); free.scale(sc);
        const reads = a.calls.read;
        s.dispatchEvent({ type: "change" });
        check("foreign_change_while_stale_refreshes_first", a.calls.read === reads + 1 && a.calls.upload === up + 2 && same(a.twin.scales, free.scales));
        // detaching: the first to go leaves the edits with the other, the last one hands them back
        s.rotate(q); free.rotate(q);
        const r0 = a.calls.read + b.calls.read;
        a.detach();
        check("detach_not_last_reads_nothing", a.calls.read + b.calls.read === r0 && s._stale === true);
        b.detach();
        check("detach_last_refreshes", b.calls.read === 1 && s._stale === false && same(s._positions, free.positions) && same(s._rotations, free.rotations));
        s.translate(t); free.translate(t);
        check("unattached_again_is_plain_js", b.calls.transform === a.calls.transform && equalScenes(s, free));
    }
    {   // setters and setData put the host in charge; the next "change" brings the devices back
        const s = sceneOf(R), free = sceneOf(R), a = stubRenderer();
        a.attach(s);
        s.scale(sc); free.scale(sc);
        const np = free.positions.slice();
        np[5] = 9; s.positions = np; free.positions = np.slice();
        check("setter_refreshes_then_owns", a.calls.read === 1 && s._diverged === true && same(s.scales, free.scales) && s.positions === np);
        const x = a.calls.transform;
        s.translate(t); free.translate(t);        // (the reference's loops: positions move, data words 0..2 follow)
        check("edit_after_setter_runs_on_host", a.calls.transform === x && a.calls.upload === 2 && equalScenes(s, free) && s._diverged === false);
        s.rotate(q); free.rotate(q);
        check("back_on_device_after_upload", a.calls.transform === x + 1 && equalScenes(s, free));
        const R2 = rows(500, 11);
        s.setData(R2); free.setData(R2);
        check("setData_uploads_and_owns", a.calls.upload === 3 && a.calls.read === 2 && s._stale === false && s.shDroppedOnDevice === false && equalScenes(s, free));
        s.scale(sc); free.scale(sc);
        check("device_path_after_setData", a.calls.transform === x + 2 && equalScenes(s, free));
    }
    {   // a host-only device scene among the attached: the whole edit takes the JavaScript path and uploads everywhere
        const s = sceneOf(R), free = sceneOf(R), a = stubRenderer(), h = stubRenderer({ hostOnly: true });
        a.attach(s); s.rotate(q); free.rotate(q);
        h.attach(s);                               // (its upload reads the arrays: the mirrors are refreshed for it)
        check("host_only_attach_sees_edits", a.calls.read === 1 && same(h.twin.positions, free.positions));
        s.scale(sc); free.scale(sc);
        check("host_only_forces_js_path", a.calls.transform === 1 && h.calls.transform === 0 && a.calls.upload === 2 && h.calls.upload === 2 && equalScenes(s, free));
    }
    {   // argument errors of limitBox: same messages, before anything runs
        const s = sceneOf(R), free = sceneOf(R), a = stubRenderer();
        a.attach(s);
        const msg = (sc2, args) => { try { sc2.limitBox(...args); return null; } catch (e) { return e.message; } };
        let ok = true;
        for (const args of [[1, 1, 0, 1, 0, 1], [0, 1, 2, 1, 0, 1], [0, 1, 0, 1, 3, -3]]) ok = ok && msg(s, args) !== null && msg(s, args) === msg(free, args);
        check("limitbox_errors_unchanged", ok && a.calls.transform === 0 && s._stale === false);
        const liar = stubRenderer({ lie: true });
        liar.attach(s);
        let threw = false;
        try { s.translate(t); } catch (e) { threw = /disagree/.test(e.message); }
        check("count_disagreement_throws", threw);
    }
    {   // any sequence: the bound scene's arrays equal the unbound scene's, bit for bit
        let seed = 12345, ok = true, edits = 0;
        const rnd = () => ((seed = (Math.imul(seed, 1103515245) + 12345) >>> 0) / 4294967296);
        for (let round = 0; round < 6 && ok; round++) {
            const Rr = rows(200 + round * 331, 100 + round), s = sceneOf(Rr), free = sceneOf(Rr);
            if (round & 1) { s.rotate(q); free.rotate(q); s.scale(sc); free.scale(sc); }      // edited on the host before its first frame
            const rs = [stubRenderer(), stubRenderer(), stubRenderer()];
            rs[0].attach(s); if (round > 2) rs[1].attach(s);
            for (let step = 0; step < 40 && ok; step++) {
                const k = Math.floor(rnd() * 9);
                const v = new G.Vector3(rnd() * 2 - 1, rnd() * 2 - 1, rnd() * 2 - 1);
                if (k === 0) { s.translate(v); free.translate(v); edits++; }
                else if (k === 1) { const e = G.Quaternion.FromEuler(v); s.rotate(e); free.rotate(e); edits++; }
                else if (k === 2) { const f = new G.Vector3(0.8 + rnd() * 0.5, 0.8 + rnd() * 0.5, 0.8 + rnd() * 0.5); s.scale(f); free.scale(f); edits++; }
                else if (k === 3) { const b = 2.5 + rnd() * 3; s.limitBox(-b, b, -b, b, -b, b); free.limitBox(-b, b, -b, b, -b, b); edits++; }
                else if (k === 4) ok = ok && equalScenes(s, free);
                else if (k === 5) { const i = Math.floor(rnd() * s.vertexCount) * 3; if (s.vertexCount) { s.positions[i] += 0.5; free.positions[i] += 0.5; s._writePosition(i / 3); free._writePosition(i / 3); s.dispatchEvent({ type: "change" }); } }
                else if (k === 6) { s.scales = s.scales.slice(); }
                else if (k === 7) { if (rs[2].dev && !s._devices.includes(rs[2].dev)) rs[2].attach(s); else rs[2].detach(); }
                else { const Rn = rows(150 + step, step); s.setData(Rn); free.setData(Rn); }
            }
            ok = ok && equalScenes(s, free);
            for (const r of rs) if (s._devices.includes(r.dev)) r.detach();
            ok = ok && s._devices.length === 0 && s._stale === false && same(raw(s).positions, free.positions) && same(raw(s).data, free.data, 8 * free.vertexCount);
        }
        check("random_sequences_equal_unbound", ok && edits > 60);
    }
    console.log(JSON.stringify({ checks, failed }));
} else {
    console.error("usage: scene_binding_check.js protocol");
    process.exit(2);
}
