#!/usr/bin/env node
// Driver of tests/test_gpu_scene_binding.py: a Scene attached to real renderers.  Every comparison is bit for bit and made here,
// against a Scene that no renderer ever saw (`free`) and fresh renderers that are handed copies of it.
//   node scene_device_check.js edits | roundrobin | sh | delivery   -> one JSON line { checks: [...names], failed: [...names] }
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
        for (let k = 0; k < 3; k++) { f[8 * i + k] = (rnd() - 0.5) * 5; f[8 * i + 3 + k] = 0.01 + rnd() * 0.08; }
        for (let k = 24; k < 32; k++) out[32 * i + k] = Math.floor(rnd() * 256);
    }
    return out;
}
const W = 640, H = 480, FX = 560;
function camera(k) {
    const cam = new G.Camera(undefined, undefined, FX, FX);
    G.OrbitControls.applyPose(cam, (2 * Math.PI * k) / 120, 0.3, 8, new G.Vector3(0, 0, 0));
    return cam;
}
// what a fresh renderer is given: data and positions only, through the plain setters (the upload the parent commit does)
function copyOf(s, withSh) {
    const c = new G.Scene();
    c.vertexCount = s.vertexCount; c.height = s.height;
    c.data = s.data.slice(); c.positions = s.positions.slice();
    if (withSh) { c.shs_rgb = s.shs_rgb; c.shHeight = s.shHeight; c.bandsIndices = s.bandsIndices; }
    return c;
}
function freshFrame(s, cam, withSh, throughput) {
    const r = new G.HIPRenderer({ width: W, height: H, throughput: !!throughput }, []);
    r.render(copyOf(s, withSh), cam);
    const out = { pixels: r.readPixels(), order: r.lastDepthIndex() };
    r.dispose();
    return out;
}
const equalScenes = (a, b) => a.vertexCount === b.vertexCount && a.height === b.height && a.data.length === b.data.length &&
    same(a.data, b.data, 8 * a.vertexCount) && same(a.positions, b.positions) && same(a.rotations, b.rotations) && same(a.scales, b.scales);
const q = G.Quaternion.FromEuler(new G.Vector3(0.1, -0.7, 0.3)), t = new G.Vector3(0.25, -0.5, 1), sc = new G.Vector3(1.1, 0.9, 1.3);
const mode = process.argv[2];

if (mode === "edits") {
    const R = rows(20000, 3), s = new G.Scene(), free = new G.Scene();
    let events = 0;
    s.addEventListener("change", () => events++);
    s.setData(R); free.setData(R);
    s.rotate(q); free.rotate(q); s.scale(sc); free.scale(sc);          // on the host, before the first frame
    const r = new G.HIPRenderer({ width: W, height: H }, []);
    const cam = camera(7);
    const frameEquals = () => {
        r.render(s, cam);
        const f = freshFrame(free, cam);
        return same(r.readPixels(), f.pixels) && same(r.lastDepthIndex(), f.order);
    };
    check("first_frame_of_a_scene_edited_on_the_host", frameEquals());
    const edits = [["rotate", (x) => x.rotate(G.Quaternion.FromEuler(new G.Vector3(-0.4, 0.2, 0.9)))], ["translate", (x) => x.translate(t)],
                   ["scale", (x) => x.scale(new G.Vector3(0.9, 1.2, 1.05))], ["limitBox", (x) => x.limitBox(-2, 2.2, -1.8, 2, -2.5, 1.9)]];
    for (const [name, edit] of edits) {
        const before = events;
        edit(s); edit(free);
        check(name + "_count_and_one_change", s.vertexCount === free.vertexCount && s.height === free.height && events === before + 1 && s._stale === true);
        check(name + "_frame", frameEquals());
        check(name + "_arrays", equalScenes(s, free));
    }
    check("limitbox_kept_some", s.vertexCount > 0 && s.vertexCount < 20000);
    // an edit waits on the device while the renderer goes away: the scene gets it back
    s.translate(t); free.translate(t);
    r.dispose();
    check("dispose_hands_the_edit_back", s._stale === false && s._devices.length === 0 && equalScenes(s, free));
    // a scene whose buffers were assigned by hand renders through the host path, and its edits too
    const hand = copyOf(free), r2 = new G.HIPRenderer({ width: W, height: H }, []);
    r2.render(hand, cam);
    check("hand_assigned_scene_is_host_only", hand._devices.length === 1 && hand._devices[0].hostOnly === true && same(r2.readPixels(), freshFrame(free, cam).pixels));
    r2.dispose();
    console.log(JSON.stringify({ checks, failed }));
} else if (mode === "roundrobin") {
    const R = rows(20000, 4), s = new G.Scene(), free = new G.Scene();
    s.setData(R); free.setData(R);
    const rs = [0, 1, 2].map(() => new G.HIPRenderer({ width: W, height: H, throughput: true }, []));
    const dq = G.Quaternion.FromEuler(new G.Vector3(0, 0.05, 0.01));
    let ok = true, orders = true;
    for (let lap = 0; lap < 3; lap++) {
        const want = [];
        for (let j = 0; j < 3; j++) {          // three frames in flight, an edit (on all three contexts) in front of each
            s.rotate(dq); free.rotate(dq);
            const cam = camera(3 * lap + j);
            rs[j].renderAsync(s, cam);
            want.push(freshFrame(free, cam, false, true));   // (the same kind of context: bit for bit)
            // (the permutation is read before the next edit: an edit withdraws the order and the depth planes of the frame in
            // front of it, as any scene change does; the pixels stay readable)
            if (lap === 2) orders = orders && same(rs[j].lastDepthIndex(), want[j].order);
        }
        for (let j = 0; j < 3; j++) ok = ok && same(rs[j].readPixels(), want[j].pixels);
    }
    check("round_robin_permutations", orders);
    check("every_round_robin_frame_equals_a_synchronous_one", ok);
    check("all_three_attached", s._devices.length === 3 && s._stale === true);
    check("arrays_after_nine_edits", equalScenes(s, free));
    rs[0].dispose(); rs[1].dispose();
    s.rotate(dq); free.rotate(dq);
    rs[2].dispose();
    check("last_renderer_hands_the_edit_back", s._stale === false && equalScenes(s, free));
    console.log(JSON.stringify({ checks, failed }));
} else if (mode === "sh") {
    const n = 6000, first = 1500, R = rows(n, 6);
    let z = 99;
    const shs = new Float32Array((n - first) * 48).map(() => ((z = (Math.imul(z, 1103515245) + 12345) >>> 0) / 4294967296 - 0.5) * 0.8);
    const make = () => { const x = new G.Scene(); x.bandsIndices = new Int32Array([first - 1, 3000, 4500]); x.setData(R, shs); return x; };
    const s = make(), free = make(), cam = camera(11);
    const r = new G.HIPRenderer({ width: W, height: H }, []);
    r.render(s, cam);
    check("sh_first_frame", same(r.readPixels(), freshFrame(free, cam, true).pixels));
    check("sh_colours_are_used", !same(r.readPixels(), freshFrame(free, cam, false).pixels));
    s.rotate(q); free.rotate(q);
    r.render(s, cam);
    check("sh_after_rotate_equals_a_reupload", same(r.readPixels(), freshFrame(free, cam, true).pixels));
    let threw = null;
    try {
        s.limitBox(-2, 2, -2, 2, -2, 2); free.limitBox(-2, 2, -2, 2, -2, 2);
        r.render(s, cam);
        r.setShTextures();
        r.render(s, cam);
    } catch (e) { threw = e.message; }
    check("sh_limitbox_does_not_throw", threw === null && s.shDroppedOnDevice === true);
    check("sh_limitbox_renders_rgba8_colours", same(r.readPixels(), freshFrame(free, cam, false).pixels) && s.vertexCount === free.vertexCount);
    s.setData(R, shs);
    r.render(s, cam);
    check("sh_back_after_setData", s.shDroppedOnDevice === false && same(r.readPixels(), freshFrame(make(), cam, true).pixels));
    r.dispose();
    console.log(JSON.stringify({ checks, failed }));
} else if (mode === "delivery") {
    const R = rows(20000, 8), s = new G.Scene(), free = new G.Scene();
    s.setData(R); free.setData(R);
    const r = new G.HIPRenderer({ width: W, height: H }, []), cam = camera(5);
    r.openDelivery(3);
    r.renderAsync(s, cam);
    const k1 = r.deliverFrame();
    const want1 = freshFrame(free, cam).pixels;
    s.rotate(q); free.rotate(q);                    // the ring stays open across the edit
    r.renderAsync(s, cam);
    const k2 = r.deliverFrame();
    const f1 = r.acquireFrame(k1);
    check("frame_before_the_edit", same(f1.pixels, want1));
    f1.release();
    const f2 = r.acquireFrame(k2);
    check("frame_after_the_edit", same(f2.pixels, freshFrame(free, cam).pixels));
    f2.release();
    r.closeDelivery();
    r.render(s, cam);
    r.readDepth();
    s.translate(t);
    let refused = false;
    try { r.readDepth(); } catch (e) { refused = true; }
    check("readDepth_after_an_edit_without_a_frame_is_refused", refused);
    r.render(s, cam);
    let ok = true;
    try { r.readDepth(); } catch (e) { ok = false; }
    check("readDepth_after_the_next_frame", ok);
    r.dispose();
    console.log(JSON.stringify({ checks, failed }));
} else {
    console.error("usage: scene_device_check.js edits | roundrobin | sh | delivery");
    process.exit(2);
}
