#!/usr/bin/env node
// Driver of tests/test_hide_binding.py: Scene.setHidden against stub device scenes.  Two of them carry the same `share` token and
// stand in front of ONE device copy; the third has no token and a copy of its own.  The mask must reach each distinct copy once,
// null must pass through as "show all", the arrays must not change and no "change" may fire; the call throws when no device
// scene is attached, when the copies are behind the arrays, when one cannot take a hidden set, and on a short mask.
//   node hide_binding_check.js   -> one JSON line { checks: [...names], failed: [...names] }
"use strict";
const path = require("path");
const G = require(path.join(__dirname, "..", "..", "gsplat.js_amd", "js"));

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
const popcount = (w, n) => { let c = 0; for (let i = 0; i < n; i++) c += (w[i >>> 5] >>> (i & 31)) & 1; return c; };

const N = 3000, WORDS = Math.ceil(N / 32);
const log = [];
function deviceScene(name, copy, share, bare) {
    const dev = { hostOnly: false, transform: () => N, read: () => { log.push(name + ":read"); } };
    if (!bare) dev.setHidden = (words) => { log.push(name + ":setHidden"); copy.words = words === null ? null : Uint32Array.from(words); return words === null ? 0 : popcount(words, N); };
    if (share !== undefined) dev.share = share;
    return dev;
}
{
    const s = new G.Scene();
    s.setData(rows(N));
    const mask = new Uint32Array(WORDS);
    for (let i = 0; i < N; i++) if ((7 * i + 3) % 5 < 2) mask[i >>> 5] |= 1 << (i & 31);
    check("no_device_throws", throws(() => s.setHidden(mask), "no renderer"));
    const token = {}, shared = { words: undefined }, single = { words: undefined };
    s.attachDevice(deviceScene("a", shared, token)); s.attachDevice(deviceScene("x", single)); s.attachDevice(deviceScene("b", shared, token));
    let changes = 0;
    s.addEventListener("change", () => { changes++; });
    const before = Uint32Array.from(s.data);
    log.length = 0;
    const count = s.setHidden(mask);
    check("set_once_per_distinct_copy", log.join(",") === "a:setHidden,x:setHidden");
    check("both_copies_hold_the_mask", [shared, single].every((c) => c.words && c.words.length === WORDS && c.words.every((w, k) => w === mask[k])));
    check("returns_the_hidden_count", count === popcount(mask, N) && count > 0 && count < N);
    check("arrays_unchanged_and_no_change_event", changes === 0 && s.vertexCount === N && s.data.every((w, k) => w === before[k]));
    log.length = 0;
    check("null_shows_all", s.setHidden(null) === 0 && shared.words === null && single.words === null && log.join(",") === "a:setHidden,x:setHidden");
    check("short_mask_throws", throws(() => s.setHidden(new Uint32Array(WORDS - 1)), "at least " + WORDS));
    check("not_a_mask_throws", throws(() => s.setHidden([1, 2, 3]), "Uint32Array"));
    s.attachDevice(deviceScene("bare", {}, undefined, true));
    log.length = 0;
    check("device_without_hidden_set_throws", throws(() => s.setHidden(mask), "cannot take") && log.length === 0);
}
{
    const s = new G.Scene();
    s.setData(rows(N));
    s.attachDevice(deviceScene("a", {}));
    s.positions = new Float32Array(s.positions);      // a plain setter: the device copies are behind until the next "change"
    check("diverged_copies_throw", throws(() => s.setHidden(null), "behind"));
    s.dispatchEvent({ type: "change" });
    check("current_again_after_change", s.setHidden(null) === 0);
}
process.stdout.write(JSON.stringify({ checks, failed }) + "\n");
