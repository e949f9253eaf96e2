"use strict";
// Scene container: API of src/core/Scene.ts.  setData() is the producer of the two buffers the render hot path
// consumes -- `positions` (f32 x 3N, read by the depth sort) and `data` (8 u32 per splat: position bits, six
// truncated halves of 4*Sigma, rgba8; the reference's RGBA32UI texture image) -- so its f64 arithmetic follows
// Scene.ts:126-177 operation for operation.  translate/rotate/scale/limitBox mutate the same buffers and fire
// "change", which makes the renderer re-upload (WebGLRenderer.ts:234-239).
//
// While the scene is attached to renderers (attachDevice), the device copies are the scene: the four transforms run on
// every attached *device scene* -- { transform(kind, Float64Array) -> vertexCount, read({data, positions, rotations,
// scales}), hostOnly } -- instead of the loops below, nothing is uploaded, and the four arrays become mirrors that are
// refreshed from the first device scene the next time they are read.  The Scene knows nothing else of a renderer, so
// the protocol runs against a stub as well (tests/test_scene_binding.py).  DESIGN.md section 4, "Scene transforms on
// the device".  Device scenes that carry the same `share` token (an object identity; renderers whose contexts share one
// device copy, gsr_share_scene) are one scene: an edit or an option is issued once per distinct token, through the
// first of them in attach order; a device scene without a token counts singly.
const { EventDispatcher } = require("./EventDispatcher");
const { Matrix3 } = require("../math/Matrix3");
const { Quaternion } = require("../math/Quaternion");
const { Vector3 } = require("../math/Vector3");
const { packHalf2x16 } = require("../utils");

const ROW = 32;        // bytes per .splat row (Scene.ts:9)
const TEX_WIDTH = 2048; // texels per data-texture row, 2 texels per splat (Scene.ts:47)

class Scene extends EventDispatcher {
    constructor() {
        super();
        this._data = new Uint32Array(0);
        this._vertexCount = 0;
        this._width = TEX_WIDTH;
        this._height = 0;
        this._shHeight = 0;
        this._positions = new Float32Array(0);
        this._rotations = new Float32Array(0);
        this._scales = new Float32Array(0);
        this._shs = new Uint32Array(0);
        this._shs_rgb = [new Uint32Array(0), new Uint32Array(0), new Uint32Array(0)];
        this._g0bands = 0;
        this._bandsIndices = new Int32Array([-1, -1, -1]);
        this._devices = [];            // attached device scenes, in attach order
        this._stale = false;           // the device copies hold edits the four arrays have not seen
        this._diverged = false;        // a plain setter replaced a buffer: the device copies are behind until the next "change"
        this._editOnDevice = false;    // true while the "change" of an edit the devices have applied is dispatched
        this._shDroppedOnDevice = false;
        // SH colour that follows the transforms (opt-in; DESIGN.md section 4, "SH frame"): shFrame is the inverse of the linear part
        // of every rotate / scale since setData, row-major; with the option on, limitBox compacts shs_rgb and recounts bandsIndices
        // (on the device while attached: the three then are mirrors like the four arrays, refreshed on first read).
        this._shFollowsTransforms = false;
        this._shFrame = new Float64Array([1, 0, 0, 0, 1, 0, 0, 0, 1]);
        this._shStale = false;         // the device compacted the SH state and shs_rgb / shHeight / bandsIndices have not seen it
        // A "change" that is not a device edit's (setData, an edit that ran here, one the caller dispatched after writing into
        // the arrays) makes every attached renderer upload the host's arrays: afterwards the device copies are current again.
        const dispatch = this.dispatchEvent;
        this.dispatchEvent = (e) => {
            dispatch(e);
            if (e.type === "change" && !this._editOnDevice) this._diverged = false;
        };
    }

    // ---- binding to device scenes ----
    attachDevice(dev) {
        if (this._devices.includes(dev)) return;
        this._devices.push(dev);
        if (dev.setShFollow) dev.setShFollow(this._shFollowsTransforms);
    }
    // one device scene per distinct device copy, in attach order
    _distinctDevices() {
        const seen = new Set();
        return this._devices.filter((d) => {
            if (!d.share) return true;
            if (seen.has(d.share)) return false;
            seen.add(d.share);
            return true;
        });
    }
    // (for the renderers) false while a plain setter has replaced a buffer and no "change" has made the attached renderers upload it yet
    get _devicesCurrent() { return !this._diverged; }
    // The last device scene to go hands its edits back first, so the scene never loses one.
    detachDevice(dev) {
        const k = this._devices.indexOf(dev);
        if (k < 0) return;
        if (this._devices.length === 1) { this._refresh(); this._refreshSh(); this._diverged = false; }
        this._devices.splice(k, 1);
    }
    // true inside the "change" of an edit every attached device scene has applied already: a renderer has nothing to upload
    get deviceEditApplied() { return this._editOnDevice; }
    // limitBox on the device renumbers the splats and drops the context's SH state; the SH textures here are stale from then
    // on, and are not sent again before the next setData
    get shDroppedOnDevice() { return this._shDroppedOnDevice; }

    // Mirrors in the shapes the loops below leave: arrays of the right length are filled in place, others are replaced (a
    // replaced `data` is zero behind 8 * vertexCount, where the limitBox loop leaves stale splats).
    _refresh() {
        if (!this._stale) return;
        const n = this._vertexCount, fit = (a, T, len) => (a.length === len ? a : new T(len));
        this._data = fit(this._data, Uint32Array, this._width * this._height * 4);
        this._positions = fit(this._positions, Float32Array, 3 * n);
        this._rotations = fit(this._rotations, Float32Array, 4 * n);
        this._scales = fit(this._scales, Float32Array, 3 * n);
        this._devices[0].read({ data: this._data, positions: this._positions, rotations: this._rotations, scales: this._scales });
        this._data.fill(0, 8 * n);
        this._stale = false;
    }

    // The SH mirrors after a limitBox the devices followed: 8 * shCount words per texture in front, zeros behind, as the loop
    // in limitBox leaves them.
    _refreshSh() {
        if (!this._shStale) return;
        this._shStale = false;
        const band = new Int32Array(3);
        const count = this._devices[0].readSh(null, band);
        this._shHeight = Math.ceil((2 * count) / this._width);
        this._shs_rgb = [0, 1, 2].map(() => new Uint32Array(this._width * this._shHeight * 4));
        if (count) this._devices[0].readSh(this._shs_rgb, band);
        this._bandsIndices = band;
    }

    // (for the renderers) a device copy rotated SH coefficients in place (rotateSH, rotateSelection { sh }, bakeSHFrame): shs_rgb is
    // read back before its next use, as after a followed limitBox; baked: the frame went into the coefficients and is the identity
    _deviceTurnedSh(baked) {
        if (this._shHeight > 0) this._shStale = true;
        if (baked) this._shFrame.set([1, 0, 0, 0, 1, 0, 0, 0, 1]);
    }

    get shFollowsTransforms() { return this._shFollowsTransforms; }
    set shFollowsTransforms(on) {
        this._shFollowsTransforms = !!on;
        for (const d of this._distinctDevices()) if (d.setShFollow) d.setShFollow(this._shFollowsTransforms);
    }
    get shFrame() { return this._shFrame; }

    // shFrame <- shFrame . R(q)^T, R as rotate builds it; every entry (a * b + c * d) + e * f
    _frameRotate(q) {
        const x = q.x, y = q.y, z = q.z, w = q.w, L = this._shFrame, out = new Float64Array(9);
        const R = [1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                   2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                   2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y];
        for (let i = 0; i < 3; i++)
            for (let j = 0; j < 3; j++) out[3 * i + j] = (L[3 * i] * R[3 * j] + L[3 * i + 1] * R[3 * j + 1]) + L[3 * i + 2] * R[3 * j + 2];
        L.set(out);
    }
    // shFrame <- shFrame . diag(1 / sx, 1 / sy, 1 / sz)
    _frameScale(f) {
        const L = this._shFrame;
        for (let i = 0; i < 3; i++)
            for (let j = 0; j < 3; j++) L[3 * i + j] = L[3 * i + j] * (1 / f[j]);
    }

    // kind: 0 translate (x, y, z), 1 rotate (x, y, z, w), 2 scale (x, y, z), 3 limitBox (xMin, xMax, yMin, yMax, zMin, zMax),
    // 4 eraseSelection ({ mask, keep }: the mask is set on the device copy, then erased there),
    // 5 translateSelection, 6 rotateSelection, 7 scaleSelection ({ mask, values, pivot }), 8 paintSelection ({ mask, rgba, byteMask }):
    // the mask is set on the device copy, then the splats it selects are edited there;
    // 9 duplicateSelection ({ mask, count }: the mask is set on the device copy, then the splats it selects are copied behind the last one there),
    // 10 append ({ data, positions, rotations, scales, count }: the rows go to the device copy through the upload's repack).
    // false: the edit has to run here (nothing attached, a host-only device scene among them, or buffers set by hand).
    _editDevices(kind, args) {
        // (a device scene that cannot follow SH -- no setShFollow / readSh -- counts as host-only while the option is on; so does
        //  one that cannot take a selection -- no setSelection / eraseSelected -- for an eraseSelection)
        const cannotFollow = this._shFollowsTransforms && this._devices.some((d) => !d.setShFollow || !d.readSh);
        const cannotErase = kind === 4 && this._devices.some((d) => !d.setSelection || !d.eraseSelected);
        const cannotEdit = kind >= 5 && kind <= 8 && this._devices.some((d) => !d.setSelection || !d.editSelected || !d.paintSelected);
        const cannotGrow = kind >= 9 && this._devices.some((d) => !d.setSelection || !d.duplicateSelected || !d.appendArrays);
        if (!this._devices.length || this._diverged || cannotFollow || cannotErase || cannotEdit || cannotGrow || this._devices.some((d) => d.hostOnly)) {
            this._refresh();
            this._refreshSh();
            return false;
        }
        const f = kind >= 4 ? null : new Float64Array(args);
        let count = -1;
        for (const d of this._distinctDevices()) {
            let c;
            if (kind === 4) { d.setSelection(args.mask); c = d.eraseSelected(args.keep); }
            else if (kind === 9) { d.setSelection(args.mask); c = d.duplicateSelected(); }   // (the copies are the copy's selection afterwards)
            else if (kind === 10) c = d.appendArrays(args.data, args.positions, args.rotations, args.scales, args.count);
            else if (kind >= 5) {   // the mask first, then the edit of what it selects; the count stays
                d.setSelection(args.mask);
                if (kind === 8) d.paintSelected(args.rgba, args.byteMask);
                else d.editSelected(kind - 5, new Float64Array(args.values), args.pivot ? new Float64Array(args.pivot) : null);
                c = this._vertexCount;
            }
            else c = d.transform(kind, f);
            if (count >= 0 && c !== count) throw new Error("device scenes disagree on vertexCount (" + count + " and " + c + ")");
            count = c;
        }
        this._vertexCount = count;
        this._height = Math.ceil((2 * count) / this._width);
        this._stale = true;
        if (kind === 3 || (kind === 4 && args.removes)) {   // (an erase that removes nothing leaves the device's SH state alone)
            if (this._shFollowsTransforms) this._shStale = this._shStale || this._shHeight > 0;   // compacted with the scene over there
            else this._shDroppedOnDevice = true;
        }
        this._editOnDevice = true;
        try { this.dispatchEvent({ type: "change" }); } finally { this._editOnDevice = false; }
        return true;
    }

    // 4*Sigma of splat i from its rotation/scale, packed as six truncated halves (Scene.ts:150-176)
    _packCovariance(i) {
        const r = this._rotations, s = this._scales;
        const rot = Matrix3.RotationFromQuaternion(new Quaternion(r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], -r[4 * i]));
        const M = Matrix3.Diagonal(new Vector3(s[3 * i], s[3 * i + 1], s[3 * i + 2])).multiply(rot).buffer;
        const d = this._data;
        d[8 * i + 4] = packHalf2x16(4 * (M[0] * M[0] + M[3] * M[3] + M[6] * M[6]), 4 * (M[0] * M[1] + M[3] * M[4] + M[6] * M[7]));
        d[8 * i + 5] = packHalf2x16(4 * (M[0] * M[2] + M[3] * M[5] + M[6] * M[8]), 4 * (M[1] * M[1] + M[4] * M[4] + M[7] * M[7]));
        d[8 * i + 6] = packHalf2x16(4 * (M[1] * M[2] + M[4] * M[5] + M[7] * M[8]), 4 * (M[2] * M[2] + M[5] * M[5] + M[8] * M[8]));
    }

    _writePosition(i) {
        const f = new Float32Array(this._data.buffer, this._data.byteOffset, this._data.length);
        f[8 * i] = this._positions[3 * i];
        f[8 * i + 1] = this._positions[3 * i + 1];
        f[8 * i + 2] = this._positions[3 * i + 2];
    }

    // One splat of translate / rotate / scale (Scene.ts:182-305), for the selection's edits below: the bodies of the whole-scene
    // loops, which stay exactly as they were.  Held to the same reference bit for bit by tests/test_edit_binding.py.
    // R: Matrix3.RotationFromQuaternion(rotation).buffer; f: [sx, sy, sz].
    _translateOne(i, x, y, z) {
        this._positions[3 * i] += x;
        this._positions[3 * i + 1] += y;
        this._positions[3 * i + 2] += z;
        this._writePosition(i);
    }
    _rotateOne(i, R, rotation) {
        const p = this._positions, r = this._rotations;
        const x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        p[3 * i] = R[0] * x + R[1] * y + R[2] * z;
        p[3 * i + 1] = R[3] * x + R[4] * y + R[5] * z;
        p[3 * i + 2] = R[6] * x + R[7] * y + R[8] * z;
        this._writePosition(i);
        const q = rotation.multiply(new Quaternion(r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], r[4 * i]));
        r[4 * i + 1] = q.x; r[4 * i + 2] = q.y; r[4 * i + 3] = q.z; r[4 * i] = q.w;
        this._packCovariance(i);
    }
    _scaleOne(i, f) {
        for (let k = 0; k < 3; k++) {
            this._positions[3 * i + k] *= f[k];
            this._scales[3 * i + k] *= f[k];
        }
        this._writePosition(i);
        this._packCovariance(i);
    }

    // data: Uint8Array of 32-byte rows [pos f32x3 | scale f32x3 | rgba u8x4 | rot u8x4 (w,x,y,z)].
    // shs (48 floats per SH-carrying splat) is packed into three half textures exactly like Scene.ts:108-124.
    setData(data, shs) {
        if (data.length % ROW) throw new Error("splat data length must be a multiple of " + ROW);
        const n = data.length / ROW;
        this._stale = false;            // the host is the truth again: whatever the devices hold is replaced by the upload
        this._shDroppedOnDevice = false;
        this._shStale = false;
        this._shFrame.set([1, 0, 0, 0, 1, 0, 0, 0, 1]);
        this._vertexCount = n;
        this._height = Math.ceil((2 * n) / this._width);
        this._data = new Uint32Array(this._width * this._height * 4);
        this._positions = new Float32Array(3 * n);
        this._rotations = new Float32Array(4 * n);
        this._scales = new Float32Array(3 * n);
        const bytes = data.byteOffset % 4 === 0 ? data : new Uint8Array(data);  // aligned view for the f32 reads
        const rowF = new Float32Array(bytes.buffer, bytes.byteOffset, n * 8);
        if (shs !== undefined) {
            const shCount = n - (this._bandsIndices[0] + 1);
            this._shHeight = Math.ceil((2 * shCount) / this._width);
            this._shs_rgb = [0, 1, 2].map(() => new Uint32Array(this._width * this._shHeight * 4));
            for (let i = 0; i < shCount; i++)
                for (let j = 0, src = i * 48; j < 8; j++, src += 6)
                    for (let c = 0; c < 3; c++) this._shs_rgb[c][8 * i + j] = packHalf2x16(shs[src + c], shs[src + 3 + c]);
        }
        const out8 = new Uint8Array(this._data.buffer);
        for (let i = 0; i < n; i++) {
            for (let k = 0; k < 3; k++) {
                this._positions[3 * i + k] = rowF[8 * i + k];
                this._scales[3 * i + k] = rowF[8 * i + 3 + k];
            }
            for (let k = 0; k < 4; k++) {
                this._rotations[4 * i + k] = (bytes[ROW * i + 28 + k] - 128) / 128;
                out8[4 * (8 * i + 7) + k] = bytes[ROW * i + 24 + k];
            }
            this._writePosition(i);
            this._packCovariance(i);
        }
        this.dispatchEvent({ type: "change" });
    }

    translate(t) {
        if (this._editDevices(0, [t.x, t.y, t.z])) return;
        for (let i = 0; i < this._vertexCount; i++) {
            this._positions[3 * i] += t.x;
            this._positions[3 * i + 1] += t.y;
            this._positions[3 * i + 2] += t.z;
            this._writePosition(i);
        }
        this.dispatchEvent({ type: "change" });
    }

    rotate(rotation) {
        if (this._shFollowsTransforms) this._frameRotate(rotation);   // (the devices keep their own: gsr_set_sh_follow)
        if (this._editDevices(1, [rotation.x, rotation.y, rotation.z, rotation.w])) return;
        const R = Matrix3.RotationFromQuaternion(rotation).buffer;
        const p = this._positions, r = this._rotations;
        for (let i = 0; i < this._vertexCount; i++) {
            const x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
            p[3 * i] = R[0] * x + R[1] * y + R[2] * z;
            p[3 * i + 1] = R[3] * x + R[4] * y + R[5] * z;
            p[3 * i + 2] = R[6] * x + R[7] * y + R[8] * z;
            this._writePosition(i);
            const q = rotation.multiply(new Quaternion(r[4 * i + 1], r[4 * i + 2], r[4 * i + 3], r[4 * i]));
            r[4 * i + 1] = q.x; r[4 * i + 2] = q.y; r[4 * i + 3] = q.z; r[4 * i] = q.w;
            this._packCovariance(i);
        }
        this.dispatchEvent({ type: "change" });
    }

    scale(s) {
        const f = [s.x, s.y, s.z];
        if (this._shFollowsTransforms) {
            for (const v of f) if (!(Number.isFinite(v) && v !== 0)) throw new Error("scale component " + v + ": with shFollowsTransforms a scale must be finite and not 0");
            this._frameScale(f);
        }
        if (this._editDevices(2, f)) return;
        for (let i = 0; i < this._vertexCount; i++) {
            for (let k = 0; k < 3; k++) {
                this._positions[3 * i + k] *= f[k];
                this._scales[3 * i + k] *= f[k];
            }
            this._writePosition(i);
            this._packCovariance(i);
        }
        this.dispatchEvent({ type: "change" });
    }

    limitBox(xMin, xMax, yMin, yMax, zMin, zMax) {
        if (xMin >= xMax) throw new Error("xMin (" + xMin + ") must be smaller than xMax (" + xMax + ")");
        if (yMin >= yMax) throw new Error("yMin (" + yMin + ") must be smaller than yMax (" + yMax + ")");
        if (zMin >= zMax) throw new Error("zMin (" + zMin + ") must be smaller than zMax (" + zMax + ")");
        if (this._editDevices(3, [xMin, xMax, yMin, yMax, zMin, zMax])) return;
        const p = this._positions;
        this._compact((i) => {
            const x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
            return x >= xMin && x <= xMax && y >= yMin && y <= yMax && z >= zMin && z <= zMax;
        });
    }

    // Remove the splats whose bit of `mask` is set -- splat i is bit i & 31 of word i >>> 5, the layout of the renderer's
    // readSelection() -- or, with { keep: true }, the others: order-preserving, with limitBox's bookkeeping (SH rows and
    // bandsIndices follow with shFollowsTransforms).  While device scenes are attached the mask is set on every distinct device
    // copy and erased there (gsr_selection_set, gsr_scene_erase_selected); otherwise the same loop runs here.  Fires "change".
    eraseSelection(mask, options) {
        const keep = !!(options && options.keep), n = this._vertexCount, words = Math.ceil(n / 32);
        if (!(mask instanceof Uint32Array) || mask.length < words) throw new Error("eraseSelection: mask must be a Uint32Array of at least " + words + " words");
        const bit = (i) => (mask[i >>> 5] >>> (i & 31)) & 1, want = keep ? 1 : 0;
        let kept = 0;
        for (let i = 0; i < n; i++) if (bit(i) === want) kept++;
        if (this._editDevices(4, { mask: mask, keep: keep, removes: kept < n })) return;
        if (kept < n) this._compact((i) => bit(i) === want);
        else this.dispatchEvent({ type: "change" });
    }

    // ---- editing a selection: translate, rotate, scale and recolour the splats whose bit of `mask` is set, and nothing else ----
    // The result is what translate / rotate / scale would leave in a Scene that held only those splats; with { pivot } (a
    // Vector3 or [x, y, z]) the operation is the three steps translate(-pivot), the operation, translate(+pivot) on them, each
    // rounded to f32 by the arrays it is stored into.  While device scenes are attached the mask is set on every distinct device
    // copy and the edit runs there (gsr_selection_set, gsr_scene_*_selected); otherwise the loops run here over the masked
    // indices.  Fires "change".  rotateSelection / scaleSelection throw while shFollowsTransforms is on and the scene has SH rows:
    // the SH frame is one per scene, and a partial rotation has none.
    _selectionArgs(what, mask, options, linear) {
        const n = this._vertexCount, words = Math.ceil(n / 32);
        if (!(mask instanceof Uint32Array) || mask.length < words) throw new Error(what + ": mask must be a Uint32Array of at least " + words + " words");
        if (linear && this._shFollowsTransforms && this.shHeight > 0)
            throw new Error(what + ": with shFollowsTransforms on and SH rows present a selection cannot be rotated or scaled (the SH frame is one per scene)");
        const p = options && options.pivot;
        return p ? (Array.isArray(p) || ArrayBuffer.isView(p) ? [p[0], p[1], p[2]] : [p.x, p.y, p.z]) : null;
    }
    // the host loop of an edit: `one(i)` on the masked splats, between the two translate steps when there is a pivot
    _editMasked(mask, pivot, one) {
        const n = this._vertexCount, bit = (i) => (mask[i >>> 5] >>> (i & 31)) & 1;
        if (pivot) for (let i = 0; i < n; i++) if (bit(i)) this._translateOne(i, -pivot[0], -pivot[1], -pivot[2]);
        for (let i = 0; i < n; i++) if (bit(i)) one(i);
        if (pivot) for (let i = 0; i < n; i++) if (bit(i)) this._translateOne(i, pivot[0], pivot[1], pivot[2]);
        this.dispatchEvent({ type: "change" });
    }
    translateSelection(mask, v) {
        this._selectionArgs("translateSelection", mask, null, false);
        if (this._editDevices(5, { mask: mask, values: [v.x, v.y, v.z], pivot: null })) return;
        this._editMasked(mask, null, (i) => this._translateOne(i, v.x, v.y, v.z));
    }
    rotateSelection(mask, q, options) {
        const pivot = this._selectionArgs("rotateSelection", mask, options, true);
        if (this._editDevices(6, { mask: mask, values: [q.x, q.y, q.z, q.w], pivot: pivot })) return;
        const R = Matrix3.RotationFromQuaternion(q).buffer;
        this._editMasked(mask, pivot, (i) => this._rotateOne(i, R, q));
    }
    scaleSelection(mask, s, options) {
        const pivot = this._selectionArgs("scaleSelection", mask, options, true), f = [s.x, s.y, s.z];
        for (const v of f) if (!Number.isFinite(v)) throw new Error("scaleSelection: scale component " + v + " must be finite");
        if (this._editDevices(7, { mask: mask, values: f, pivot: pivot })) return;
        this._editMasked(mask, pivot, (i) => this._scaleOne(i, f));
    }
    // rgba: { r, g, b, a } bytes 0..255; absent channels are left alone.  The word is data[8i + 7]: r, g, b in the low three bytes,
    // opacity in the top one (splats that take their colour from SH show only the opacity).
    paintSelection(mask, rgba) {
        this._selectionArgs("paintSelection", mask, null, false);
        const [value, byteMask] = Scene.rgbaWord(rgba);
        if (this._editDevices(8, { mask: mask, rgba: value, byteMask: byteMask })) return;
        const d = this._data;
        this._editMasked(mask, null, (i) => { d[8 * i + 7] = (d[8 * i + 7] & ~byteMask) | value; });
    }
    // ---- growing the scene: copies of the masked splats, or another Scene's splats, behind the last one ----
    // duplicateSelection(mask): the splats whose bit of `mask` is set, in ascending order, copied bit for bit behind the last splat;
    // append(other): all of another Scene's splats likewise (its SH rows are not carried: the copies keep their rgba word).  Existing
    // indices do not move.  While device scenes are attached the call is issued once per distinct device copy (gsr_selection_set +
    // gsr_scene_duplicate_selected, gsr_scene_append_arrays), where the new splats become the selection; otherwise the four arrays are
    // concatenated here.  Both return { first, count }, fire "change", and throw while the scene has SH rows: SH rows are indexed by
    // splat order, and a splat appended at the tail would have none to read.
    duplicateSelection(mask) {
        const n = this._vertexCount, words = Math.ceil(n / 32);
        if (!(mask instanceof Uint32Array) || mask.length < words) throw new Error("duplicateSelection: mask must be a Uint32Array of at least " + words + " words");
        if (this.shHeight > 0) throw new Error("duplicateSelection: the scene has SH rows (a splat appended at the tail would have no SH row)");
        const idx = [];
        for (let i = 0; i < n; i++) if ((mask[i >>> 5] >>> (i & 31)) & 1) idx.push(i);
        if (!this._editDevices(9, { mask: mask, count: idx.length })) this._appendRows(this._data, this._positions, this._rotations, this._scales, idx);
        return { first: n, count: idx.length };
    }
    append(other) {
        if (!(other instanceof Scene) || other === this) throw new Error("append: another Scene is needed");
        if (this.shHeight > 0) throw new Error("append: the scene has SH rows (a splat appended at the tail would have no SH row)");
        const m = other.vertexCount, data = other.data, positions = other.positions, rotations = other.rotations, scales = other.scales;
        if (data.length < 8 * m || positions.length !== 3 * m || rotations.length !== 4 * m || scales.length !== 3 * m)
            throw new Error("append: the other scene needs positions, rotations and scales of its vertexCount");
        const n = this._vertexCount, idx = [];
        for (let i = 0; i < m; i++) idx.push(i);
        if (!this._editDevices(10, { data: data, positions: positions, rotations: rotations, scales: scales, count: m })) this._appendRows(data, positions, rotations, scales, idx);
        return { first: n, count: m };
    }
    // the host loop of both: rows idx of the given arrays behind this scene's last row.  Rows travel through set() between arrays of
    // one type, which copies bytes: a NaN keeps its payload.
    _appendRows(data, positions, rotations, scales, idx) {
        const n = this._vertexCount, total = n + idx.length, height = Math.ceil((2 * total) / this._width);
        const grow = (T, old, len, keep) => { const a = new T(len); a.set(old.subarray(0, keep)); return a; };
        const d = grow(Uint32Array, this._data, this._width * height * 4, 8 * n), p = grow(Float32Array, this._positions, 3 * total, 3 * n);
        const r = grow(Float32Array, this._rotations, 4 * total, 4 * n), s = grow(Float32Array, this._scales, 3 * total, 3 * n);
        idx.forEach((i, j) => {
            d.set(data.subarray(8 * i, 8 * i + 8), 8 * (n + j));
            p.set(positions.subarray(3 * i, 3 * i + 3), 3 * (n + j));
            r.set(rotations.subarray(4 * i, 4 * i + 4), 4 * (n + j));
            s.set(scales.subarray(3 * i, 3 * i + 3), 3 * (n + j));
        });
        this._data = d; this._positions = p; this._rotations = r; this._scales = s;
        this._vertexCount = total;
        this._height = height;
        this.dispatchEvent({ type: "change" });
    }

    // { r, g, b, a } -> [word with the present channels' bytes, mask of their bytes]
    static rgbaWord(rgba) {
        let value = 0, byteMask = 0;
        ["r", "g", "b", "a"].forEach((ch, k) => {
            const v = rgba ? rgba[ch] : undefined;
            if (v === undefined || v === null) return;
            if (!Number.isInteger(v) || v < 0 || v > 255) throw new Error("paintSelection: " + ch + " must be an integer in 0..255");
            value |= v << (8 * k);
            byteMask |= 0xff << (8 * k);
        });
        return [value >>> 0, byteMask >>> 0];
    }

    // Hide the splats whose bit of `mask` is set (the layout of the renderer's readHidden() / readSelection()); null shows all.
    // The hidden set exists on the device copies only -- the four arrays do not change and no "change" fires -- so the set is
    // issued once per distinct device copy (gsr_hidden_set), as eraseSelection issues its mask, and the call throws when there is
    // no copy, when the copies are behind the arrays (an upload leaves nothing hidden), or when one cannot take it.
    setHidden(mask) {
        const words = Math.ceil(this._vertexCount / 32);
        if (mask !== null && (!(mask instanceof Uint32Array) || mask.length < words)) throw new Error("setHidden: mask must be null or a Uint32Array of at least " + words + " words");
        if (!this._devices.length) throw new Error("setHidden: no renderer holds this scene (the hidden set lives on the device copies)");
        if (this._diverged) throw new Error("setHidden: the device copies are behind the scene's arrays (dispatch 'change' first)");
        if (this._devices.some((d) => !d.setHidden)) throw new Error("setHidden: a device scene cannot take a hidden set");
        let count = -1;
        for (const d of this._distinctDevices()) count = d.setHidden(mask);
        return count;
    }

    // limitBox's loop over its predicate: the splats `stays` keeps move to the front of the four arrays in order; with
    // shFollowsTransforms the SH rows of the kept splats move up with them, and bandsIndices'[k] = (kept splats with index <=
    // bandsIndices[k]) - 1
    _compact(stays) {
        const follow = this._shFollowsTransforms && this._shHeight > 0;
        const band = this._bandsIndices, first = band[0] + 1, below = [0, 0, 0], sh = this._shs_rgb;
        let kept = 0, shKept = 0;
        for (let i = 0; i < this._vertexCount; i++) {
            if (!stays(i)) continue;
            if (follow) {
                for (let k = 0; k < 3; k++) if (i <= band[k]) below[k]++;
                if (i >= first) {
                    for (let c = 0; c < 3; c++) sh[c].copyWithin(8 * shKept, 8 * (i - first), 8 * (i - first) + 8);
                    shKept++;
                }
            }
            this._data.copyWithin(8 * kept, 8 * i, 8 * i + 8);
            this._positions.copyWithin(3 * kept, 3 * i, 3 * i + 3);
            this._rotations.copyWithin(4 * kept, 4 * i, 4 * i + 4);
            this._scales.copyWithin(3 * kept, 3 * i, 3 * i + 3);
            kept++;
        }
        this._height = Math.ceil((2 * kept) / this._width);
        this._vertexCount = kept;
        this._data = new Uint32Array(this._data.buffer, 0, this._width * this._height * 4);
        this._positions = new Float32Array(this._positions.buffer, 0, 3 * kept);
        this._rotations = new Float32Array(this._rotations.buffer, 0, 4 * kept);
        this._scales = new Float32Array(this._scales.buffer, 0, 3 * kept);
        if (follow) {   // (no SH splat kept: the cleared state, as after a setData without shs)
            this._shHeight = Math.ceil((2 * shKept) / this._width);
            this._shs_rgb = sh.map((t) => { const o = new Uint32Array(this._width * this._shHeight * 4); o.set(t.subarray(0, 8 * shKept)); return o; });
            this._bandsIndices = shKept ? new Int32Array([below[0] - 1, below[1] - 1, below[2] - 1]) : new Int32Array([-1, -1, -1]);
        }
        this.dispatchEvent({ type: "change" });
    }

    // The 32-byte .splat rows of the current scene (what Scene.saveToFile downloads in a browser, Scene.ts:368-403).
    toSplatBytes() {
        this._refresh();
        const n = this._vertexCount;
        const out = new Uint8Array(n * ROW), outF = new Float32Array(out.buffer), src8 = new Uint8Array(this._data.buffer);
        for (let i = 0; i < n; i++) {
            for (let k = 0; k < 3; k++) {
                outF[8 * i + k] = this._positions[3 * i + k];
                outF[8 * i + 3 + k] = this._scales[3 * i + k];
            }
            for (let k = 0; k < 4; k++) {
                out[ROW * i + 24 + k] = src8[4 * (8 * i + 7) + k];
                out[ROW * i + 28 + k] = (this._rotations[4 * i + k] * 128 + 128) & 0xff;
            }
        }
        return out;
    }

    // Node replacement for the browser download: writes the rows with fs.
    saveToFile(name) { require("fs").writeFileSync(name, this.toSplatBytes()); }

    updateColor() {}
}

// plain accessors, as in Scene.ts:414-508.  Reading one of the four mirrors refreshes them first; assigning a buffer or a count
// makes the host the truth (the mirrors are refreshed first, so no edit is lost) and takes the scene off the device path until
// the next "change" has made the attached renderers upload it.
const MIRRORS = ["data", "positions", "rotations", "scales"], SH_MIRRORS = ["shs_rgb", "shHeight", "bandsIndices"], UPLOADED = MIRRORS.concat(["vertexCount", "height"]);
for (const k of ["data", "vertexCount", "width", "height", "positions", "rotations", "scales", "shs", "shs_rgb", "shHeight",
                 "g0bands", "bandsIndices"]) {
    const mirror = MIRRORS.includes(k), uploaded = UPLOADED.includes(k), shMirror = SH_MIRRORS.includes(k);
    Object.defineProperty(Scene.prototype, k, {
        get() { if (mirror) this._refresh(); if (shMirror) this._refreshSh(); return this["_" + k]; },
        set(v) {
            if (shMirror) this._refreshSh();
            if (uploaded) { this._refresh(); this._diverged = this._devices.length > 0; }
            this["_" + k] = v;
        },
        configurable: true,
    });
}
Scene.RowLength = ROW;
module.exports = { Scene };
