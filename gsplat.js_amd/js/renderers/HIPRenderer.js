"use strict";
// HIPRenderer: drop-in for the render path of src/renderers/WebGLRenderer.ts on an AMD MI355X.
//   renderer.render(scene, camera) = camera.update + depth sort + projection + front-to-back composite,
// all on one HIP stream through libgsplat_hip.so (see include/gsplat_hip.h).  Differences from the WebGL
// renderer, all forced by the missing browser: no `domElement`/`gl`; the image is read back with readPixels() /
// readPixelsFloat(); the sort is synchronous with the frame (the reference sorts in a worker and draws with a
// stale order until it finishes, WebGLRenderer.ts:105-110,223-229), so every frame is deterministic.
// There is no CPU fallback: the constructor throws if the addon or a GPU is missing.
const path = require("path");
const { FadeInPass } = require("./FadeInPass");
const { Vector3 } = require("../math/Vector3");
const { Quaternion } = require("../math/Quaternion");
const { Scene } = require("../core/Scene");

let native = null;
function loadNative() {
    if (!native) {
        try {
            native = require(path.join(__dirname, "..", "native", "gsplat_hip.node"));
        } catch (e) {
            throw new Error("gsplat_hip.node is not built or libgsplat_hip.so cannot be loaded (" + e.message +
                            "); run `python -c \"import __graft_entry__ as g; g.build()\"`");
        }
    }
    return native;
}

class HIPRenderer {
    // new HIPRenderer(canvasLike | options | null, shaderPasses | null)
    //   canvasLike: anything with numeric width/height (stands in for the HTMLCanvasElement of WebGLRenderer.ts:23)
    //   options: { width, height, device, earlyOutEps, band: [x0, x1], timing, throughput }
    //   (throughput: several renderers keep frames in flight on one device; see GSR_FLAG_THROUGHPUT)
    //   (shareSceneWith: another HIPRenderer of the same device; a Scene that one has attached is shared with it, not uploaded again)
    constructor(target, optionalShaderPasses) {
        const o = target || {};
        this._n = loadNative();
        this.width = o.width || 1920;
        this.height = o.height || 1080;
        const band = o.band || [0, 0];
        this._h = this._n.create({ device: o.device || 0, width: this.width, height: this.height,
                                   earlyOutEps: o.earlyOutEps || 0, bandX0: band[0], bandX1: band[1], timing: o.timing ? 1 : 0, throughput: o.throughput ? 1 : 0 });
        const passes = optionalShaderPasses || [];
        if (!optionalShaderPasses) passes.push(new FadeInPass());
        let activeScene = null, activeCamera = null, initialized = false, vertexCount = 0;
        const f32 = { view: new Float32Array(16), proj: new Float32Array(16), vp: new Float32Array(16) };

        // While a Scene is this renderer's active scene, the renderer is one of its device scenes (Scene.attachDevice): the
        // Scene's transforms run here as kernels on this context's stream, behind whatever frames it has in flight, and the
        // Scene reads its arrays back from here when somebody asks for them.  DESIGN.md section 4, "Scene transforms on the device".
        // Shared scenes (gsr_share_scene): renderers whose contexts render one device copy carry the same token, and the Scene
        // issues an edit once per token.  null: this renderer's scene is its own.
        this._shareToken = null;
        const self = this;
        const device = {
            get share() { return self._shareToken; },
            hostOnly: false,             // the last upload could not carry rotations / scales: edits run in JavaScript and upload
            transform: (kind, f64) => (vertexCount = this._n.sceneTransform(this._h, kind, f64)),
            read: (out) => this._n.readSceneArrays(this._h, out.data, out.positions, out.rotations, out.scales),
            // SH colour that follows the transforms (Scene.shFollowsTransforms): the context keeps frame and textures up itself
            setShFollow: (on) => this._n.setShFollow(this._h, on ? 1 : 0),
            readSh: (textures, band) => this._n.readSceneSh(this._h, textures ? textures[0] : null, textures ? textures[1] : null, textures ? textures[2] : null, band),
            // Scene.eraseSelection: the mask becomes the device copy's selection, then the copy is compacted there
            setSelection: (words) => this._n.setSelection(this._h, words, 0),
            eraseSelected: (keep) => (vertexCount = this._n.eraseSelected(this._h, keep ? 1 : 0)),
            // Scene.setHidden: the mask becomes the device copy's hidden set (null: nothing hidden)
            setHidden: (words) => this._n.setHidden(this._h, words, 0),
            // Scene.translateSelection / rotateSelection / scaleSelection / paintSelection: the mask becomes the device copy's
            // selection (setSelection), then the selected splats are edited there; kind 0 translate, 1 rotate, 2 scale
            editSelected: (kind, f64, pivot) => this._n.editSelected(this._h, kind, f64, pivot),
            paintSelected: (rgba, byteMask) => this._n.paintSelected(this._h, rgba, byteMask),
            // Scene.duplicateSelection / Scene.append: the mask becomes the device copy's selection and the selected splats are copied
            // behind the last one there; another Scene's four arrays are appended through the upload's repack.  Both return the new count.
            duplicateSelected: () => grown(this._n.duplicateSelected(this._h)),
            appendArrays: (data, positions, rotations, scales, m) => grown(this._n.appendArrays(this._h, data, positions, rotations, scales, m)),
        };
        const grown = (r) => (vertexCount = r.first + r.count);
        const upload = () => {   // initWebGL's scene part: worker init + texImage2D (WebGLRenderer.ts:105-110,185-195)
            const s = activeScene, n = s.vertexCount, positions = s.positions, rotations = s.rotations, scales = s.scales;
            void s.shs_rgb;              // (SH mirrors of a followed limitBox are read back before the upload clears the context's SH state)
            vertexCount = n;
            // a Scene whose buffers were assigned one by one (Scene.ts:474-496) may carry no rotations or scales
            device.hostOnly = !(positions.length === 3 * n && rotations.length === 4 * n && scales.length === 3 * n);
            if (device.hostOnly) this._n.setScene(this._h, s.data, positions, n);
            else this._n.setSceneArrays(this._h, s.data, positions, rotations, scales, n);
            this._shareToken = null;     // (an upload takes the context out of a share: the scene is its own again)
            this.setShTextures();
            for (const p of passes) p.init(this, null);
            initialized = true;
        };
        const onSceneChange = (e) => {          // WebGLRenderer.ts:234-239
            if (!activeScene.deviceEditApplied) {
                // the re-upload is made once per device copy too: the renderer named in shareSceneWith uploads, this one shares again
                if (shareAttached(e)) return;
                upload();
                uploadedFor = e;
                return;
            }
            vertexCount = activeScene.vertexCount;   // the edit ran here already: nothing to upload; the passes start over as after an upload
            for (const p of passes) p.init(this, null);
        };
        // { shareSceneWith: other }: a Scene `other` has attached, with its device copy current, is shared instead of uploaded
        const shareFrom = (other) => {
            vertexCount = this._n.shareScene(this._h, other._h);
            this._shareToken = other._shareToken || (other._shareToken = {});
        };
        // `forEvent`: inside a "change" that makes the renderers upload -- then only behind `other`'s upload for this very event
        // (whichever order the listeners run in, this renderer never shares a copy that is about to be replaced)
        let uploadedFor = null;
        const shareAttached = (forEvent) => {
            const other = o.shareSceneWith;
            if (!other || !other._h || !other._attached) return false;
            const st = other._attached();
            if (st.scene !== activeScene || st.hostOnly) return false;
            if (forEvent ? st.uploadedFor !== forEvent : !activeScene._devicesCurrent) return false;
            shareFrom(other);
            device.hostOnly = false;
            if (!this._n.readSceneSh(this._h, null, null, null, new Int32Array(3))) this.setShTextures();   // (only if the share carried no SH)
            for (const p of passes) p.init(this, null);
            initialized = true;
            return true;
        };
        this._attached = () => ({ scene: activeScene, hostOnly: device.hostOnly, uploadedFor: uploadedFor });
        const detach = () => {
            if (!activeScene) return;
            activeScene.removeEventListener("change", onSceneChange);
            activeScene.detachDevice(device);
            activeScene = null;
        };
        const attach = (scene) => {
            if (scene === activeScene) return;
            detach();
            activeScene = scene;
            scene.addEventListener("change", onSceneChange);
            if (!shareAttached()) upload();
            scene.attachDevice(device);
        };

        // ---- frame delivery: finished RGBA8 frames through the library's pinned ring while the next frames render ----
        //   renderer.openDelivery(3);
        //   renderer.renderAsync(scene, camera); const k = renderer.deliverFrame();   // no host wait; throws when the ring is full
        //   ... further frames ...
        //   const f = renderer.acquireFrame(k);   // waits for THAT frame's copy only; f.pixels: Uint8Array, width*height*4
        //   present(f.pixels); f.release();       // the slot may be reused
        // `pixels` is a view of the slot's pinned block: one external ArrayBuffer per slot, created when the ring is opened, so
        // nothing is allocated or copied per frame and `pixels.buffer` is the same object every lap.  Before the blocks are freed
        // (closeDelivery, setSize to another size, dispose) the buffers are detached: an old view then has length 0.
        // For a video encoder: openDelivery(3, { format: "nv12" | "i420", fullRange: false, background: [0, 0, 0] }) delivers 4:2:0 Y'CbCr
        // (BT.709), 1.5 bytes per pixel.  `pixels` is then the whole payload, as `ffmpeg -f rawvideo -pix_fmt nv12 | yuv420p` reads
        // it -- process.stdout.write(f.pixels) -- and `planes` its parts: Uint8Array views carrying `stride` and `rows`.
        // For a client that reprojects: openDelivery(3, { format, depth: { format: "u16" | "f32", step: 1 | 2, near: 0.1 } }) delivers, beside
        // every frame, that frame's hit depth at every step-th pixel in both directions: `f.depth`, a Uint16Array (inverse depth against
        // `near`: 0 no hit, 65535 at or in front of near, z ~ near * 65535 / u) or Float32Array view of the same block, and `f.depthLayout`.
        const FORMATS = ["rgba8", "nv12", "i420"], DEPTH_FORMATS = ["none", "f32", "u16"];
        let slotBuffers = null, slotViews = null, slotPlanes = null, ringFormat = "rgba8", slotDepth = null, ringDepthLayout = null;
        const held = new Map();                  // serial -> frame object
        const wrapSlots = (buffers) => {
            const layout = this._n.deliveryLayout(this._h);
            slotBuffers = buffers;
            slotViews = buffers.map((b) => new Uint8Array(b, 0, layout.bytes));   // (a depth ring's buffer goes on behind the colour payload)
            slotPlanes = buffers.map((b) => layout.planes.map((p) => Object.assign(new Uint8Array(b, p.offset, p.stride * p.rows), { stride: p.stride, rows: p.rows })));
            ringFormat = FORMATS[layout.format];
            slotDepth = ringDepthLayout = null;
            if (buffers.length && buffers[0].byteLength > layout.bytes) {   // a depth ring
                const d = this._n.depthLayout(this._h);
                d.format = DEPTH_FORMATS[d.format];
                ringDepthLayout = d;
                slotDepth = buffers.map((b) => (d.format === "u16" ? new Uint16Array(b, d.offset, d.width * d.height) : new Float32Array(b, d.offset, d.width * d.height)));
            }
        };
        const dropSlots = () => {
            if (slotBuffers) this._n.detachBuffers(slotBuffers);
            slotBuffers = slotViews = slotPlanes = slotDepth = ringDepthLayout = null;
        };
        this.depthLayout = () => {
            const d = this._n.depthLayout(this._h);
            d.format = DEPTH_FORMATS[d.format];
            return d;
        };
        this.deliveryLayout = () => {
            const layout = this._n.deliveryLayout(this._h);
            layout.format = FORMATS[layout.format];
            return layout;
        };
        const refuseWhileHeld = (what) => {
            if (held.size) throw new Error(what + ": a delivered frame is held (release() it first): its pixels would be freed");
        };
        this.openDelivery = (slots, options) => {
            refuseWhileHeld("openDelivery");
            const o = options || {}, format = FORMATS.indexOf(o.format === undefined ? "rgba8" : o.format), bg = o.background || [0, 0, 0];
            if (format < 0) throw new Error("openDelivery: format must be one of " + FORMATS.join(", "));
            const n = slots === undefined ? 3 : slots;
            if (o.depth) {                       // (refused by the library while a ring is open: closeDelivery() first)
                const depth = DEPTH_FORMATS.indexOf(o.depth.format === undefined ? "u16" : o.depth.format);
                if (depth < 1) throw new Error("openDelivery: depth.format must be one of f32, u16");
                const step = o.depth.step === undefined ? 1 : o.depth.step, near = o.depth.near === undefined ? 0.1 : o.depth.near;
                wrapSlots(this._n.openDeliveryDepth(this._h, n, format, o.fullRange ? 1 : 0, bg[0] | 0, bg[1] | 0, bg[2] | 0, depth, step | 0, +near));
            } else if (format === 0) {
                dropSlots();
                wrapSlots(this._n.openDelivery(this._h, n));
            } else {                             // (refused by the library while a ring is open: closeDelivery() first)
                const buffers = this._n.openDeliveryEx(this._h, n, format, o.fullRange ? 1 : 0, bg[0] | 0, bg[1] | 0, bg[2] | 0);
                wrapSlots(buffers);
            }
            if (o.overlay) this._n.deliverySetOverlay(this._h, 1);   // the ring delivers the selection overlay (setSelectionOverlay first)
        };
        this.closeDelivery = () => {
            refuseWhileHeld("closeDelivery");
            dropSlots();
            this._n.closeDelivery(this._h);
        };
        this.deliverFrame = () => this._n.deliverFrame(this._h);
        this.frameReady = (serial) => this._n.frameReady(this._h, serial || 0);
        // A frame that was not composited (bin-list overflow behind renderAsync) throws ("... was not composited") and frees its
        // slot: render and deliver that pose again.
        this.acquireFrame = (serial) => {
            const f = this._n.acquireFrame(this._h, serial || 0);
            const frame = { serial: f[0], pixels: slotViews[f[1]], width: this.width, height: this.height, format: ringFormat, planes: slotPlanes[f[1]],
                            depth: slotDepth ? slotDepth[f[1]] : undefined, depthLayout: ringDepthLayout || undefined,
                            release: () => { if (held.delete(frame.serial)) this._n.releaseFrame(this._h, frame.serial); } };
            held.set(frame.serial, frame);
            return frame;
        };

        this.setSize = (width, height) => {     // WebGLRenderer.ts:85-102
            const ring = slotBuffers !== null && (width !== this.width || height !== this.height);
            if (ring) { refuseWhileHeld("setSize"); dropSlots(); }
            this.width = width;
            this.height = height;
            this._n.resize(this._h, width, height);
            if (ring) wrapSlots(this._n.deliverySlots(this._h));   // the ring follows the framebuffer: new blocks
        };
        this.resize = () => {};                  // no DOM: nothing to measure
        this.setBand = (x0, x1) => this._n.setBand(this._h, x0, x1);

        const pushCamera = () => {               // uniforms + postMessage({viewProj}) (WebGLRenderer.ts:144-159,268-269,275)
            activeCamera.update(this.width, this.height);
            f32.view.set(activeCamera.viewMatrix.buffer);         // f64 -> f32 exactly like new Float32Array(m.buffer)
            f32.proj.set(activeCamera.projectionMatrix.buffer);
            f32.vp.set(activeCamera.viewProj.buffer);
            this._n.setCamera(this._h, f32.view, f32.proj, f32.vp, activeCamera.fx, activeCamera.fy);
        };
        this.setCameraBuffers = () => pushCamera();
        // the two uniforms a FadeInPass drives (u_useDepthFade, u_depthFade)
        this.setDepthFade = (use, value) => this._n.setDepthFade(this._h, use ? 1 : 0, value);
        // SH textures + u_bandIndex, only for scenes that carry SH data (WebGLRenderer.ts:202-211,321-366)
        this.setShTextures = () => {
            if (!activeScene || !activeScene.shHeight || activeScene.shDroppedOnDevice) return;
            const band = activeScene.bandsIndices;
            const t = activeScene.shs_rgb;
            const count = activeScene.vertexCount - (band[0] + 1);
            this._n.setSceneSh(this._h, t[0], t[1], t[2], count, band);
            // a re-upload hands the frame back: the scene has kept it through its rotate / scale (gsr_set_scene_sh resets it)
            if (count > 0 && activeScene.shFrame) this._n.setShFrame(this._h, activeScene.shFrame);
        };

        // ---- multi-GPU (one process per GPU): joinGroup() is collective -- every rank calls it with the same id
        // (HIPRenderer.createGroupId() on rank 0, passed on by the host: a file, a socket, an env var), its rank, the
        // world size and the same band edges [[x0, x1], ...] (contiguous runs of whole 32-px columns covering the
        // width; HIPRenderer.bandEdges(width, world) gives equal ones).  After that render(scene, camera) draws this
        // rank's band and all-gathers the RGBA8 slabs over xGMI (RCCL) inside the library, and readPixels() returns the
        // whole frame on every rank.
        let group = null;
        this.joinGroup = (g) => {
            const x0 = new Int32Array(g.world), x1 = new Int32Array(g.world);
            for (let q = 0; q < g.world; q++) { x0[q] = g.edges[q][0]; x1[q] = g.edges[q][1]; }
            this._n.commInit(this._h, g.id, g.rank, g.world, x0, x1);
            group = { rank: g.rank, world: g.world };
            if (g.depth) this.setGroupDepth(g.depth);
        };
        // Depth in a group (gsr_comm_set_depth): setGroupDepth({ format: "u16" | "f32", step: 1 | 2, near: 0.1 }) -- or joinGroup({ ..., depth })
        // -- makes every rank exchange its band's hit depth beside the colour slab: readFrameDepth() returns the gathered plane of the
        // last frame (frameDepthLayout(): width x height samples), and openDelivery(n, { depth }) with the same options works in the
        // group: f.depth and f.depthLayout as on a single renderer.  Every rank (and every sharer) passes the same options; null
        // switches it off again.
        this.setGroupDepth = (depth) => {
            if (!depth) { this._n.commSetDepth(this._h, 0, 1, 0); return; }
            const format = DEPTH_FORMATS.indexOf(depth.format === undefined ? "u16" : depth.format);
            if (format < 1) throw new Error("setGroupDepth: depth.format must be one of f32, u16");
            this._n.commSetDepth(this._h, format, (depth.step === undefined ? 1 : depth.step) | 0, +(depth.near === undefined ? 0.1 : depth.near));
        };
        this.frameDepthLayout = () => {
            const d = this._n.frameDepthLayout(this._h);
            d.format = DEPTH_FORMATS[d.format];
            return d;
        };
        this.readFrameDepth = () => {
            const d = this._n.frameDepthLayout(this._h);
            const bytes = new Uint8Array(d.bytes);
            this._n.readFrameDepth(this._h, bytes);
            return DEPTH_FORMATS[d.format] === "u16" ? new Uint16Array(bytes.buffer, 0, d.width * d.height) : new Float32Array(bytes.buffer, 0, d.width * d.height);
        };
        // A second renderer of the SAME rank (frames in flight with renderAsync) joins through the first one: it shares the
        // communicator and the exchange stream, so the rank's collectives go out in frame order (gsr_comm_share).
        this.shareGroup = (leader) => {
            this._n.commShare(this._h, leader._h);
            group = Object.assign({}, leader.group());
        };
        this.leaveGroup = () => { this._n.commDestroy(this._h); group = null; };
        this.group = () => group;

        // WebGLRenderer.ts:241-296
        this.render = (scene, camera) => {
            activeCamera = camera;
            attach(scene);
            pushCamera();
            for (const p of passes) p.render();
            if (group) {
                // band frame, then the framebuffer all-gather; readPixels() waits for the exchange.  The frame is rendered with
                // the blocking call, which repairs a bin-list overflow (regrow + render again) before the band is packed:
                // behind renderAsync the host would not know yet that the compositor drew nothing, and ship the old band.
                this._n.render(this._h);
                this._n.allgatherFrameAsync(this._h);
            } else {
                this._n.render(this._h);
            }
        };
        // Frames in flight (no counterpart in the reference, whose render() is one synchronous draw): renderAsync()
        // enqueues the frame and returns; sync() waits for it.  Several renderers created with { throughput: true }
        // and used round-robin keep the GPU full (bench.py --frames-in-flight).
        this.renderAsync = (scene, camera) => {
            activeCamera = camera;
            attach(scene);
            pushCamera();
            for (const p of passes) p.render();
            this._n.renderAsync(this._h);
            if (group) this._n.allgatherFrameAsync(this._h);
        };
        // sync() throws once (code GSPLAT_HIP, "... frame(s) were not composited") when asynchronous frames were lost
        // to a list overflow; the renderer stays usable and the last frame has been rendered again.
        this.sync = () => this._n.sync(this._h);
        this.overflowPending = () => this._n.overflowPending(this._h);
        this.setListCapacity = (entries) => this._n.setListCapacity(this._h, entries);
        this.sort = (camera) => {                // the worker's job alone (Worker.ts:36-43)
            if (camera) { activeCamera = camera; pushCamera(); }
            this._n.sort(this._h);
        };
        this.dispose = () => {                   // WebGLRenderer.ts:298-310
            detach();                            // (while the context lives: a scene with edits reads them back from it)
            held.clear();
            if (this._h) { dropSlots(); this._n.destroy(this._h); this._h = null; }
            initialized = false;
        };

        // ---- optional device-side scene (SURVEY 8(f) rank 2): .splat rows in, Scene.setData and the transforms run as
        // kernels (bit-identical to Scene.js), no re-upload per change; render with renderDeviceScene(camera) ----
        this.setSceneRows = (rows) => {
            detach();
            this._n.setSceneRows(this._h, rows);
            this._shareToken = null;
            vertexCount = rows.length / 32;
            for (const p of passes) p.init(this, null);
            initialized = true;
        };
        // Shared scenes for callers who manage it themselves: this renderer gives up its scene and renders `other`'s device scene
        // (edit it with scene* through either; setSceneRows or a Scene takes this renderer out again).  sceneSharing(): how many
        // renderers render this renderer's scene (1: not shared) and the device bytes they hold once.
        this.shareScene = (other) => {
            detach();
            shareFrom(other);
            for (const p of passes) p.init(this, null);
            initialized = true;
        };
        this.sceneSharing = () => this._n.sceneSharing(this._h);
        const xf = (kind, args) => { vertexCount = this._n.sceneTransform(this._h, kind, new Float64Array(args)); };
        this.sceneTranslate = (v) => xf(0, [v.x, v.y, v.z]);
        this.sceneRotate = (q) => xf(1, [q.x, q.y, q.z, q.w]);
        this.sceneScale = (v) => xf(2, [v.x, v.y, v.z]);
        this.sceneLimitBox = (xMin, xMax, yMin, yMax, zMin, zMax) => xf(3, [xMin, xMax, yMin, yMax, zMin, zMax]);
        this.readSceneData = () => {
            const data = new Uint32Array(vertexCount * 8), positions = new Float32Array(vertexCount * 3);
            this._n.readScene(this._h, data, positions);
            return { data: data, positions: positions, vertexCount: vertexCount };
        };
        this.renderDeviceScene = (camera) => {
            activeCamera = camera;
            pushCamera();
            for (const p of passes) p.render();
            this._n.render(this._h);
        };

        // ---- results ----
        this.lastDepthIndex = () => { const a = new Uint32Array(vertexCount); this._n.readDepthIndex(this._h, a); return a; };
        // readPixels(out?) / readPixelsFloat(out?): like gl.readPixels, a caller that reads every frame passes its own
        // array (width*height*4 elements) and gets it back filled; without one a fresh array is allocated per call, which
        // costs more than the copy itself (8 MB of zeroed pages at 1080p: 583 -> frames/s with a reused array in
        // tools/bench_node.js).
        // readPixels({ overlay: true, out? }): the selection overlay (setSelectionOverlay) as RGBA8 instead of the frame.
        this.readPixels = (out) => {
            if (out && !ArrayBuffer.isView(out) && out.overlay) {
                const o = out.out || new Uint8Array(this.width * this.height * 4);
                this._n.readOverlayPixels(this._h, o, this.width, this.height);
                return o;
            }
            if (out && !ArrayBuffer.isView(out)) out = out.out;
            const a = out || new Uint8Array(this.width * this.height * 4);
            if (group) this._n.readFrame(this._h, a, this.width, this.height);   // the gathered frame of all ranks
            else this._n.readPixels(this._h, a, this.width, this.height);
            return a;
        };
        this.readPixelsFloat = (out) => { const a = out || new Float32Array(this.width * this.height * 4); this._n.readPixels(this._h, a, this.width, this.height); return a; };
        // Depth planes and picking (gsr_read_depth / gsr_pick): which splat, and how far away, is under a pixel of the last
        // rendered frame.  readDepth({mean?, hit?, index?}) fills the caller's arrays (width*height each; Float32Array,
        // Float32Array, Uint32Array) like readPixels(out) and returns the same object; without an argument all three are
        // allocated.  mean: sum of T_k B_k z_k, premultiplied like the colour channels; hit: z of the first fragment at
        // which accumulated alpha reaches the hit alpha (Infinity: none); index: that fragment's splat (0xffffffff: none).
        this.setHitAlpha = (a) => this._n.setHitAlpha(this._h, a);
        this.depthAsync = () => this._n.depthAsync(this._h);
        this.readDepth = (out) => {
            const np = this.width * this.height;
            const o = out || { mean: new Float32Array(np), hit: new Float32Array(np), index: new Uint32Array(np) };
            this._n.readDepth(this._h, o.mean || null, o.hit || null, o.index || null, this.width, this.height);
            return o;
        };
        // pick(x, y) -> { index, depth, alpha, point }: point is the pixel's centre un-projected to `depth` through the active
        // camera, in doubles -- what a caller assigns to an OrbitControls target; null where nothing is hit
        const pickXY = new Int32Array(2), pickOut = new Float32Array(4), pickBits = new Uint32Array(pickOut.buffer);
        this.pick = (x, y) => {
            pickXY[0] = x; pickXY[1] = y;
            this._n.pick(this._h, pickXY, pickOut);
            const index = pickBits[0], depth = pickOut[1];
            let point = null;
            if (index !== 0xffffffff && activeCamera) {
                const v = activeCamera.viewMatrix.buffer, t = activeCamera.position;
                const cx = (x + 0.5 - this.width / 2) * depth / activeCamera.fx, cy = (y + 0.5 - this.height / 2) * depth / activeCamera.fy;
                point = new Vector3(v[0] * cx + v[1] * cy + v[2] * depth + t.x, v[4] * cx + v[5] * cy + v[6] * depth + t.y,
                                    v[8] * cx + v[9] * cy + v[10] * depth + t.z);
            }
            return { index, depth, mean: pickOut[2], alpha: pickOut[3], point };
        };
        // ---- selection (gsr_select_* / gsr_selection_*): one bit per splat of the device scene, splat i = bit i & 31 of word i >>> 5 ----
        //   renderer.selectRegion({ x0, y0, x1, y1, mask?, stride? }, { mode: "centre" | "hit", op: "replace" | "add" | "subtract" | "intersect" })
        //   scene.eraseSelection(renderer.readSelection(), { keep: false });   // on every device copy of the Scene, and in its mirrors
        // mask: Uint8Array, one byte per pixel of the rectangle, non-zero = inside, rows `stride` (default x1 - x0) apart: a rasterised
        // lasso or brush.  "centre": the last frame's listed splats whose centre pixel lies in the region; "hit": the splats that are
        // the hit of one of its pixels (readDepth().index).  Every call returns the number of selected splats.
        const MODES = { centre: 0, hit: 1 }, OPS = { replace: 0, add: 1, subtract: 2, intersect: 3 };
        const code = (table, v, dflt, what) => {
            const k = v === undefined ? dflt : v;
            if (!(k in table)) throw new Error(what + " must be one of " + Object.keys(table).join(", "));
            return table[k];
        };
        this.selectRegion = (region, options) => {
            const r = region, o2 = options || {};
            const stride = r.mask ? (r.stride === undefined ? r.x1 - r.x0 : r.stride) : 0;
            return this._n.selectRegion(this._h, new Int32Array([r.x0, r.y0, r.x1, r.y1, stride, code(MODES, o2.mode, "centre", "mode"), code(OPS, o2.op, "replace", "op")]),
                                        r.mask || null);
        };
        this.selectBox = (box, options) => this._n.selectBox(this._h, new Float64Array(box), code(OPS, (options || {}).op, "replace", "op"));
        this.setSelection = (words, op) => this._n.setSelection(this._h, words || null, code(OPS, op, "replace", "op"));
        this.invertSelection = () => this._n.invertSelection(this._h);
        this.readSelection = () => this._n.readSelection(this._h);
        // ---- hidden splats (gsr_hide_selected / gsr_hidden_set / gsr_read_hidden / gsr_select_hidden): hide without erasing ----
        //   renderer.selectRegion(lasso); renderer.hideSelection();            // the floaters are out of the way: not drawn, not picked
        //   renderer.invertSelection(); renderer.hideSelection({ op: "replace" });   // isolate what was selected
        //   renderer.showAll();                                                 // undo
        // A hidden splat is in no list of the frames rendered from now on; nothing is erased and the splats keep their numbers.  The
        // set belongs to the device copy (one for the renderers of a shared scene) and survives limitBox / eraseSelection of other
        // splats; Scene.setHidden(mask) sets it on every device copy of a Scene.  A change is a scene edit: pick, selectRegion and
        // readDepth need a new frame afterwards.  Every call returns the number of hidden (selectHidden: selected) splats.
        this.hideSelection = (options) => this._n.hideSelected(this._h, code(OPS, (options || {}).op, "add", "op"));
        this.showAll = () => this._n.setHidden(this._h, null, OPS.replace);
        this.setHidden = (words, options) => this._n.setHidden(this._h, words || null, code(OPS, (options || {}).op, "replace", "op"));
        this.readHidden = () => this._n.readHidden(this._h);
        this.selectHidden = (options) => this._n.selectHidden(this._h, code(OPS, (options || {}).op, "replace", "op"));
        // ---- editing the selection (gsr_selection_bounds / gsr_scene_*_selected): the selected splats and nothing else ----
        //   renderer.selectRegion(lasso); const { min, max } = renderer.selectionBounds();
        //   renderer.rotateSelection(q, { pivot: [(min[0] + max[0]) / 2, (min[1] + max[1]) / 2, (min[2] + max[2]) / 2] });
        //   renderer.paintSelection({ a: 0 });                                  // transparent; absent channels are left alone
        // What Scene.translate / rotate / scale would leave in a Scene holding only the selected splats; a pivot is translate(-pivot),
        // the operation, translate(+pivot).  These edit THIS renderer's device copy only: a Scene attached to it does not learn of
        // them -- Scene.translateSelection(mask, v) and its kin edit every device copy and keep the Scene's arrays right.  A scene
        // edit: pick, selectRegion and readDepth need a new frame afterwards; selection, hidden set and contribution state stay.
        const vec = (v, k) => (Array.isArray(v) || ArrayBuffer.isView(v) ? new Float64Array(v) : new Float64Array(k === 4 ? [v.x, v.y, v.z, v.w] : [v.x, v.y, v.z]));
        const pivotOf = (options) => (options && options.pivot ? vec(options.pivot, 3) : null);
        this.selectionBounds = () => {
            const box = new Float32Array(6), count = this._n.selectionBounds(this._h, box);
            return { count, min: box.slice(0, 3), max: box.slice(3, 6) };
        };
        this.translateSelection = (v) => this._n.editSelected(this._h, 0, vec(v, 3), null);
        // { sh: true }: the selected splats' SH coefficients turn with them (gsr_scene_rotate_selected_sh, below); default: today's path
        this.rotateSelection = (q, options) => {
            if (!(options && options.sh)) return this._n.editSelected(this._h, 1, vec(q, 4), pivotOf(options));
            this._n.rotateSelectedSh(this._h, vec(q, 4), pivotOf(options));
            shTurned(false);
        };
        this.scaleSelection = (s, options) => this._n.editSelected(this._h, 2, vec(s, 3), pivotOf(options));
        this.paintSelection = (rgba) => {
            const [value, byteMask] = Scene.rgbaWord(rgba);
            this._n.paintSelected(this._h, value, byteMask);
        };
        // ---- rotating SH coefficients (gsr_scene_rotate_sh / _rotate_selected_sh / _bake_sh_frame): a selection turns with its SH colour ----
        //   renderer.selectRegion(lasso); renderer.rotateSelection(q, { pivot, sh: true });    // the highlights turn with the object
        //   renderer.bakeSHFrame();               // first, where a followed scene.rotate has left a frame: it moves into the coefficients
        // rotateSH(q, { selected }) rotates the coefficients alone -- every SH row, or the selected splats' rows -- and returns the
        // rows rotated; the SH frame is neither read nor written.  rotateSelection(q, { sh: true }) needs the identity frame, which
        // bakeSHFrame() makes of any frame that is a rotation times a uniform scale; it returns the Quaternion it rotated by.  These
        // act on THIS renderer's device copy; an attached Scene's shs_rgb mirror is marked stale and read back on its next use.
        const shTurned = (baked) => { if (activeScene && activeScene._deviceTurnedSh) activeScene._deviceTurnedSh(baked); };
        this.rotateSH = (q, options) => {
            const rows = this._n.rotateSh(this._h, vec(q, 4), options && options.selected ? 1 : 0);
            shTurned(false);
            return rows;
        };
        this.bakeSHFrame = () => {
            const q = this._n.bakeShFrame(this._h);
            shTurned(true);
            return new Quaternion(q[0], q[1], q[2], q[3]);
        };
        // ---- growing the scene (gsr_scene_reserve / _capacity / _duplicate_selected / _append_selected): copies and pasted splats ----
        //   renderer.selectRegion(lasso); const { first, count } = renderer.duplicateSelection();   // the copies are now the selection ...
        //   renderer.translateSelection([1, 0, 0]);                                                  // ... so this moves them
        //   renderer.reserveScene(renderer.sceneCapacity() * 2);    // a host that will copy many times: nothing is re-allocated until then
        // The selected splats are copied bit for bit behind the scene's last splat -- appendSelectionFrom(other): the splats selected
        // in another renderer of the same GPU, device to device -- and become the selection; existing indices, the hidden set and the
        // contribution state stay.  These act on THIS renderer's device copy only: Scene.duplicateSelection(mask) / Scene.append(other)
        // grow every device copy and keep the Scene's arrays right.  Refused while the device scene has SH rows.
        this.reserveScene = (rows) => { this._n.reserveScene(this._h, rows); };
        this.sceneCapacity = () => this._n.sceneCapacity(this._h);
        this.duplicateSelection = () => { const r = this._n.duplicateSelected(this._h); grown(r); return r; };
        this.appendSelectionFrom = (other) => { const r = this._n.appendSelected(this._h, other._h); grown(r); return r; };
        // ---- contribution (gsr_contrib_* / gsr_select_contrib): per splat of the device scene, what it showed over the frames of a tour ----
        //   renderer.resetContribution(); for (const cam of tour) { renderer.render(scene, cam); renderer.accumulateContribution(); }
        //   renderer.selectContribution({ stat: "pixels", below: 1 }); scene.eraseSelection(renderer.readSelection());   // what never showed
        // weight[i] * 2^-24: the sum of splat i's fragment weights ("fully opaque pixels' worth"); peak[i]: its largest weight;
        // pixels[i]: the pixels it covered; frames: the passes counted.  selectContribution picks the splats whose value is below
        // `below` (f64, over all splats) and folds them into the selection; it throws while no pass has contributed.
        const STATS = { weight: 0, peak: 1, pixels: 2 };
        this.resetContribution = () => { this._n.contribReset(this._h); };
        this.accumulateContribution = () => { this._n.contribAccumulate(this._h); };
        this.readContribution = () => this._n.readContrib(this._h);
        this.selectContribution = (options) => {
            const o2 = options || {};
            const below = o2.below === undefined ? 0 : Number(o2.below);
            return this._n.selectContrib(this._h, code(STATS, o2.stat, "weight", "stat"), below, code(OPS, o2.op, "replace", "op"));
        };
        // ---- splat data (gsr_attr_stats / gsr_attr_histogram / gsr_select_attr): an attribute's distribution, a range of it as a picker ----
        //   const { min, max } = renderer.splatStats("scale_max");
        //   const h = renderer.splatHistogram("scale_max", { lo: min, hi: max * (1 + 1e-12), bins: 64 });   // h.counts, h.edges
        //   renderer.selectAttribute("scale_max", { lo: h.edges[48] });        // the huge ones: exactly the splats of bins 48 .. 63
        // attr: x, y, z, distance (from `origin`), red, green, blue, opacity (bytes, 0 .. 255), scale_x / _y / _z / _min / _max,
        // contrib_weight / _peak / _pixels (selectContribution's values).  selected / visible restrict the statistics to the selection /
        // to what is not hidden; selectAttribute ranges over every splat and picks lo <= value < hi (never a NaN).  The histogram's
        // edges are HIPRenderer.attrEdges(lo, hi, bins): selectAttribute(attr, { lo: edges[a], hi: edges[b] }) selects exactly the
        // splats an unscoped histogram counts in bins a .. b - 1.
        const ATTRS = { x: 0, y: 1, z: 2, distance: 3, red: 4, green: 5, blue: 6, opacity: 7, scale_x: 8, scale_y: 9, scale_z: 10,
                        scale_min: 11, scale_max: 12, contrib_weight: 13, contrib_peak: 14, contrib_pixels: 15 };
        const originOf = (o) => (o.origin === undefined || o.origin === null ? null : vec(o.origin, 3));
        const scopeOf = (o) => (o.selected ? 1 : 0) | (o.visible ? 2 : 0);
        this.splatStats = (attr, options) => {
            const o2 = options || {};
            return this._n.attrStats(this._h, code(ATTRS, attr, undefined, "attr"), originOf(o2), scopeOf(o2));
        };
        this.splatHistogram = (attr, options) => {
            const o2 = options || {}, lo = Number(o2.lo), hi = Number(o2.hi), bins = o2.bins === undefined ? 64 : o2.bins;
            const a = code(ATTRS, attr, undefined, "attr");
            if (!Number.isInteger(bins) || bins < 1 || bins > 4096) throw new Error("bins must be an integer in 1 .. 4096");
            const h = this._n.attrHistogram(this._h, a, originOf(o2), scopeOf(o2), lo, hi, bins);
            return { counts: h.counts, below: h.below, above: h.above, nan: h.nan, edges: HIPRenderer.attrEdges(lo, hi, bins) };
        };
        this.selectAttribute = (attr, options) => {
            const o2 = options || {};
            const lo = o2.lo === undefined ? -Infinity : Number(o2.lo), hi = o2.hi === undefined ? Infinity : Number(o2.hi);
            return this._n.selectAttr(this._h, code(ATTRS, attr, undefined, "attr"), originOf(o2), lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        // ---- neighbours (gsr_neighbours / gsr_select_neighbours): how many other splats lie within a radius of each ----
        //   renderer.selectNeighbours(0.05, { below: 3 }); scene.eraseSelection(renderer.readSelection());   // floaters: fewer than 3 neighbours within 0.05
        //   const { counts, hist } = renderer.splatNeighbours(0.05, { cap: 64 });       // hist[k]: splats with k neighbours, hist[cap]: cap or more
        // A splat's count is the number of OTHER splats in scope within `radius` of it (f64, distance exactly radius counts), at most
        // `cap` (1 .. 4095, default 64); scope: "selected", "visible" or both -- counted among and reported for those only.
        // selectNeighbours picks lo <= count < hi (below: hi with lo 0; default hi cap + 1) and returns the selected count; with op
        // "replace" exactly hist.slice(lo, hi) summed.  Both index the device scene as it is now.  budget: the most pair tests the
        // call may make (default 2^34); a radius that would need more throws before the count pass runs.
        const NB_SCOPES = { selected: 1, visible: 2 };
        const nbScope = (o) => {
            const names = o.scope === undefined || o.scope === null ? [] : (typeof o.scope === "string" ? [o.scope] : Array.from(o.scope));
            return names.reduce((m, name) => m | code(NB_SCOPES, name, undefined, "scope"), 0);
        };
        const nbArgs = (radius, o) => {
            const cap = o.cap === undefined ? 64 : o.cap, budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (!Number.isInteger(cap) || cap < 1 || cap > 4095) throw new Error("cap must be an integer in 1 .. 4095");
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            return [Number(radius), cap, nbScope(o), budget];
        };
        this.splatNeighbours = (radius, options) => {
            const o2 = options || {};
            const r = this._n.neighbours(this._h, ...nbArgs(radius, o2));
            return { counts: r.counts, hist: r.hist, inScope: r.inScope, nonfinite: r.nonfinite, pairBound: r.pairBound };
        };
        this.selectNeighbours = (radius, options) => {
            const o2 = options || {}, args = nbArgs(radius, o2), cap = args[1];
            const lo = o2.lo === undefined ? 0 : o2.lo, hi = o2.below !== undefined ? o2.below : o2.hi === undefined ? cap + 1 : o2.hi;
            if (o2.below !== undefined && (o2.hi !== undefined || o2.lo !== undefined)) throw new Error("selectNeighbours: below goes alone (it is { lo: 0, hi: below })");
            if (!Number.isInteger(lo) || !Number.isInteger(hi) || lo < 0 || lo > hi || hi > cap + 1) throw new Error("selectNeighbours: 0 <= lo <= hi <= cap + 1 must hold");
            return this._n.selectNeighbours(this._h, ...args, lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        // ---- planes (gsr_fit_plane / gsr_plane_inliers / gsr_select_plane / gsr_plane_alignment): the floor found, selected by, aligned to ----
        //   const fit = renderer.fitPlane(0.01);                                           // RANSAC on the device: 512 hypotheses, every one scored in f64
        //   renderer.selectPlane(fit.plane, { hi: -0.01 }); scene.eraseSelection(renderer.readSelection());   // everything under the floor
        //   const { rotation, translation } = renderer.planeAlignment(fit.plane); scene.rotate(rotation); scene.translate(translation);   // the floor at y = 0
        // fitPlane draws `hypotheses` (1 .. 4096, default 512) planes through three splats in scope each -- a counter-based generator
        // from `seed` -- and scores each by the splats within `threshold` of it (a distance of exactly threshold counts); the largest
        // score wins, ties go to the smallest index.  plane: Float64Array (nx, ny, nz, d), unit normal; null when nothing was found.
        // planeInliers scores planes of the host's, used as given.  selectPlane picks lo <= distance <= hi over all splats (within: t is
        // { lo: -t, hi: t }): after an unscoped fit, selectPlane(plane, { within: threshold }) selects exactly fit.inliers splats.
        // budget: the most tests (hypotheses x candidates) a call may make (default 2^34); more throws before the scoring pass runs.
        const planeOf = (plane, what) => {
            const p = Float64Array.from(plane);
            if (p.length !== 4) throw new Error(what + ": a plane is (a, b, c, d)");
            return p;
        };
        const planeBudget = (o) => {
            const budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            return budget;
        };
        this.fitPlane = (threshold, options) => {
            const o2 = options || {};
            const hypotheses = o2.hypotheses === undefined ? 512 : o2.hypotheses, seed = o2.seed === undefined ? 0 : o2.seed;
            if (!Number.isInteger(hypotheses) || hypotheses < 1 || hypotheses > 4096) throw new Error("hypotheses must be an integer in 1 .. 4096");
            if (!Number.isSafeInteger(seed) || seed < 0) throw new Error("seed must be a non-negative integer");
            const r = this._n.fitPlane(this._h, Number(threshold), hypotheses, seed, nbScope(o2), planeBudget(o2), !!o2.scores);
            const out = { plane: r.found ? r.plane : null, found: !!r.found, best: r.best, triple: r.triple, inliers: r.inliers, degenerate: r.degenerate,
                          inScope: r.inScope, nonfinite: r.nonfinite, hypotheses: r.hypotheses, tests: r.tests };
            if (o2.scores) out.scores = r.scores;
            return out;
        };
        this.planeInliers = (planes, threshold, options) => {
            const o2 = options || {};
            const rows = Array.from(planes, (p) => planeOf(p, "planeInliers"));
            if (rows.length < 1 || rows.length > 4096) throw new Error("planeInliers: 1 .. 4096 planes");
            const flat = new Float64Array(4 * rows.length);
            rows.forEach((p, k) => flat.set(p, 4 * k));
            return this._n.planeInliers(this._h, flat, rows.length, Number(threshold), nbScope(o2), planeBudget(o2)).inliers;
        };
        this.selectPlane = (plane, options) => {
            const o2 = options || {};
            if (o2.within !== undefined && (o2.lo !== undefined || o2.hi !== undefined)) throw new Error("selectPlane: within goes alone (it is { lo: -within, hi: within })");
            const lo = o2.within !== undefined ? -Number(o2.within) : o2.lo === undefined ? -Infinity : Number(o2.lo);
            const hi = o2.within !== undefined ? Number(o2.within) : o2.hi === undefined ? Infinity : Number(o2.hi);
            return this._n.selectPlane(this._h, planeOf(plane, "selectPlane"), lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        // the whole-scene rotation and translation that take `plane` to axis . p = 0 (axis: default +y), by the library's one
        // statement of it (a pure function: no device): scene.rotate(rotation); scene.translate(translation) acts on every device copy
        this.planeAlignment = (plane, options) => {
            const o2 = options || {}, a = o2.axis === undefined ? [0, 1, 0] : (Array.isArray(o2.axis) || ArrayBuffer.isView(o2.axis) ? o2.axis : [o2.axis.x, o2.axis.y, o2.axis.z]);
            const axis = Float64Array.from(a);
            if (axis.length !== 3) throw new Error("planeAlignment: axis is (x, y, z)");
            const r = this._n.planeAlignment(planeOf(plane, "planeAlignment"), axis);
            return { rotation: new Quaternion(r.q[0], r.q[1], r.q[2], r.q[3]), translation: new Vector3(r.t[0], r.t[1], r.t[2]) };
        };
        // ---- matching and registration (gsr_match / gsr_select_match / gsr_register): this renderer's scene matched to another's, aligned with it ----
        //   const fit = renderer.registerTo(other, 0.25); scene.rotate(fit.rotation); scene.translate(fit.translation);   // this capture onto the other one
        //   renderer.selectMatch(other, 0.05, { lo: 0.05 });                                // what the other capture lacks: no splat of it within 0.05
        //   const { idx, d2 } = renderer.matchScene(other, 0.05);                           // per splat: the nearest splat of `other`, 0xffffffff / Infinity without one
        // For every splat in scope, moved by `transform` (12 numbers, row-major 3 x 4 (R | t); default the identity), the nearest splat of
        // `target`'s scene in targetScope within `radius` (f64, smallest in (squared distance, index), a distance of exactly radius counts);
        // NaN outside the scope.  sums: true adds { pairs, sums: Float64Array(16) }, what a rigid solve takes.  selectMatch picks
        // lo <= distance < hi (hi undefined or Infinity: no upper end, the unmatched splats included).  registerTo iterates match, reduce
        // and solve from `transform` and returns the rigid transform that takes this scene onto the target's -- status "converged",
        // "max_iterations" or "too_few" -- with its rotation and translation; neither device scene is written.  scope, targetScope and
        // budget as splatNeighbours.  `target` may be this renderer.
        const REGISTER_STATUS = ["converged", "max_iterations", "too_few"];
        const matchArgs = (target, radius, o) => {
            if (!(target instanceof HIPRenderer) || !target._h) throw new Error("target must be a live HIPRenderer");
            const budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            let m = null;
            if (o.transform !== undefined && o.transform !== null) {
                m = Float64Array.from(o.transform);
                if (m.length !== 12) throw new Error("transform is 12 numbers, row-major 3 x 4 (R | t)");
            }
            return [target._h, m, Number(radius), nbScope(o), nbScope({ scope: o.targetScope }), budget];
        };
        this.matchScene = (target, radius, options) => {
            const o2 = options || {};
            const r = this._n.matchScene(this._h, ...matchArgs(target, radius, o2), !!o2.sums);
            const out = { idx: r.idx, d2: r.d2, inScope: r.inScope, nonfinite: r.nonfinite, targetIndexed: r.targetIndexed, matched: r.matched, pairBound: r.pairBound,
                          d2Min: r.d2Min, d2Max: r.d2Max };
            if (o2.sums) { out.pairs = r.pairs; out.sums = r.sums; }
            return out;
        };
        this.selectMatch = (target, radius, options) => {
            const o2 = options || {}, args = matchArgs(target, radius, o2);
            const lo = o2.lo === undefined ? 0 : Number(o2.lo), hi = o2.hi === undefined || o2.hi === null ? Infinity : Number(o2.hi);
            if (Number.isNaN(lo) || Number.isNaN(hi) || lo > hi) throw new Error("selectMatch: lo <= hi must hold, neither a NaN");
            return this._n.selectMatch(this._h, ...args, lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        // Point to plane (gsr_match_surface / gsr_register_surface): registerTo(other, radius, { residual: "surface", normals: { source:
        // "own" | "knn", radius, k } }) pulls every splat toward the other capture's SURFACE along the normal of its match instead of
        // toward the nearest sample -- far fewer steps on floors, walls and table tops, and no biased pose; normals says how `target`'s
        // normals are made (default its splats' own shortest axes; "knn" as splatNormals), once per call.  It adds status "degenerate"
        // (the residuals leave a direction free: a target of one or two planes; "too_few" is fewer than 6 pairs with a normal) and
        // surfacePairs, surfaceRms, valid.  residual "point", the default, is the path above.  matchSurface is one such step as data:
        // { pairs, surfacePairs, sums: Float64Array(29) }, what SPLAT.surfaceSolve takes.
        const SURFACE_STATUS = REGISTER_STATUS.concat(["degenerate"]);
        const surfaceNormals = (o) => {
            const nm = o.normals || {}, source = code(NORMAL_SOURCES, nm.source, "own", "normals.source");
            const budget = nm.budget === undefined || nm.budget === null ? 0 : Number(nm.budget);
            if (!(budget >= 0)) throw new Error("normals.budget must be a non-negative number");
            if (source === NORMAL_SOURCES.own) return [source, 0, 0, budget];
            const k = nm.k === undefined ? 8 : nm.k;
            if (!(Number(nm.radius) > 0)) throw new Error("normals: the knn source needs a radius");
            if (!Number.isInteger(k) || k < 2 || k > 32) throw new Error("normals.k must be an integer in 2 .. 32");
            return [source, Number(nm.radius), k, budget];
        };
        this.matchSurface = (target, radius, options) => {
            const o2 = options || {};
            const r = this._n.matchSurface(this._h, ...matchArgs(target, radius, o2), ...surfaceNormals(o2));
            return { pairs: r.pairs, surfacePairs: r.surfacePairs, sums: r.sums, inScope: r.inScope, nonfinite: r.nonfinite, targetIndexed: r.targetIndexed,
                     matched: r.matched, pairBound: r.pairBound, d2Min: r.d2Min, d2Max: r.d2Max };
        };
        this.registerTo = (target, radius, options) => {
            const o2 = options || {}, args = matchArgs(target, radius, o2);
            const steps = o2.maxIterations === undefined ? 32 : o2.maxIterations, tolerance = o2.tolerance === undefined ? 2 ** -40 : Number(o2.tolerance);
            if (!Number.isInteger(steps) || steps < 1 || steps > 256) throw new Error("maxIterations must be an integer in 1 .. 256");
            if (!(tolerance >= 0)) throw new Error("tolerance must be a non-negative number");
            const residual = o2.residual === undefined ? "point" : o2.residual;
            if (residual !== "point" && residual !== "surface") throw new Error("residual is \"point\" or \"surface\"");
            if (residual === "surface") {
                const s = this._n.registerSurface(this._h, ...args, ...surfaceNormals(o2), steps, tolerance, !!o2.history);
                const fit = { transform: s.transform, rotation: new Quaternion(s.q[0], s.q[1], s.q[2], s.q[3]), translation: new Vector3(s.t[0], s.t[1], s.t[2]),
                              status: SURFACE_STATUS[s.status], iterations: s.iterations, pairs: s.pairs, surfacePairs: s.surfacePairs, rms: s.rms,
                              surfaceRms: s.surfaceRms, delta: s.delta, valid: s.valid };
                if (o2.history) { fit.stepPairs = s.stepPairs; fit.stepSurfacePairs = s.stepSurfacePairs; fit.stepRms = s.stepRms; fit.stepSurfaceRms = s.stepSurfaceRms; }
                return fit;
            }
            if (o2.normals !== undefined) throw new Error("normals goes with residual: \"surface\"");
            const r = this._n.registerTo(this._h, ...args, steps, tolerance, !!o2.history);
            const out = { transform: r.transform, rotation: new Quaternion(r.q[0], r.q[1], r.q[2], r.q[3]), translation: new Vector3(r.t[0], r.t[1], r.t[2]),
                          status: REGISTER_STATUS[r.status], iterations: r.iterations, pairs: r.pairs, rms: r.rms };
            if (o2.history) { out.stepPairs = r.stepPairs; out.stepRms = r.stepRms; }
            return out;
        };
        // the rotation and translation of a transform (12 numbers), by the library's one statement of it (a pure function: no device):
        // scene.rotate(rotation); scene.translate(translation) applies it to every device copy
        this.rigidDecompose = (transform) => {
            const m = Float64Array.from(transform);
            if (m.length !== 12) throw new Error("rigidDecompose: transform is 12 numbers, row-major 3 x 4 (R | t)");
            const r = this._n.rigidDecompose(m);
            return { rotation: new Quaternion(r.q[0], r.q[1], r.q[2], r.q[3]), translation: new Vector3(r.t[0], r.t[1], r.t[2]) };
        };
        // ---- clusters (gsr_clusters / gsr_select_clusters / gsr_select_cluster_at): the connected islands of splats at a linking radius ----
        //   const p = renderer.pick(x, y); renderer.selectClusterAt(0.05, { seed: p.index });        // the island under the cursor
        //   renderer.selectClusters(0.05, { below: 50 }); scene.eraseSelection(renderer.readSelection());   // noise and every island of fewer than 50 splats
        //   renderer.selectClusterAt(0.05, { largest: true }); renderer.invertSelection();            // everything but the largest island
        // Two splats within `radius` of each other (f64, distance exactly radius links) share a cluster; minPts (0 .. 4095, default 0)
        // makes it DBSCAN: only a splat with minPts or more others within radius links, a splat beside such a one takes the smallest
        // such label, the rest is noise.  labels[i]: the smallest splat index of i's cluster, 0xffffffff for noise and outside the
        // scope; sizes[i]: the splats labelled like i.  selectClusters picks the splats whose cluster has atLeast <= size < below
        // splats (noise has size 0); selectClusterAt the cluster of splat `seed`, or the largest one.  scope and budget as splatNeighbours.
        const CLUSTER_LARGEST = 0xffffffff;
        const clArgs = (radius, o) => {
            const minPts = o.minPts === undefined ? 0 : o.minPts, budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (!Number.isInteger(minPts) || minPts < 0 || minPts > 4095) throw new Error("minPts must be an integer in 0 .. 4095");
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            return [Number(radius), minPts, nbScope(o), budget];
        };
        this.splatClusters = (radius, options) => {
            const o2 = options || {};
            const r = this._n.clusters(this._h, ...clArgs(radius, o2));
            return { labels: r.labels, sizes: r.sizes, inScope: r.inScope, nonfinite: r.nonfinite, pairBound: r.pairBound, core: r.core, border: r.border,
                     noise: r.noise, clusters: r.clusters, largestLabel: r.largestLabel, largestSize: r.largestSize };
        };
        this.selectClusters = (radius, options) => {
            const o2 = options || {}, args = clArgs(radius, o2);
            const lo = o2.atLeast === undefined ? 0 : o2.atLeast, hi = o2.below === undefined ? CLUSTER_LARGEST : o2.below;
            if (!Number.isInteger(lo) || !Number.isInteger(hi) || lo < 0 || lo > hi || hi > CLUSTER_LARGEST) throw new Error("selectClusters: 0 <= atLeast <= below < 2^32 must hold");
            return this._n.selectClusters(this._h, ...args, lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        this.selectClusterAt = (radius, options) => {
            const o2 = options || {}, args = clArgs(radius, o2);
            if ((o2.largest === true) === (o2.seed !== undefined)) throw new Error("selectClusterAt: give either seed (a splat index) or largest: true");
            if (o2.seed !== undefined && (!Number.isInteger(o2.seed) || o2.seed < 0 || o2.seed >= CLUSTER_LARGEST)) throw new Error("selectClusterAt: seed must be a splat index");
            return this._n.selectClusterAt(this._h, ...args, o2.largest === true ? CLUSTER_LARGEST : o2.seed, code(OPS, o2.op, "replace", "op"));
        };
        // ---- k nearest neighbours (gsr_knn / gsr_select_knn): per-splat neighbour lists, and statistical outlier removal ----
        //   renderer.selectStatisticalOutliers(0.1, { k: 8, stdRatio: 2 }); scene.eraseSelection(renderer.readSelection());
        //   const { found, idx, d2, values } = renderer.splatKnn(0.1, { k: 8, lists: true });   // row i of idx / d2 at [i * k]
        // For every splat in scope the k (1 .. 32, default 8) nearest OTHER splats in scope within `radius`, ascending by (squared
        // distance, index): found[i] how many there are, idx / d2 (lists: true) their indices and squared distances, padded with
        // 0xffffffff / Infinity.  values[i]: stat "kth", the distance to the k-th (Infinity without one); "mean" (the default), the mean
        // distance to those found (Infinity with none); NaN outside the scope.  hist[t]: the splats in scope with found == t.
        // selectKnn picks lo <= value < hi (hi undefined or Infinity: no upper end, the Infinity values included).
        // selectStatisticalOutliers picks value >= mean + stdRatio * (sample standard deviation) of the finite values and returns
        // { selected, threshold }.  scope and budget as splatNeighbours.
        const KNN_STATS = { kth: 0, mean: 1 };
        const knnArgs = (radius, o) => {
            const k = o.k === undefined ? 8 : o.k, budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (!Number.isInteger(k) || k < 1 || k > 32) throw new Error("k must be an integer in 1 .. 32");
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            return [Number(radius), k, nbScope(o), budget, code(KNN_STATS, o.stat, "mean", "stat")];
        };
        this.splatKnn = (radius, options) => {
            const o2 = options || {};
            const r = this._n.knn(this._h, ...knnArgs(radius, o2), o2.lists ? 1 : 0);
            const out = { found: r.found, values: r.values, hist: r.hist, inScope: r.inScope, nonfinite: r.nonfinite, pairBound: r.pairBound, complete: r.complete,
                          finiteValues: r.finiteValues, valueMin: r.valueMin, valueMax: r.valueMax };
            if (o2.lists) { out.idx = r.idx; out.d2 = r.d2; }
            return out;
        };
        this.selectKnn = (radius, options) => {
            const o2 = options || {}, args = knnArgs(radius, o2);
            const lo = o2.lo === undefined ? 0 : Number(o2.lo), hi = o2.hi === undefined || o2.hi === null ? Infinity : Number(o2.hi);
            if (Number.isNaN(lo) || Number.isNaN(hi) || lo > hi) throw new Error("selectKnn: lo <= hi must hold, neither a NaN");
            return this._n.selectKnn(this._h, ...args, lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        this.selectStatisticalOutliers = (radius, options) => {
            const o2 = options || {}, stdRatio = o2.stdRatio === undefined ? 2 : Number(o2.stdRatio);
            const o3 = { k: o2.k, scope: o2.scope, budget: o2.budget, stat: "mean" };
            const values = this.splatKnn(radius, o3).values;
            let count = 0, sum = 0;
            for (let i = 0; i < values.length; i++) if (Number.isFinite(values[i])) { count++; sum += values[i]; }
            let threshold = Infinity;   // fewer than two finite values: only the splats without a neighbour
            if (count >= 2) {
                const mu = sum / count;
                let sq = 0;
                for (let i = 0; i < values.length; i++) if (Number.isFinite(values[i])) sq += (values[i] - mu) * (values[i] - mu);
                threshold = mu + stdRatio * Math.sqrt(sq / (count - 1));
            }
            return { selected: this.selectKnn(radius, { ...o3, lo: threshold, op: o2.op }), threshold };
        };
        // ---- normals (gsr_normals / gsr_select_normal): per-splat surface normals, selection by direction or surface variation ----
        //   renderer.selectNormal("abs_dot", { axis: [0, 1, 0], hi: 0.2, radius: 0.1, k: 8 });   // the walls: |n . up| small
        //   const { normals, variation } = renderer.splatNormals(0.1, { k: 8, toward: camera.position });   // row i of normals at [3 * i]
        // A unit normal per splat in scope: source "knn" (the default), the eigenvector of the smallest eigenvalue of the covariance of
        // the splat and its k (2 .. 32, default 8) nearest others in scope within `radius`; "own", the splat's own shortest axis (no
        // index, no walk; radius is not read).  variation[i] = l_min / (l_0 + l_1 + l_2): 0 on a plane, large at edges and corners.
        // toward: [x, y, z], every normal faces that viewpoint; without it the first non-zero component is positive.  A splat without
        // a normal holds NaN in both; found[i] is the length of its list.  selectNormal picks lo <= value <= hi, both ends closed,
        // the value from the stored float32 normal: stat "dot" n . axis, "abs_dot" |n . axis|, "variation" (no axis).  scope and
        // budget as splatNeighbours.
        const NORMAL_SOURCES = { knn: 0, own: 1 }, NORMAL_STATS = { dot: 0, abs_dot: 1, variation: 2 };
        const vec3 = (v, what) => {
            if (!v || v.length !== 3) throw new Error(what + " must hold three numbers");
            return [Number(v[0]), Number(v[1]), Number(v[2])];
        };
        const normalArgs = (radius, o) => {
            const source = code(NORMAL_SOURCES, o.source, "knn", "source");
            const k = o.k === undefined ? 8 : o.k, budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (source === 0 && (!Number.isInteger(k) || k < 2 || k > 32)) throw new Error("k must be an integer in 2 .. 32");
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            const oriented = o.toward !== undefined && o.toward !== null, t = oriented ? vec3(o.toward, "toward") : [0, 0, 0];
            return [source, source === 0 ? Number(radius) : 0, source === 0 ? k : 0, nbScope(o), budget, oriented ? 1 : 0, t[0], t[1], t[2]];
        };
        this.splatNormals = (radius, options) => {
            const r = this._n.normals(this._h, ...normalArgs(radius, options || {}));
            return { normals: r.normals, variation: r.variation, found: r.found, inScope: r.inScope, nonfinite: r.nonfinite, pairBound: r.pairBound, valid: r.valid,
                     variationMin: r.variationMin, variationMax: r.variationMax };
        };
        this.selectNormal = (stat, options) => {
            const o2 = options || {}, args = normalArgs(o2.radius, o2), s = code(NORMAL_STATS, stat, undefined, "stat");
            const lo = o2.lo === undefined || o2.lo === null ? -Infinity : Number(o2.lo), hi = o2.hi === undefined || o2.hi === null ? Infinity : Number(o2.hi);
            if (Number.isNaN(lo) || Number.isNaN(hi) || lo > hi) throw new Error("selectNormal: lo <= hi must hold, neither a NaN");
            const hasAxis = s !== 2, a = hasAxis ? vec3(o2.axis, "axis") : [0, 0, 0];
            return this._n.selectNormal(this._h, ...args, s, hasAxis ? 1 : 0, a[0], a[1], a[2], lo, hi, code(OPS, o2.op, "replace", "op"));
        };
        // ---- merging cells (gsr_cells / gsr_scene_merge_cells): voxel simplification of this renderer's copy ----
        //   const { rowsAfter, hist } = renderer.splatCells(0.05); renderer.mergeCells(0.05);   // the report, then the edit it announced
        // The candidates -- the splats in scope with finite position, rotation and scale -- fall into the cells of a grid of side
        // `cell`.  splatCells reports them: hist[k] the cells with k members (hist[cap]: cap or more; cap 1 .. 4095, default 64),
        // leader[i] (leaders: true) the smallest candidate index of i's cell, 0xffffffff for a splat that is no candidate, and
        // rowsAfter, the rows mergeCells would leave.  mergeCells replaces every cell of two or more by one splat, by moment matching
        // (opacity x volume weighted mean, the mixture's covariance, rotation and scale from its eigen-decomposition), at the smallest
        // member's row, removes the other members as eraseSelection removes, and returns { count, ... }; afterwards the selection is
        // exactly the merged rows.  Like rotateSelection it acts on the device copy: the Scene object's arrays are not changed.  scope
        // and budget as splatNeighbours.  A scene with SH rows is refused.
        const cellBudget = (o) => {
            const budget = o.budget === undefined || o.budget === null ? 0 : Number(o.budget);
            if (!(budget >= 0)) throw new Error("budget must be a non-negative number");
            return budget;
        };
        const cellInfo = (r) => ({ inScope: r.inScope, candidates: r.candidates, cells: r.cells, mergedCells: r.mergedCells, mergedMembers: r.mergedMembers,
                                   largest: r.largest, rowsAfter: r.rowsAfter, pairBound: r.pairBound });
        this.splatCells = (cell, options) => {
            const o2 = options || {}, cap = o2.cap === undefined ? 64 : o2.cap;
            if (!Number.isInteger(cap) || cap < 1 || cap > 4095) throw new Error("cap must be an integer in 1 .. 4095");
            const r = this._n.cells(this._h, Number(cell), cap, nbScope(o2), cellBudget(o2), o2.leaders ? 1 : 0);
            const out = { hist: r.hist, ...cellInfo(r) };
            if (o2.leaders) out.leader = r.leader;
            return out;
        };
        this.mergeCells = (cell, options) => {
            const o2 = options || {};
            const r = this._n.mergeCells(this._h, Number(cell), nbScope(o2), cellBudget(o2));
            vertexCount = r.count;   // (the device copy's: readSceneData and lastDepthIndex are sized by it)
            return { count: r.count, ...cellInfo(r) };
        };
        // ---- selection overlay (gsr_set_overlay / gsr_read_overlay*): the last frame with the selected splats tinted ----
        //   renderer.setSelectionOverlay({ tint: [1, 0.5, 0], mix: 0.5 }); renderer.render(scene, cam);
        //   const { rgba, cover } = renderer.readOverlay();   // or readPixels({ overlay: true }), or openDelivery(n, { overlay: true })
        // Selected splats are drawn with lerp(colour, tint, mix); cover[p] is the share of pixel p's alpha they supply (outlines are
        // drawn from it).  null switches it off and frees its buffers.
        this.setSelectionOverlay = (options) => {
            if (options === null || options === undefined) { this._n.setOverlay(this._h, 0, 0, 0, 0, 0); return; }
            const t = options.tint === undefined ? [1, 0.5, 0] : options.tint, mix = options.mix === undefined ? 0.5 : options.mix;
            if (!t || t.length !== 3) throw new Error("setSelectionOverlay: tint must be [r, g, b]");
            this._n.setOverlay(this._h, 1, +t[0], +t[1], +t[2], +mix);
        };
        this.readOverlay = () => this._n.readOverlay(this._h, this.width, this.height);
        // ---- selection outline (gsr_set_overlay_outline): the overlay image with the selection's edge drawn into it ----
        //   renderer.setSelectionOutline({ color: [1, 1, 1], alpha: 1, threshold: 0.5, width: 2, side: "outer" });
        // A pixel is inside where cover >= threshold; "outer" draws the pixels around the selection within `width` (1 .. 16) of an
        // inside pixel, "inner" the inside pixels within `width` of one that is not.  Needs setSelectionOverlay; null switches it off.
        const SIDES = { outer: 0, inner: 1 };
        this.setSelectionOutline = (options) => {
            if (options === null || options === undefined) { this._n.setOutline(this._h, 0, 0, 0, 0, 0, 0, 0, 0); return; }
            const t = options.color === undefined ? [1, 1, 1] : options.color;
            if (!t || t.length !== 3) throw new Error("setSelectionOutline: color must be [r, g, b]");
            const alpha = options.alpha === undefined ? 1 : options.alpha, threshold = options.threshold === undefined ? 0.5 : options.threshold;
            const width = options.width === undefined ? 2 : options.width;
            if (!Number.isInteger(width)) throw new Error("setSelectionOutline: width must be an integer");
            this._n.setOutline(this._h, 1, +t[0], +t[1], +t[2], +alpha, +threshold, width, code(SIDES, options.side, "outer", "side"));
        };
        this.stats = () => this._n.getTimings(this._h);
        this.deviceInfo = () => this._n.deviceInfo(this._h);
        this.isInitialized = () => initialized;
    }
}

HIPRenderer.createGroupId = () => loadNative().commUniqueId();
// equal bands of whole 32-px compositor columns, the tail clipped to the image (same rule as gsplat_hip.bands.band_edges)
HIPRenderer.bandEdges = (width, world) => {
    const nbx = Math.ceil(width / 32), per = Math.ceil(nbx / world), e = [];
    for (let q = 0; q < world; q++) e.push([Math.min(q * per * 32, width), Math.min((q + 1) * per * 32, width)]);
    return e;
};
// the bins + 1 edges of splatHistogram, by gsr_attr_histogram's f64 rule: w = (hi - lo) / bins, edge(k) = min(lo + k * w, hi), edge(bins) = hi
HIPRenderer.attrEdges = (lo, hi, bins) => {
    const e = new Float64Array(bins + 1), w = (hi - lo) / bins;
    for (let k = 0; k < bins; k++) e[k] = Math.min(lo + k * w, hi);
    e[bins] = hi;
    return e;
};

// the wasm export's drop-in (wasm/wasm.cpp:8-13, call site Worker.ts:39)
function sortHost(viewProj, vertexCount, fBuffer, depthBuffer, depthIndex) {
    loadNative().sortHost(viewProj, vertexCount, fBuffer, depthBuffer || null, depthIndex);
}

// The band matrices that rotate SH coefficients by q = (x, y, z, w) (gsr_sh_rotation; a pure function, no device): Float64Array views
// of D_1 (3 x 3), D_2 (5 x 5) and D_3 (7 x 7), row-major.  q must be finite and not zero; it is normalised.
function shRotation(q) {
    const v = Array.isArray(q) || ArrayBuffer.isView(q) ? new Float64Array(q) : new Float64Array([q.x, q.y, q.z, q.w]);
    const m = loadNative().shRotation(v);
    return [m.subarray(0, 9), m.subarray(9, 34), m.subarray(34, 83)];
}

// One point-to-plane step solved (gsr_surface_solve; a pure function, no device): from matchSurface's { surfacePairs, sums } the small
// rigid motion { transform: Float64Array(12), rms, degenerate }.  degenerate = j + 1 when pivot j of the 6 x 6 system is not above
// its floor (the residuals leave a direction free): transform is then the identity and rms NaN.
function surfaceSolve(sums) {
    const v = Float64Array.from(sums.sums);
    if (v.length !== 29) throw new Error("surfaceSolve: sums holds 29 values");
    return loadNative().surfaceSolve(Number(sums.surfacePairs), v);
}

module.exports = { HIPRenderer, sortHost, shRotation };
module.exports.surfaceSolve = surfaceSolve;
