// TypeScript surface of the MI355X drop-in.  Mirrors the declarations a user of Lanv1/gsplat.js imports
// (src/index.ts:1-12); WebGLRenderer is the HIP renderer.
export class Vector3 {
    readonly x: number; readonly y: number; readonly z: number;
    constructor(x?: number, y?: number, z?: number);
    equals(v: Vector3): boolean;
    add(v: Vector3 | number): Vector3;
    subtract(v: Vector3 | number): Vector3;
    multiply(v: Vector3 | number): Vector3;
    lerp(v: Vector3, t: number): Vector3;
    length(): number;
    distanceTo(v: Vector3): number;
    normalize(): Vector3;
    flat(): number[];
    clone(): Vector3;
}
export class Quaternion {
    readonly x: number; readonly y: number; readonly z: number; readonly w: number;
    constructor(x?: number, y?: number, z?: number, w?: number);
    equals(q: Quaternion): boolean;
    normalize(): Quaternion;
    multiply(q: Quaternion): Quaternion;
    flat(): number[];
    clone(): Quaternion;
    toEuler(): Vector3;
    static FromEuler(e: Vector3): Quaternion;
    static FromMatrix3(m: Matrix3): Quaternion;
}
export class Matrix3 {
    readonly buffer: number[];
    constructor(n11?: number, n12?: number, n13?: number, n21?: number, n22?: number, n23?: number, n31?: number, n32?: number, n33?: number);
    equals(m: Matrix3): boolean;
    multiply(m: Matrix3): Matrix3;
    clone(): Matrix3;
    static Eye(v?: number): Matrix3;
    static Diagonal(v: Vector3): Matrix3;
    static RotationFromQuaternion(q: Quaternion): Matrix3;
    static RotationFromEuler(m: Vector3): Matrix3;
}
export class Matrix4 {
    readonly buffer: number[];
    constructor(...n: number[]);
    equals(m: Matrix4): boolean;
    multiply(m: Matrix4): Matrix4;
    clone(): Matrix4;
}
export interface SceneEvent { type: string }
/** What a renderer hands a Scene while the Scene is its active scene: the Scene's transforms run through it instead of the
 *  JavaScript loops, and the Scene reads its arrays back through it when they are next asked for. */
export interface DeviceScene {
    /** optional: an object identity that is equal for device scenes that are one device copy (renderers whose contexts share a
     *  scene).  The Scene issues every edit and option once per distinct token, through the first such device scene in attach
     *  order; without a token a device scene counts singly. */
    readonly share?: object | null;
    /** the last upload carried no rotations / scales: the Scene's edits run in JavaScript and are uploaded again */
    hostOnly: boolean;
    /** kind 0 translate (x, y, z), 1 rotate (x, y, z, w), 2 scale (x, y, z), 3 limitBox (xMin, xMax, yMin, yMax, zMin, zMax); returns vertexCount */
    transform(kind: number, args: Float64Array): number;
    /** fills the first 8 / 3 / 4 / 3 words per splat of the four arrays */
    read(out: { data: Uint32Array; positions: Float32Array; rotations: Float32Array; scales: Float32Array }): void;
    /** optional: Scene.shFollowsTransforms, told on attach and on every change of the option.  While the option is on, a device scene
     *  without setShFollow and readSh is treated like a host-only one: the edits run in JavaScript and every renderer uploads. */
    setShFollow?(on: boolean): void;
    /** needed with setShFollow: the SH state after a followed limitBox; fills `textures` (8 * shCount words each; null: none) and
     *  `band` (bandsIndices), returns shCount */
    readSh?(textures: [Uint32Array, Uint32Array, Uint32Array] | null, band: Int32Array): number;
    /** optional, the two together: Scene.eraseSelection sets its mask as the device copy's selection (splat i = bit i & 31 of word
     *  i >>> 5), then has the copy erase the selected splats (keep: the others) and return vertexCount.  A device scene without
     *  them is treated like a host-only one for an eraseSelection. */
    setSelection?(words: Uint32Array): void;
    eraseSelected?(keep: boolean): number;
    /** optional: Scene.setHidden sets its mask (the selection's layout; null: nothing hidden) as the device copy's hidden set and
     *  returns the number of hidden splats.  Scene.setHidden throws when an attached device scene has none. */
    setHidden?(words: Uint32Array | null): number;
    /** optional, the two together with setSelection: Scene.translateSelection / rotateSelection / scaleSelection / paintSelection set
     *  their mask as the device copy's selection, then have the copy edit the selected splats.  kind 0 translate (x, y, z), 1 rotate
     *  (x, y, z, w), 2 scale (x, y, z); pivot (x, y, z) or null.  A device scene without them is treated like a host-only one for
     *  these edits. */
    editSelected?(kind: number, args: Float64Array, pivot: Float64Array | null): void;
    paintSelected?(rgba: number, byteMask: number): void;
    /** optional, the two together with setSelection: Scene.duplicateSelection sets its mask as the device copy's selection, then has
     *  the copy duplicate the selected splats behind its last one; Scene.append hands it another Scene's four arrays (m splats).  Both
     *  return vertexCount.  A device scene without them is treated like a host-only one for these calls. */
    duplicateSelected?(): number;
    appendArrays?(data: Uint32Array, positions: Float32Array, rotations: Float32Array, scales: Float32Array, m: number): number;
}
/** The new splats of a growing call: [first, first + count). */
export interface GrownRange { first: number; count: number }
/** Bytes 0..255; absent channels are left alone. */
export interface PaintChannels { r?: number; g?: number; b?: number; a?: number }
export type Vec3Like = Vector3 | [number, number, number] | Float64Array | Float32Array;
export interface SelectionBounds { count: number; min: Float32Array; max: Float32Array }
export type SelectMode = "centre" | "hit";
export type SelectOp = "replace" | "add" | "subtract" | "intersect";
export type ContribStat = "weight" | "peak" | "pixels";
export type SplatAttribute = "x" | "y" | "z" | "distance" | "red" | "green" | "blue" | "opacity" | "scale_x" | "scale_y" | "scale_z" | "scale_min" | "scale_max" |
    "contrib_weight" | "contrib_peak" | "contrib_pixels";
export interface SplatScope { origin?: ArrayLike<number> | { x: number; y: number; z: number } | null; selected?: boolean; visible?: boolean }
export interface SplatStats { count: number; nan: number; min: number; max: number }
export type NeighbourScope = "selected" | "visible";
export interface NeighbourOptions { cap?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number }
export interface SplatNeighbours { counts: Uint32Array; hist: Uint32Array; inScope: number; nonfinite: number; pairBound: number }
export type Plane = ArrayLike<number>;   // (a, b, c, d): a . x + b . y + c . z + d = 0
export interface PlaneFitOptions { hypotheses?: number; seed?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number; scores?: boolean }
export interface PlaneFit { plane: Float64Array | null; found: boolean; best: number; triple: Uint32Array; inliers: number; degenerate: number; inScope: number;
    nonfinite: number; hypotheses: number; tests: number; scores?: Uint32Array }
export type RigidTransform = ArrayLike<number>;   // 12 numbers, row-major 3 x 4 (R | t)
export interface MatchOptions { transform?: RigidTransform | null; scope?: NeighbourScope | NeighbourScope[]; targetScope?: NeighbourScope | NeighbourScope[]; budget?: number }
export interface SceneMatch { idx: Uint32Array; d2: Float64Array; inScope: number; nonfinite: number; targetIndexed: number; matched: number; pairBound: number;
    d2Min: number; d2Max: number; pairs?: number; sums?: Float64Array }
export type RegisterStatus = "converged" | "max_iterations" | "too_few";
export interface Registration { transform: Float64Array; rotation: Quaternion; translation: Vector3; status: RegisterStatus; iterations: number; pairs: number;
    rms: number; stepPairs?: Float64Array; stepRms?: Float64Array }
/** How a target's normals are made for point-to-plane registration: its splats' own shortest axes (the default), or the PCA of the
 *  k (2 .. 32, default 8) nearest within radius, as splatNormals. */
export interface SurfaceNormals { source?: "own" | "knn"; radius?: number; k?: number; budget?: number }
export type SurfaceRegisterStatus = RegisterStatus | "degenerate";
export interface SurfaceRegistration { transform: Float64Array; rotation: Quaternion; translation: Vector3; status: SurfaceRegisterStatus; iterations: number; pairs: number;
    surfacePairs: number; rms: number; surfaceRms: number; delta: number; valid: number; stepPairs?: Float64Array; stepSurfacePairs?: Float64Array; stepRms?: Float64Array;
    stepSurfaceRms?: Float64Array }
export interface SurfaceMatch { pairs: number; surfacePairs: number; sums: Float64Array; inScope: number; nonfinite: number; targetIndexed: number; matched: number;
    pairBound: number; d2Min: number; d2Max: number }
export interface ClusterOptions { minPts?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number }
export interface SplatClusters { labels: Uint32Array; sizes: Uint32Array; inScope: number; nonfinite: number; pairBound: number; core: number; border: number;
    noise: number; clusters: number; largestLabel: number; largestSize: number }
export type KnnStat = "kth" | "mean";
export interface KnnOptions { k?: number; stat?: KnnStat; scope?: NeighbourScope | NeighbourScope[]; budget?: number }
export interface SplatKnn { found: Uint32Array; values: Float64Array; hist: Uint32Array; idx?: Uint32Array; d2?: Float64Array; inScope: number; nonfinite: number;
    pairBound: number; complete: number; finiteValues: number; valueMin: number; valueMax: number }
export type NormalSource = "knn" | "own";
export type NormalStat = "dot" | "abs_dot" | "variation";
export interface NormalOptions { k?: number; source?: NormalSource; toward?: ArrayLike<number>; scope?: NeighbourScope | NeighbourScope[]; budget?: number }
export interface SplatNormals { normals: Float32Array; variation: Float64Array; found: Uint32Array; inScope: number; nonfinite: number; pairBound: number;
    valid: number; variationMin: number; variationMax: number }
export interface CellOptions { scope?: NeighbourScope | NeighbourScope[]; budget?: number }
export interface CellInfo { inScope: number; candidates: number; cells: number; mergedCells: number; mergedMembers: number; largest: number; rowsAfter: number;
    pairBound: number }
export interface SplatCells extends CellInfo { hist: Uint32Array; leader?: Uint32Array }
export interface SplatHistogram { counts: Uint32Array; below: number; above: number; nan: number; edges: Float64Array }
export interface Contribution { weight: BigUint64Array; peak: Float32Array; pixels: Uint32Array; frames: number }
/** A screen region: the pixels [x0, x1) x [y0, y1), optionally one byte per pixel of the rectangle (non-zero = inside; rows
 *  `stride` >= x1 - x0 apart, default x1 - x0; row 0 is y0): a rasterised lasso or brush. */
export interface SelectRegion { x0: number; y0: number; x1: number; y1: number; mask?: Uint8Array; stride?: number }
export class Scene {
    static RowLength: number;
    constructor();
    addEventListener(type: string, listener: (e: SceneEvent) => void): void;
    removeEventListener(type: string, listener: (e: SceneEvent) => void): void;
    hasEventListener(type: string, listener: (e: SceneEvent) => void): boolean;
    dispatchEvent(e: SceneEvent): void;
    setData(data: Uint8Array, shs?: Float32Array): void;
    translate(translation: Vector3): void;
    rotate(rotation: Quaternion): void;
    scale(scale: Vector3): void;
    limitBox(xMin: number, xMax: number, yMin: number, yMax: number, zMin: number, zMax: number): void;
    /** Remove the splats whose bit of `mask` is set (HIPRenderer.readSelection()'s layout; at least ceil(vertexCount / 32) words),
     *  or with { keep: true } the others: order-preserving, with limitBox's bookkeeping.  While device scenes are attached the mask
     *  is set on every distinct device copy and erased there; otherwise the same loop runs here.  Fires "change". */
    eraseSelection(mask: Uint32Array, options?: { keep?: boolean }): void;
    /** Hide the splats whose bit of `mask` is set (HIPRenderer.readHidden()'s layout; at least ceil(vertexCount / 32) words); null
     *  shows all.  The hidden set exists on the device copies only: it is set once on every distinct device copy, the arrays do not
     *  change and no "change" fires.  Throws when no renderer holds the scene, when the copies are behind the arrays, or when a
     *  device scene cannot take it.  Returns the number of hidden splats. */
    setHidden(mask: Uint32Array | null): number;
    /** Edit the splats whose bit of `mask` is set (HIPRenderer.readSelection()'s layout) and nothing else: what translate / rotate /
     *  scale would leave in a Scene holding only them.  { pivot }: translate(-pivot), the operation, translate(+pivot) on them, each
     *  step rounded to f32.  While device scenes are attached the mask is set on every distinct device copy and the edit runs
     *  there; otherwise the loops run here over the masked indices.  Fires "change".  rotateSelection / scaleSelection throw while
     *  shFollowsTransforms is on and the scene has SH rows. */
    translateSelection(mask: Uint32Array, v: Vector3): void;
    rotateSelection(mask: Uint32Array, q: Quaternion, options?: { pivot?: Vec3Like }): void;
    scaleSelection(mask: Uint32Array, s: Vector3, options?: { pivot?: Vec3Like }): void;
    /** data[8i + 7] of the masked splats: r, g, b in the low three bytes, opacity in the top one; absent channels are left alone */
    paintSelection(mask: Uint32Array, rgba: PaintChannels): void;
    /** Grow the scene: the splats whose bit of `mask` is set, in ascending order, copied bit for bit behind the last splat
     *  (duplicateSelection), or all of another Scene's splats (append; its SH rows are not carried).  Existing indices do not move.
     *  While device scenes are attached the call is issued once per distinct device copy, where the new splats become the
     *  selection; otherwise the four arrays are concatenated here.  Fires "change".  Both throw while the scene has SH rows. */
    duplicateSelection(mask: Uint32Array): GrownRange;
    append(other: Scene): GrownRange;
    static rgbaWord(rgba: PaintChannels): [number, number];
    saveToFile(name: string): void;
    toSplatBytes(): Uint8Array;
    data: Uint32Array; vertexCount: number; width: number; height: number;
    positions: Float32Array; rotations: Float32Array; scales: Float32Array;
    shs: Uint32Array; shs_rgb: [Uint32Array, Uint32Array, Uint32Array]; shHeight: number;
    g0bands: number; bandsIndices: Int32Array;
    /** While device scenes are attached (HIPRenderer.render / renderAsync attach, dispose and another scene detach), translate /
     *  rotate / scale / limitBox run on every one of them and `data`, `positions`, `rotations`, `scales` are refreshed from the
     *  first when they are next read; setData and assigning a buffer make the host the truth again. */
    attachDevice(device: DeviceScene): void;
    detachDevice(device: DeviceScene): void;
    /** true inside the "change" of an edit the attached device scenes have applied already (nothing to upload) */
    readonly deviceEditApplied: boolean;
    /** limitBox ran on the device, which drops the SH state there: the SH textures are not sent again before the next setData */
    readonly shDroppedOnDevice: boolean;
    /** SH colour follows rotate / scale / limitBox (default false: the reference's behaviour).  On: rotate / scale keep `shFrame` up
     *  and the renderer evaluates SH for the direction in the coefficients' own frame; limitBox compacts `shs_rgb` and recounts
     *  `bandsIndices` (on the device while attached: the three are then mirrors, like the four arrays), `shDroppedOnDevice` stays
     *  false; a scale with a component that is 0 or not finite throws. */
    shFollowsTransforms: boolean;
    /** 3x3 row-major: the inverse of the linear part of every rotate / scale since setData (the identity after setData) */
    readonly shFrame: Float64Array;
}
export class Camera {
    position: Vector3; rotation: Quaternion;
    fx: number; fy: number; near: number; far: number;
    projectionMatrix: Matrix4; viewMatrix: Matrix4; viewProj: Matrix4; viewToWorld: Matrix4;
    constructor(position?: Vector3, rotation?: Quaternion, fx?: number, fy?: number, near?: number, far?: number);
    update(width: number, height: number): void;
    setFromData(data: any): void;
    static fromData(data: any): Camera;
    dumpSettings(width: number, height: number): object;
    addEventListener(type: string, listener: (e: SceneEvent) => void): void;
    removeEventListener(type: string, listener: (e: SceneEvent) => void): void;
}
export class ShaderPass { init(renderer: HIPRenderer, program: null): void; render(): void; }
export class FadeInPass implements ShaderPass {
    constructor(speed?: number);
    init(renderer: HIPRenderer, program: null): void;
    render(): void;
}
export interface HIPRendererOptions {
    width?: number; height?: number; device?: number;
    /** 0 (default): composite every splat like the reference; >0: a tile stops once every pixel's 1-alpha is below this */
    earlyOutEps?: number;
    /** multi-GPU: composite only pixel columns [x0, x1) */
    band?: [number, number];
    timing?: boolean;
    /** several renderers keep frames in flight on one device (GSR_FLAG_THROUGHPUT): longer compositor work items */
    throughput?: boolean;
    /** another renderer of the same device: when render / renderAsync attaches a Scene that renderer has attached (its device copy
     *  current), this one shares that device copy (gsr_share_scene) instead of uploading the scene again.  A "change" that makes the
     *  renderers upload (setData, a buffer assigned by hand) is uploaded once, by that renderer, and shared again by this one. */
    shareSceneWith?: HIPRenderer;
}
export interface FrameStats {
    msProjectKey: number; msSort: number; msBin: number; msBlend: number; msCombine: number; msTotal: number;
    visible: number; binEntries: number; tileEntries: number; n: number; frames: number;
}
export type DeliveryFormat = "rgba8" | "nv12" | "i420";
export interface DeliveryOptions {
    /** "rgba8" (default), or 4:2:0 Y'CbCr (BT.709) for a video encoder: "nv12" (Y, interleaved CbCr) / "i420" (Y, Cb, Cr) */
    format?: DeliveryFormat;
    /** Y'CbCr: 0..255 ("pc", yuvj420p) instead of limited range 16..235 / 16..240 ("tv"); default false */
    fullRange?: boolean;
    /** Y'CbCr carries no alpha: the [R, G, B] bytes the premultiplied frame is laid over; default black */
    background?: [number, number, number];
    /** a depth plane beside every frame, for a client that reprojects between server frames (not in a group) */
    depth?: DepthDeliveryOptions;
    /** deliver the selection overlay (setSelectionOverlay first) in place of the frame; default false (not in a group) */
    overlay?: boolean;
}
export type DepthDeliveryFormat = "f32" | "u16";
export interface DepthDeliveryOptions {
    /** "u16" (default): 16-bit inverse depth against `near` -- 0 no hit, 65535 at or in front of `near`, z ~ near * 65535 / u;
     *  "f32": the hit depth as it is, +Infinity without a hit */
    format?: DepthDeliveryFormat;
    /** 1 (default) or 2: the plane holds pixel (step * i, step * j) at (i, j): ceil(width / step) x ceil(height / step) samples */
    step?: 1 | 2;
    /** "u16": the depth that maps to 65535; > 0, default 0.1 */
    near?: number;
}
export interface DepthLayout {
    format: DepthDeliveryFormat; step: number; width: number; height: number;
    /** bytes per row, and where the plane lies in the slot's ArrayBuffer (`depth.byteOffset`) */
    stride: number; offset: number; bytes: number; near: number;
}
/** a view of one plane of a delivered frame, `rows` rows of `stride` bytes */
export type DeliveredPlane = Uint8Array & { stride: number; rows: number };
export interface DeliveryLayout {
    format: DeliveryFormat; width: number; height: number;
    /** the payload: `pixels.length` */
    bytes: number;
    planes: { offset: number; stride: number; rows: number }[];
}
export interface DeliveredFrame {
    serial: number;
    /** RGBA8, row 0 = top: byte for byte what readPixels() returns for that frame.  On an "nv12" / "i420" ring: the whole
     *  payload, planes tightly packed -- what `ffmpeg -f rawvideo -pix_fmt nv12 | yuv420p` reads; write it to a pipe as it is */
    pixels: Uint8Array;
    width: number; height: number;
    format: DeliveryFormat;
    /** views of `pixels.buffer`: one for "rgba8", Y and CbCr for "nv12", Y, Cb and Cr for "i420" */
    planes: DeliveredPlane[];
    /** a depth ring only: the SAME frame's hit depth, row 0 = top, `depthLayout.width` x `depthLayout.height` samples; a view of
     *  `pixels.buffer` behind the colour payload, valid until release() */
    depth?: Uint16Array | Float32Array;
    depthLayout?: DepthLayout;
    release(): void;
}
export class HIPRenderer {
    width: number; height: number;
    constructor(targetOrOptions?: HIPRendererOptions | { width: number; height: number } | null, shaderPasses?: ShaderPass[] | null);
    render(scene: Scene, camera: Camera): void;
    /** enqueue the frame and return; pair with sync() (several `throughput` renderers used round-robin keep the GPU full) */
    renderAsync(scene: Scene, camera: Camera): void;
    /** waits for the enqueued frames; throws once if asynchronous frames were lost to a list overflow (the renderer stays usable) */
    sync(): void;
    overflowPending(): boolean;
    setListCapacity(entries: number): void;
    /** multi-GPU, one process per GPU. Collective: same id (createGroupId() on rank 0), world and edges on every rank.
     *  Afterwards render() draws this rank's tile-column band and all-gathers the RGBA8 frame over xGMI inside the
     *  library (RCCL); readPixels() returns the whole frame on every rank. */
    joinGroup(group: { id: Uint8Array; rank: number; world: number; edges: Array<[number, number]>; depth?: DepthDeliveryOptions }): void;
    /** Depth in a group: every rank exchanges its band's hit depth beside the colour slab (the same options on every rank and sharer;
     *  null switches it off).  openDelivery(n, { depth }) with these options then works in the group. */
    setGroupDepth(depth: DepthDeliveryOptions | null): void;
    /** the gathered plane of the last frame, frameDepthLayout().width x .height samples, row 0 = top */
    readFrameDepth(): Uint16Array | Float32Array;
    frameDepthLayout(): DepthLayout;
    /** Another renderer of the same rank (frames in flight) joins the group `leader` has joined: one communicator and one
     *  exchange stream per rank (gsr_comm_share).  Leave (or dispose) it before the leader. */
    shareGroup(leader: HIPRenderer): void;
    leaveGroup(): void;
    group(): { rank: number; world: number } | null;
    static createGroupId(): Uint8Array;
    static bandEdges(width: number, world: number): Array<[number, number]>;
    sort(camera?: Camera): void;
    setSize(width: number, height: number): void;
    resize(): void;
    setBand(x0: number, x1: number): void;
    setCameraBuffers(): void;
    setShTextures(): void;
    setDepthFade(useDepthFade: boolean, depthFade: number): void;
    /** device-side scene: .splat rows in; Scene.setData and the transforms run as kernels, bit-identical to Scene */
    setSceneRows(rows: Uint8Array): void;
    sceneTranslate(t: Vector3): void;
    sceneRotate(q: Quaternion): void;
    sceneScale(s: Vector3): void;
    sceneLimitBox(xMin: number, xMax: number, yMin: number, yMax: number, zMin: number, zMax: number): void;
    readSceneData(): { data: Uint32Array; positions: Float32Array; vertexCount: number };
    renderDeviceScene(camera: Camera): void;
    /** give up this renderer's scene and render `other`'s device scene from now on: nothing is copied or uploaded; edits through
     *  either renderer (or the Scene) change the one copy.  setSceneRows, or a Scene that is uploaded, takes the renderer out again. */
    shareScene(other: HIPRenderer): void;
    /** renderers that render this renderer's device scene (1: not shared) and the device bytes they hold once */
    sceneSharing(): { members: number; sceneBytes: number };
    /** Selection: one bit per splat of the device scene (renderers that share a scene have one together).  selectRegion picks by a
     *  region of the last rendered frame -- "centre": the listed splats whose centre pixel lies in it; "hit": the splats that are the
     *  hit of one of its pixels (readDepth().index) -- and folds the picked set into the selection with `op`; every call returns the
     *  number of selected splats.  Scene.eraseSelection(renderer.readSelection()) then removes them everywhere. */
    selectRegion(region: SelectRegion, options?: { mode?: SelectMode; op?: SelectOp }): number;
    /** the splats inside [xMin, xMax, yMin, yMax, zMin, zMax]: limitBox's comparisons; needs no frame */
    selectBox(box: ArrayLike<number>, options?: { op?: SelectOp }): number;
    /** fold the host's own words into the selection (null: the empty set); bits at and above vertexCount are dropped */
    setSelection(words: Uint32Array | null, op?: SelectOp): number;
    invertSelection(): number;
    /** ceil(vertexCount / 32) words: splat i is bit i & 31 of word i >>> 5 */
    readSelection(): Uint32Array;
    /** Hidden splats: one more bit per splat of the device scene (renderers that share a scene have one set together).  A hidden
     *  splat is in no list of the frames rendered from now on -- not drawn, not picked, no depth, no contribution, no overlay -- and
     *  nothing is erased: the splats keep their numbers, and the set survives limitBox / eraseSelection of other splats.
     *  hideSelection folds the selection into the hidden set (default "add": hide; "subtract": show; "replace"; "intersect"), showAll
     *  empties it, setHidden folds the host's own words (null: the empty set), selectHidden folds the hidden set into the selection.
     *  A change is a scene edit: pick, selectRegion and readDepth need a new frame.  Each returns the number of hidden (selectHidden:
     *  selected) splats. */
    hideSelection(options?: { op?: SelectOp }): number;
    showAll(): number;
    setHidden(words: Uint32Array | null, options?: { op?: SelectOp }): number;
    /** ceil(vertexCount / 32) words: splat i is bit i & 31 of word i >>> 5 */
    readHidden(): Uint32Array;
    selectHidden(options?: { op?: SelectOp }): number;
    /** Editing the selection on THIS renderer's device copy (a Scene attached to it does not learn of it: Scene.translateSelection
     *  and its kin edit every copy and the Scene's arrays).  selectionBounds: the selected splats' count and the box of their centres
     *  (nothing selected: 0, +Infinity, -Infinity; a NaN coordinate is counted and never enters the box).  The edits leave what
     *  Scene.translate / rotate / scale would leave in a Scene holding only the selected splats; { pivot }: translate(-pivot), the
     *  operation, translate(+pivot).  paintSelection writes the given channels' bytes.  Each is a scene edit: pick, selectRegion and
     *  readDepth need a new frame; selection, hidden set and contribution state stay.  rotate / scale throw while SH follows the
     *  transforms and the scene has SH rows. */
    selectionBounds(): SelectionBounds;
    translateSelection(v: Vec3Like): void;
    rotateSelection(q: Quaternion | [number, number, number, number] | Float64Array, options?: { pivot?: Vec3Like; sh?: boolean }): void;
    scaleSelection(s: Vec3Like, options?: { pivot?: Vec3Like }): void;
    paintSelection(rgba: PaintChannels): void;
    /** Rotating SH coefficients on THIS renderer's device copy.  rotateSH rotates, in place, the coefficients of every SH row (or of
     *  the selected splats' rows) by q and returns the rows rotated; the SH frame is neither read nor written.
     *  rotateSelection(q, { pivot, sh: true }) turns the selected splats and their coefficients as one edit; it is allowed with
     *  shFollowsTransforms on or off while the SH frame is the identity and throws otherwise -- bakeSHFrame() moves a frame that is
     *  a rotation times a positive uniform scale into the coefficients (throws for any other frame) and returns the rotation it
     *  used.  `sh` defaults to false: today's rotateSelection.  Each is a scene edit; an attached Scene's shs_rgb mirror is marked
     *  stale and read back from the device on its next use. */
    rotateSH(q: Quaternion | [number, number, number, number] | Float64Array, options?: { selected?: boolean }): number;
    bakeSHFrame(): Quaternion;
    /** Growing THIS renderer's device copy (Scene.duplicateSelection / Scene.append grow every copy and the Scene's arrays).
     *  duplicateSelection copies the selected splats bit for bit behind the last splat; appendSelectionFrom copies the splats selected
     *  in another renderer of the same GPU, device to device (that renderer is not changed, its SH rows are not carried).  The new
     *  splats [first, first + count) become the selection; existing indices, the hidden set and the contribution state stay.  With
     *  nothing selected nothing changes and the last frame stays valid.  reserveScene makes the device arrays hold at least `rows`
     *  splats, so that copies up to that count re-allocate nothing; sceneCapacity returns what they hold.  The growing calls throw
     *  while the device scene has SH rows. */
    reserveScene(rows: number): void;
    sceneCapacity(): number;
    duplicateSelection(): GrownRange;
    appendSelectionFrom(other: HIPRenderer): GrownRange;
    /** Contribution: per splat of the device scene (renderers that share a scene have one set together), what it showed over the
     *  frames of a tour.  resetContribution zeroes the accumulators (blocking); accumulateContribution enqueues the pass behind the
     *  frame rendered last (no wait; a frame whose lists did not fit adds nothing); readContribution returns weight (sum of the
     *  fragment weights in quanta of 2^-24), peak (the largest weight), pixels (the pixels covered, modulo 2^32) and frames (the
     *  passes counted); selectContribution picks the splats whose value -- weight * 2^-24, peak or pixels -- is below `below` and
     *  folds them into the selection with `op`, returning the number of selected splats.  It throws while no pass has contributed. */
    resetContribution(): void;
    accumulateContribution(): void;
    readContribution(): Contribution;
    selectContribution(options?: { stat?: ContribStat; below?: number; op?: SelectOp }): number;
    /** Splat data: how an attribute of the splats themselves is distributed over the device scene, and a range of it as a picker.
     *  splatStats: the splats in scope (selected: only the selection; visible: only what is not hidden), how many have a NaN value,
     *  and min / max of the others (Infinity, -Infinity when there are none).  splatHistogram: the values in [lo, hi) in `bins` bins
     *  (1 .. 4096, default 64) by the edge rule of HIPRenderer.attrEdges -- a value's bin is the last one whose edge is <= it -- plus
     *  the splats in scope below lo, at or above hi, and NaN.  selectAttribute picks lo <= value < hi over every splat (defaults
     *  -Infinity, Infinity; never a NaN) and folds them into the selection with `op`, returning the number of selected splats:
     *  selectAttribute(attr, { lo: edges[a], hi: edges[b] }) selects exactly the splats an unscoped histogram counts in bins a .. b - 1.
     *  origin is what "distance" is measured from.  Scale attributes need a scene with rotations / scales, contribution attributes a
     *  tour; unknown names throw. */
    splatStats(attr: SplatAttribute, options?: SplatScope): SplatStats;
    splatHistogram(attr: SplatAttribute, options: SplatScope & { lo: number; hi: number; bins?: number }): SplatHistogram;
    selectAttribute(attr: SplatAttribute, options?: { lo?: number; hi?: number; origin?: SplatScope["origin"]; op?: SelectOp }): number;
    static attrEdges(lo: number, hi: number, bins: number): Float64Array;
    /** Neighbours: for every splat in scope (scope: "selected", "visible" or both; none: every splat) the number of OTHER splats in
     *  scope within `radius` of it -- f64, distance exactly radius counts, a splat never counts itself -- at most `cap` (1 .. 4095,
     *  default 64); 0 outside the scope.  splatNeighbours: counts per splat, hist[k] = the splats in scope with k neighbours
     *  (hist[cap]: cap or more; the histogram sums to inScope), nonfinite = splats in scope with a NaN or infinite position (count 0),
     *  pairBound = the most pair tests the count pass makes.  selectNeighbours picks lo <= count < hi (below: { lo: 0, hi: below };
     *  default hi cap + 1) and folds them into the selection with `op`, returning the number of selected splats: with "replace"
     *  exactly hist.slice(lo, hi) summed.  selectNeighbours(r, { below: k }) then Scene.eraseSelection(readSelection()) is the radius
     *  outlier filter.  Both index the device scene as it is now.  budget: the most pair tests a call may make (default 2^34, at
     *  most 2^38); a radius that needs more throws before the count pass runs, with both numbers in the message. */
    splatNeighbours(radius: number, options?: NeighbourOptions): SplatNeighbours;
    selectNeighbours(radius: number, options?: NeighbourOptions & { below?: number; lo?: number; hi?: number; op?: SelectOp }): number;
    /** Planes: fitPlane finds the dominant plane of the splats in scope by RANSAC on the device -- `hypotheses` (1 .. 4096, default
     *  512) planes through three splats each, drawn by a counter-based generator from `seed`, every one scored in f64 by the splats
     *  within `threshold` of it (a distance of exactly threshold counts); the largest score wins, ties go to the smallest index.
     *  plane: (nx, ny, nz, d) with a unit normal, null when every hypothesis was degenerate; scores: true adds every hypothesis's
     *  score.  planeInliers scores up to 4096 planes of the host's, used as given.  selectPlane picks lo <= signed distance <= hi
     *  over all splats (within: t is { lo: -t, hi: t }; a NaN distance is never picked) and folds them into the selection with `op`,
     *  returning the number of selected splats: after an unscoped fit, selectPlane(plane, { within: threshold }) selects exactly
     *  `inliers` splats, and selectPlane(plane, { hi: -t }) is everything under the floor.  planeAlignment returns the whole-scene
     *  rotation and translation that take the plane to axis . p = 0 (axis: default +y): scene.rotate(rotation);
     *  scene.translate(translation).  budget: the most tests (hypotheses x candidates) a call may make (default 2^34, at most 2^38);
     *  more throws before the scoring pass runs, with both numbers in the message. */
    fitPlane(threshold: number, options?: PlaneFitOptions): PlaneFit;
    planeInliers(planes: ArrayLike<Plane>, threshold: number, options?: { scope?: NeighbourScope | NeighbourScope[]; budget?: number }): Uint32Array;
    selectPlane(plane: Plane, options?: { within?: number; lo?: number; hi?: number; op?: SelectOp }): number;
    planeAlignment(plane: Plane, options?: { axis?: ArrayLike<number> | Vector3 }): { rotation: Quaternion; translation: Vector3 };
    /** Matching and registration: matchScene finds, for every splat in scope moved by `transform` (12 numbers, row-major 3 x 4
     *  (R | t); default the identity), the nearest splat of `target`'s scene in targetScope within `radius` -- f64, smallest in
     *  (squared distance, index), a distance of exactly radius counts: idx[i] its index (0xffffffff without one), d2[i] the squared
     *  distance (Infinity without one, NaN outside the scope); sums: true adds pairs and the 16 sums a rigid solve takes.  selectMatch
     *  picks lo <= distance < hi (hi undefined or Infinity: no upper end, the unmatched splats included) and folds them into the
     *  selection with `op`: { hi: r } is what the other capture already has, { lo: r } what it lacks.  registerTo iterates match,
     *  reduce and solve from `transform` and returns the rigid transform that takes this scene onto the target's, with its rotation
     *  and translation: scene.rotate(rotation); scene.translate(translation).  It stops "converged" when a step moves no entry by more
     *  than `tolerance` (default 2^-40), "too_few" when a step matches fewer than 3 splats, "max_iterations" after maxIterations
     *  (1 .. 256, default 32) steps; history: true adds every step's pairs and rms.  Neither device scene is written, and the same
     *  scenes give the same bits on every run.  rigidDecompose splits any such transform.  budget as splatNeighbours. */
    matchScene(target: HIPRenderer, radius: number, options?: MatchOptions & { sums?: boolean }): SceneMatch;
    selectMatch(target: HIPRenderer, radius: number, options?: MatchOptions & { lo?: number; hi?: number; op?: SelectOp }): number;
    registerTo(target: HIPRenderer, radius: number, options?: MatchOptions & { maxIterations?: number; tolerance?: number; history?: boolean }): Registration;
    rigidDecompose(transform: RigidTransform): { rotation: Quaternion; translation: Vector3 };
    /** Point-to-plane registration: registerTo with residual "surface" pulls every splat toward the target's SURFACE along the normal
     *  of its match, not toward the nearest sample: far fewer steps on floors, walls and table tops, and no biased pose.  normals
     *  says how the target's normals are made, once per call.  It stops "too_few" with fewer than 6 pairs that have a normal and
     *  "degenerate" when the residuals leave a direction free (a target of one or two planes).  residual "point", the default, is
     *  registerTo as above.  matchSurface is one such step as data: the 29 sums SPLAT.surfaceSolve takes. */
    registerTo(target: HIPRenderer, radius: number, options: MatchOptions & { residual: "surface"; normals?: SurfaceNormals; maxIterations?: number; tolerance?: number;
        history?: boolean }): SurfaceRegistration;
    registerTo(target: HIPRenderer, radius: number, options: MatchOptions & { residual: "point"; maxIterations?: number; tolerance?: number; history?: boolean }): Registration;
    matchSurface(target: HIPRenderer, radius: number, options?: MatchOptions & { normals?: SurfaceNormals }): SurfaceMatch;
    /** Clusters: the connected islands of the splats in scope at the linking radius `radius` (f64, distance exactly radius links).
     *  minPts (0 .. 4095, default 0: plain connected components) makes it DBSCAN: a splat with minPts or more others within radius is
     *  core, core splats within radius of each other share a cluster, a non-core splat beside a core one takes the smallest such
     *  label (border), the rest is noise.  splatClusters: labels[i] = the smallest splat index of i's cluster (0xffffffff: noise, not
     *  finite, outside the scope), sizes[i] = the splats labelled like i (0 without a label), and the counts: inScope == core + border +
     *  noise, clusters, largestLabel / largestSize (ties: the smallest label; 0xffffffff / 0 without a cluster).  selectClusters picks
     *  the splats in scope with atLeast <= size < below (defaults 0 and no upper end) and folds them into the selection with `op`,
     *  returning the number of selected splats: selectClusters(r, { below: k }) then Scene.eraseSelection(readSelection()) removes noise
     *  and every island smaller than k.  selectClusterAt picks the cluster of splat `seed` (pick(x, y).index: the island under the
     *  cursor) or, with largest: true, the largest one; a seed that is noise or outside the scope picks nothing.  All index the device
     *  scene as it is now; budget as splatNeighbours takes it, for each of up to three walks. */
    splatClusters(radius: number, options?: ClusterOptions): SplatClusters;
    selectClusters(radius: number, options?: ClusterOptions & { below?: number; atLeast?: number; op?: SelectOp }): number;
    selectClusterAt(radius: number, options: ClusterOptions & { seed?: number; largest?: boolean; op?: SelectOp }): number;
    /** k nearest neighbours: for every splat in scope the k (1 .. 32, default 8) nearest OTHER splats in scope within `radius`,
     *  ascending by (squared distance, index), equal distances to the smaller index.  splatKnn: found[i] = how many there are;
     *  with lists: true, idx and d2 hold their indices and squared distances, row i at [i * k], padded with 0xffffffff / Infinity;
     *  values[i] = the distance to the k-th (stat "kth"; Infinity without one) or the mean distance to those found (stat "mean",
     *  the default; Infinity with none), NaN outside the scope; hist[t] = the splats in scope with found == t; complete = those
     *  with k; finiteValues, valueMin / valueMax over the finite values.  selectKnn picks lo <= value < hi (hi undefined or
     *  Infinity: no upper end, the Infinity values included) and folds them into the selection with `op`, returning the number of
     *  selected splats.  selectStatisticalOutliers is statistical outlier removal: it picks value >= threshold = mean + stdRatio
     *  (default 2) * sample standard deviation of the finite mean distances, the splats without a neighbour included; then
     *  Scene.eraseSelection(readSelection()) removes them.  All index the device scene as it is now; budget as splatNeighbours. */
    splatKnn(radius: number, options?: KnnOptions & { lists?: boolean }): SplatKnn;
    selectKnn(radius: number, options?: KnnOptions & { lo?: number; hi?: number; op?: SelectOp }): number;
    selectStatisticalOutliers(radius: number, options?: { k?: number; stdRatio?: number; scope?: NeighbourScope | NeighbourScope[]; budget?: number; op?: SelectOp }): { selected: number; threshold: number };
    /** Normals: a unit surface normal per splat in scope, row i of normals at [3 * i].  source "knn" (the default): the eigenvector
     *  of the smallest eigenvalue of the covariance of the splat and its k (2 .. 32, default 8) nearest others in scope within
     *  `radius` (splatKnn's lists; at least two are needed); "own": the splat's own shortest axis, no index and no walk (radius is
     *  not read; the scene must carry rotations and scales).  variation[i] = l_min / (l_0 + l_1 + l_2): 0 on a plane, large at edges
     *  and corners.  toward: [x, y, z]: every normal faces that viewpoint; without it the first non-zero component is positive.  A
     *  splat without a normal holds NaN in both; found[i] = the length of its list (0 for "own"); valid = the splats with a normal,
     *  variationMin / variationMax over them.  selectNormal picks lo <= value <= hi, both ends closed (lo default -Infinity, hi
     *  default Infinity), the value computed from the stored float32 normal: "dot" n . axis, "abs_dot" |n . axis| (for normals that
     *  are not oriented: selectNormal("abs_dot", { axis: up, hi: 0.2, radius }) is "the walls"), "variation" (no axis); axis is
     *  used as given, not normalised.  It folds them into the selection with `op` and returns the number of selected splats.
     *  Both index the device scene as it is now; budget as splatNeighbours. */
    splatNormals(radius: number | undefined, options?: NormalOptions): SplatNormals;
    selectNormal(stat: NormalStat, options?: NormalOptions & { radius?: number; axis?: ArrayLike<number>; lo?: number; hi?: number; op?: SelectOp }): number;
    /** Merging cells: voxel simplification of this renderer's device copy.  The candidates -- the splats in scope with finite
     *  position, rotation and scale -- fall into the cells of a grid of side `cell`.  splatCells is the report: hist[k] = the cells
     *  with k members (hist[cap]: cap or more; cap 1 .. 4095, default 64), with leaders: true leader[i] = the smallest candidate
     *  index of i's cell (0xffffffff: no candidate), rowsAfter = the rows mergeCells would leave.  mergeCells replaces every cell of
     *  two or more by one splat -- the opacity x volume weighted mean, the covariance of the mixture, a rotation and scale from its
     *  eigen-decomposition -- at the smallest member's row and removes the other members in order; count === rowsAfter of the
     *  report, and the selection becomes exactly the merged rows.  Nothing to merge: nothing changes.  It acts on the device copy
     *  like rotateSelection; a scene with SH rows is refused; budget as splatNeighbours. */
    splatCells(cell: number, options?: CellOptions & { cap?: number; leaders?: boolean }): SplatCells;
    mergeCells(cell: number, options?: CellOptions): CellInfo & { count: number };
    dispose(): void;
    /** RGBA8, row 0 = top, round(clamp(x,0,1)*255), premultiplied alpha */
    /** RGBA8, row 0 = top; pass an array of width*height*4 elements to have it filled and returned (no allocation per frame). */
    /** Selection overlay: the frame rendered last with the selected splats drawn in lerp(colour, tint, mix) (tint [r, g, b] as
     *  the framebuffer's channels, mix in [0, 1]; null: off, the buffers are freed).  readOverlay returns the image (premultiplied
     *  RGBA float32, width * height * 4) and cover (width * height: the share of the pixel's alpha that selected splats supply);
     *  readPixels({ overlay: true }) returns the image as RGBA8, and openDelivery(n, { overlay: true }) delivers it in place of
     *  the frame.  Refused in a group. */
    setSelectionOverlay(options: { tint?: [number, number, number]; mix?: number } | null): void;
    readOverlay(): { rgba: Float32Array; cover: Float32Array };
    /** Selection outline: the overlay image with the selection's edge drawn into it (needs setSelectionOverlay; null: off).  A pixel
     *  is inside where cover >= threshold (> 0); side "outer" draws the pixels around the selection within `width` (1 .. 16) of an
     *  inside pixel, "inner" the inside pixels within `width` of one that is not.  An edge pixel becomes lerp(overlay, color, alpha),
     *  its alpha lerp(a, 1, alpha).  readOverlay, readPixels({ overlay: true }) and an overlay ring all show it; cover is unchanged.
     *  Defaults: color [1, 1, 1], alpha 1, threshold 0.5, width 2, side "outer". */
    setSelectionOutline(options: { color?: [number, number, number]; alpha?: number; threshold?: number; width?: number; side?: "outer" | "inner" } | null): void;
    readPixels(options: { overlay?: boolean; out?: Uint8Array }): Uint8Array;
    readPixels(out?: Uint8Array): Uint8Array;
    readPixelsFloat(out?: Float32Array): Float32Array;
    /** Depth planes of the last rendered frame, width*height each, row 0 = top; pass arrays to have them filled (like
     *  readPixels(out)), omit a plane to skip it.  Per pixel, over the fragments of its bin's list front to back, from
     *  T = 1, D = 0: w = T * B; D = fma(w, z, D); T -= w, z being the w of the splat centre's clip position.
     *  mean: D, premultiplied like the colour channels (divide by the framebuffer's alpha for expected depth);
     *  hit: z of the first fragment at which 1 - T reaches the hit alpha, Infinity when none does;
     *  index: that fragment's splat index, 0xffffffff when none. */
    readDepth(out?: { mean?: Float32Array; hit?: Float32Array; index?: Uint32Array }): { mean?: Float32Array; hit?: Float32Array; index?: Uint32Array };
    /** enqueue the depth pass behind the frame enqueued last (no host wait); readDepth() runs it itself when needed */
    depthAsync(): void;
    /** The splat under pixel (x, y) of the last rendered frame: its index (0xffffffff: none), depth (Infinity: none), the
     *  pixel's premultiplied mean depth and alpha, and `point`: the pixel centre un-projected to `depth` through the
     *  active camera -- what to assign to an OrbitControls target; null when nothing is hit. */
    pick(x: number, y: number): { index: number; depth: number; mean: number; alpha: number; point: Vector3 | null };
    /** accumulated alpha at which a pixel's hit is taken, in (0, 1]; default 0.5 */
    setHitAlpha(a: number): void;
    /** Frame delivery: a ring of `slots` (2..8, default 3) pinned RGBA8 frames inside the library.  renderAsync() +
     *  deliverFrame() enqueue a frame and its copy to the host without waiting; acquireFrame() waits for that frame's copy
     *  only, so frame k is presented while k+1 and k+2 render.  Works after joinGroup() too (the gathered frame). */
    openDelivery(slots?: number, options?: DeliveryOptions): void;
    /** the open ring's frame layout at the current size (it follows setSize) */
    deliveryLayout(): DeliveryLayout;
    /** the depth plane of the open depth ring's frames at the current size; throws on a ring without depth */
    depthLayout(): DepthLayout;
    /** throws while a frame is held; detaches the slots' ArrayBuffers (old `pixels` views then have length 0) */
    closeDelivery(): void;
    /** enqueue the delivery of the frame enqueued last; returns its serial (1, 2, 3 ...).  Throws ("... (-7) ...") and
     *  enqueues nothing when every slot is in flight or held. */
    deliverFrame(): number;
    /** has the frame's copy finished?  never blocks.  serial 0 / omitted: the oldest frame not acquired yet */
    frameReady(serial?: number): boolean;
    /** Waits for frame `serial` (omitted: the oldest not acquired yet).  `pixels` views the slot's pinned block -- no copy,
     *  no allocation, `pixels.buffer` is the same ArrayBuffer every lap of the ring -- and stays valid until release().
     *  A frame that was not composited (list overflow) throws ("... (-5) ...") and frees its slot: render that pose again. */
    acquireFrame(serial?: number): DeliveredFrame;
    lastDepthIndex(): Uint32Array;
    stats(): FrameStats;
    deviceInfo(): { name: string; computeUnits: number; clockKhz: number };
}
export { HIPRenderer as WebGLRenderer };
export class Loader {
    static LoadAsync(file: string, scene: Scene, onProgress?: (p: number) => void): Promise<Scene>;
    static LoadFromFileAsync(file: string, scene: Scene, onProgress?: (p: number) => void): Promise<Scene>;
    static LoadSync(file: string, scene: Scene): Scene;
}
export class PLYLoader {
    /** format: "" | "polycam"; useShs: also read the 45 f_rest_* floats; quantized (with useShs): the codebook variant */
    static LoadAsync(file: string, scene: Scene, onProgress?: (p: number, done?: boolean) => void, format?: string,
                     useShs?: boolean, quantized?: boolean): Promise<Scene>;
    static LoadFromFileAsync(file: string, scene: Scene, onProgress?: (p: number, done?: boolean) => void, format?: string,
                             useShs?: boolean, quantized?: boolean): Promise<Scene>;
    static LoadFromBytes(bytes: Uint8Array, scene: Scene, format?: string, useShs?: boolean, quantized?: boolean): Scene;
}
export class OrbitControls {
    minAngle: number; maxAngle: number; minZoom: number; maxZoom: number;
    orbitSpeed: number; panSpeed: number; zoomSpeed: number; dampening: number;
    desiredAlpha: number; desiredBeta: number; desiredRadius: number; desiredTarget: Vector3;
    constructor(camera: Camera, domElement?: unknown, alpha?: number, beta?: number, radius?: number,
                enableKeyboardControls?: boolean, inputTarget?: Vector3);
    setCameraTarget(newTarget: Vector3): void;
    snap(): void;
    update(): void;
    dispose(): void;
    static applyPose(camera: Camera, alpha: number, beta: number, radius: number, target: Vector3): void;
}
/** Drop-in for the wasm export `sort` (wasm/wasm.cpp:8-13) on host typed arrays. */
/** The band matrices [D_1 (3 x 3), D_2 (5 x 5), D_3 (7 x 7)], row-major, that rotate SH coefficients by q (finite, not zero;
 *  normalised): c' = D_l c makes the colour seen from d the colour formerly seen from R(q)^T d.  A pure function: no device. */
export function shRotation(q: Quaternion | [number, number, number, number] | Float64Array): [Float64Array, Float64Array, Float64Array];
/** One point-to-plane step solved (a pure function, no device): the small rigid motion of matchSurface's sums.  degenerate = j + 1
 *  when pivot j of the 6 x 6 system is not above its floor: transform is then the identity and rms NaN. */
export function surfaceSolve(sums: { surfacePairs: number; sums: ArrayLike<number> }): { transform: Float64Array; rms: number; degenerate: number };
export function sortHost(viewProj: Float32Array, vertexCount: number, fBuffer: Float32Array,
                         depthBuffer: Uint32Array | null, depthIndex: Uint32Array): void;
