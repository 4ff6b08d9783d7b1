"use strict";
/**
 * @fluidframework/merge-tree-native — batched, GPU-resident replay of merge-tree op logs.
 *
 * Mirrors the slice of @fluidframework/merge-tree's Client API that the replay / summarize path uses
 * (client.ts:805-836 applyMsg, textSegment.ts:154-172 getText, snapshotV1.ts:85-247 SnapshotV1 emit),
 * but for many documents at once: messages are staged per document and replayed on the MI355X in one
 * launch. There is no CPU fallback — without a HIP device createEngine throws.
 */
const path = require("path");
const addon = require(path.join(__dirname, "build", "mte_native.node"));

const DocStatus = Object.freeze({ Ok: 0, InsertFailed: 1, SequenceOrder: 2, Capacity: 3, Unsupported: 4 });
/** View queries (mte_views): kinds, per-query statuses, the client that owns no slot, the LOCATE flag. */
const ViewKind = Object.freeze({ Length: 0, Locate: 1, Text: 2 });
const ViewStatus = Object.freeze({ Ok: 0, PastEnd: 1, OutOfWindow: 2, DocFailed: 3, BadQuery: 4 });
const VIEW_NO_CLIENT = 0xFFFFFFFF;
const VIEW_F_REMOVED = 1;
/** SharedMatrix reads (mte_matrix_cells): kinds, per-query statuses, the id of "no cell". */
const MatrixQuery = Object.freeze({ Shape: 0, Cell: 1, Rect: 2 });
const MatrixStatus = Object.freeze({ Ok: 0, OutOfRange: 1, DocFailed: 2, BadQuery: 3 });
const CELL_NONE = 0xFFFFFFFF;

/** Marker queries (mte_markers): kinds and per-query statuses. */
const MarkerQuery = Object.freeze({ TileBefore: 0, TileAfter: 1, Paragraphs: 2 });
const MarkerStatus = Object.freeze({ Ok: 0, NotFound: 1, Unsupported: 2, DocFailed: 3, BadQuery: 4 });

class BatchedMergeEngine {
    constructor(options = {}) {
        this.device = options.device || 0;
        this.chunkSize = options.chunkSize || 10000;  // SnapshotV1.chunkSize (snapshotV1.ts:40)
        // newMergeTreeSnapshotFormat (client.ts:930-941): SnapshotV1 only when it is true, else the
        // reference's default, SnapshotLegacy
        this.legacyFormat = options.newMergeTreeSnapshotFormat !== true;
        this._engine = addon.createEngine(this.device, this.chunkSize, this.legacyFormat ? 1 : 0);
        this._docs = 0;
    }
    /** Stage per-document logs: docs = [{ observer, messages: ISequencedDocumentMessage[], summary? }]
     *  summary (optional): a SnapshotV1 ITree to resume from (SnapshotLoader); messages are the suffix. */
    load(docs) {
        this._idle();
        const b = addon.createBuilder();
        for (const d of docs) {
            const obs = d.observer === undefined ? "__observer__" : d.observer;
            if (d.matrix !== undefined && d.summary !== undefined) {  // SharedMatrix summary + suffix
                const s = typeof d.summary === "string" ? d.summary : JSON.stringify(d.summary);
                addon.builderAddMatrixFromSummary(b, obs, s, JSON.stringify(d.matrix));
            } else if (d.matrix !== undefined) {  // SharedMatrix messages: two documents, rows then cols
                addon.builderAddMatrixLog(b, obs, JSON.stringify(d.matrix));
            } else if (d.summary !== undefined) {
                const s = typeof d.summary === "string" ? d.summary : JSON.stringify(d.summary);
                addon.builderAddDocFromSummary(b, obs, s, d.messages ? JSON.stringify(d.messages) : null);
            } else {
                addon.builderAddDoc(b, obs, JSON.stringify(d.messages));
            }
        }
        addon.load(this._engine, b);
        this._docs = addon.builderDocCount(b);
    }
    _loadBuilder(b) {
        this._idle();
        addon.load(this._engine, b);
        this._docs = addon.builderDocCount(b);
    }
    /** mte_retain: keep each document's state after a replay, so replaying logs that extend the last
     *  pass's replays only their new ops (Client.applyMsg's incremental cost, client.ts:805-836). */
    retain(on = true) { this._idle(); addon.retain(this._engine, on); }
    /** op records the last replay did not replay again (continued from the pass before): the row
     *  engines' ("resumed_ops") plus the block engine's ("resumed_ops_blk": documents loaded from a
     *  summary, with relative positions, 64+ clients, ...) */
    resumedOps() {
        this._idle();
        return addon.getInfo(this._engine, "resumed_ops") + addon.getInfo(this._engine, "resumed_ops_blk");
    }
    /** mte_get_info: routing and counters of the last pass ("resumed_docs", "rows", "solo", ...) */
    getInfo(key) { this._idle(); return addon.getInfo(this._engine, key); }
    generate(kind, nDocs, nOps, nClients = 8, seed = 0) {
        this._idle();
        addon.generate(this._engine, kind, nDocs, nOps, nClients, seed);
        this._docs = nDocs;
    }
    replay() {
        this._idle();
        return addon.replay(this._engine);
    }
    /** mte_replay on a worker thread (N-API async work): the event loop keeps running. While it is
     *  pending, every other call on this engine throws (the engine is not re-entrant). */
    replayAsync() {
        this._idle();
        this._busy = true;
        return addon.replayAsync(this._engine).finally(() => { this._busy = false; });
    }
    _idle() { if (this._busy) throw new Error("BatchedMergeEngine: a replayAsync() is still running"); }
    /** Client.getLength() of a document: the observer's visible length, markers counting 1. */
    getLength(doc) { this._idle(); return addon.getLength(this._engine, doc); }
    docStatus(doc) { this._idle(); return addon.docStatus(this._engine, doc); }
    getText(doc) { this._idle(); return addon.getText(this._engine, doc); }
    /**
     * mte_views: positional reads in any client's view, answered on the GPU from the last replay's rows
     * without downloading the batch. queries: [{ doc, refSeq, client, kind, pos1, pos2 }] -- client a short
     * id (clientSlot), 0 = the observer, VIEW_NO_CLIENT = a client without a slot. Returns, in query order,
     * [{ status, row, offset, length, curPos, removed, text? }]: Length -> length (getLength(refSeq, client));
     * Locate -> row / offset / length (getContainingSegment), curPos (getPosition), removed; Text -> text
     * (MergeTreeTextHelper.getText(refSeq, client, "", pos1, pos2)).
     */
    views(queries) {
        this._idle();
        const qb = Buffer.alloc(queries.length * 24);
        queries.forEach((q, i) => {
            qb.writeUInt32LE(q.doc >>> 0, i * 24);
            qb.writeInt32LE(q.refSeq | 0, i * 24 + 4);
            qb.writeUInt32LE((q.client === undefined ? 0 : q.client) >>> 0, i * 24 + 8);
            qb.writeUInt32LE(q.kind >>> 0, i * 24 + 12);
            qb.writeUInt32LE((q.pos1 || 0) >>> 0, i * 24 + 16);
            qb.writeUInt32LE((q.pos2 === undefined ? 0xFFFFFFFF : q.pos2) >>> 0, i * 24 + 20);
        });
        const [rb, tb] = addon.views(this._engine, qb);
        return queries.map((q, i) => {
            const o = i * 32;
            const r = { status: rb.readInt32LE(o), row: rb.readUInt32LE(o + 4), offset: rb.readUInt32LE(o + 8),
                length: rb.readUInt32LE(o + 12), curPos: rb.readUInt32LE(o + 16),
                removed: (rb.readUInt32LE(o + 20) & VIEW_F_REMOVED) !== 0 };
            if (q.kind === ViewKind.Text && r.status === ViewStatus.Ok) {
                const at = Number(rb.readBigUInt64LE(o + 24));
                r.text = tb.toString("utf16le", at * 2, (at + r.length) * 2);
            }
            return r;
        });
    }
    /**
     * mte_markers: findTile and getTextAndMarkers in the observer's current view, answered on the GPU from the
     * last replay's rows and their property maps. queries: [{ doc, kind, pos1, pos2, label }] -- label a string.
     * Returns, in query order, [{ status, row?, pos?, removed?, pieces? }]: TileBefore / TileAfter -> row / pos
     * (Client.findTile; status NotFound for its undefined, Unsupported when an annotate of the document's log sets
     * referenceTileLabels); Paragraphs -> pieces, [{ row, pos, text }], one per tile of [pos1, pos2).
     */
    markers(queries) {
        this._idle();
        const labels = [], slot = new Map();
        const qb = Buffer.alloc(queries.length * 20);
        queries.forEach((q, i) => {
            if (!slot.has(q.label)) { slot.set(q.label, labels.length); labels.push(String(q.label)); }
            [q.doc, q.kind, q.pos1 || 0, q.pos2 === undefined ? 0xFFFFFFFF : q.pos2, slot.get(q.label)].forEach((v, k) => {
                qb.writeUInt32LE(v >>> 0, i * 20 + 4 * k);
            });
        });
        const [rb, pb, tb] = addon.markers(this._engine, qb, labels);
        return queries.map((q, i) => {
            const o = i * 32;
            const r = { status: rb.readInt32LE(o) };
            if (r.status !== MarkerStatus.Ok) return r;
            if (q.kind !== MarkerQuery.Paragraphs) {
                r.row = rb.readUInt32LE(o + 4);
                r.pos = rb.readUInt32LE(o + 8);
                r.removed = (rb.readUInt32LE(o + 12) & 1) !== 0;
                return r;
            }
            const n = rb.readUInt32LE(o + 16), first = Number(rb.readBigUInt64LE(o + 24));
            r.pieces = [];
            for (let k = first; k < first + n; k++) {
                const at = Number(pb.readBigUInt64LE(k * 24 + 8)), len = pb.readUInt32LE(k * 24 + 16);
                r.pieces.push({ row: pb.readUInt32LE(k * 24), pos: pb.readUInt32LE(k * 24 + 4),
                    text: tb.toString("utf16le", at * 2, (at + len) * 2) });
            }
            return r;
        });
    }
    /** mte_client_slot: the short id of a long client id in a document, VIEW_NO_CLIENT when it has none */
    clientSlot(doc, name) { this._idle(); return addon.clientSlot(this._engine, doc, name); }
    /** mte_view_props: the property object of row `row` (a Locate result's) of a document, or null */
    viewProps(doc, row) { this._idle(); return JSON.parse(addon.viewProps(this._engine, doc, row)); }
    /** The ITree SnapshotV1.emit(serializer) returns: { entries: [...], id: null } */
    snapshotV1(doc) { this._idle(); return JSON.parse(addon.snapshotV1(this._engine, doc)); }
    /** SharedMatrix summary of a { matrix } document pair (its rows and cols PermutationVectors) */
    snapshotMatrix(rowsDoc, colsDoc) { this._idle(); return JSON.parse(addon.snapshotMatrix(this._engine, rowsDoc, colsDoc)); }
    /**
     * mte_matrix_cells: IMatrixReader reads (matrix.ts:147-171) of replayed { matrix } document pairs, answered
     * on the GPU without the summary blob. queries: [{ rowsDoc, colsDoc, kind, row, col, nRows, nCols }].
     * Returns, in query order, [{ status, rowCount, colCount, value?, rowHandle?, colHandle?, values? }]: Shape ->
     * the counts alone; Cell -> value (getCell: the parsed JSON, undefined for no cell), rowHandle / colHandle
     * (0 = unallocated); Rect -> values, the nRows x nCols getCells from (row, col) on as an array of rows (all
     * undefined when status is OutOfRange).
     */
    matrixCells(queries) {
        this._idle();
        const qb = Buffer.alloc(queries.length * 32);
        queries.forEach((q, i) => {
            [q.rowsDoc, q.colsDoc, q.kind, q.row, q.col, q.nRows, q.nCols, 0].forEach((v, k) => {
                qb.writeUInt32LE((v || 0) >>> 0, i * 32 + 4 * k);
            });
        });
        const [rb, vb] = addon.matrixCells(this._engine, qb);
        const texts = new Map();
        const value = (id) => {
            if (id === CELL_NONE) return undefined;
            if (!texts.has(id)) texts.set(id, JSON.parse(addon.valueText(this._engine, id)));
            return texts.get(id);
        };
        return queries.map((q, i) => {
            const o = i * 32;
            const r = { status: rb.readInt32LE(o), rowCount: rb.readUInt32LE(o + 4), colCount: rb.readUInt32LE(o + 8) };
            if (q.kind === MatrixQuery.Cell && r.status === MatrixStatus.Ok) {
                r.value = value(rb.readUInt32LE(o + 12));
                r.rowHandle = rb.readUInt32LE(o + 16);
                r.colHandle = rb.readUInt32LE(o + 20);
            } else if (q.kind === MatrixQuery.Rect && (r.status === MatrixStatus.Ok || r.status === MatrixStatus.OutOfRange)) {
                const at = Number(rb.readBigUInt64LE(o + 24));
                const nr = q.nRows || 0, nc = q.nCols || 0;
                r.values = [];
                for (let a = 0; a < nr; a++) {
                    const row = [];
                    for (let b = 0; b < nc; b++) row.push(value(vb.readUInt32LE((at + a * nc + b) * 4)));
                    r.values.push(row);
                }
            }
            return r;
        });
    }
    /** mte_value_text: the canonical JSON text of a value id of the loaded batch */
    valueText(id) { this._idle(); return addon.valueText(this._engine, id); }
    /** SnapshotLegacy ITree (snapshotlegacy.ts:103-182): header, body, catch-up messages */
    snapshotLegacy(doc, catchUpBlobName = "catchupOps") {
        this._idle();
        return JSON.parse(addon.snapshotLegacy(this._engine, doc, catchUpBlobName));
    }
    /** 32-byte records {checksum u64, ops, length, segments, snapshotBytes, status, docId} */
    summaries() {
        this._idle();
        return parseSummaries(addon.summaries(this._engine, this._docs));
    }
    /**
     * Multi-GPU (one process per GPU, documents sharded by id): every rank's summaries in rank order,
     * all-gathered over RCCL (mte_gather_summaries). A collective: every rank calls it after its replay.
     * comm: rcclCommCreate(...) of this engine; null when world is 1.
     */
    gatherSummaries(rank, world, comm = null) {
        this._idle();
        return parseSummaries(addon.gatherSummaries(this._engine, rank, world, comm));
    }
    /** This rank's RCCL communicator on the engine's device, from the id rank 0 made (rcclUniqueId()). */
    rcclCommCreate(id, rank, world) { this._idle(); return addon.rcclCommCreate(this._engine, id, rank, world); }
}

function parseSummaries(buf) {
    const out = [];
    for (let o = 0; o + 32 <= buf.length; o += 32) {
        out.push({
            checksum: buf.readBigUInt64LE ? buf.readBigUInt64LE(o) : buf.toString("hex", o, o + 8),
            ops: buf.readUInt32LE(o + 8), length: buf.readUInt32LE(o + 12), segments: buf.readUInt32LE(o + 16),
            snapshotBytes: buf.readUInt32LE(o + 20), status: buf.readInt32LE(o + 24), docId: buf.readUInt32LE(o + 28),
        });
    }
    return out;
}

/**
 * Client-shaped facade for one document (client.ts:42): applyMsg, getText, getLength, snapshot.
 *
 * Incremental like Client.applyMsg (client.ts:805-836): applyMsg stages a message; the next read
 * parses the staged messages onto the document's open log (builderAppendMessages) and replays on the
 * GPU only the ops since the previous read, continuing the document's state from that pass (the
 * engine's retain mode, mte_retain). Reads without new messages reuse the last results. A document
 * the row engines cannot hold (loaded from a summary, relative positions, 64+ clients, ...) is
 * continued by the block engine from a block checkpoint. After load(summary) each read stages the
 * summary and the whole suffix again (host work linear in the log); the engine's prefix check finds
 * the log an extension of the last read's, so the GPU still replays only the new messages. Still
 * replayed from its first op at each read: a document over the engine's "ck_blk_budget_mb" option, a
 * client with newMergeTreeSnapshotFormat false whose log has catch-up messages (the legacy snapshot's
 * delta records), and a document after k_solo's LDS fallback or a host re-run.
 */
class MergeTreeClient {
    constructor(observer = "__observer__", options = {}) {
        this.observer = observer;
        this.options = options;
        this.pending = [];
        this.summary = undefined;
        this.messages = [];       // (summary mode only: the suffix replayed with it)
        this._builder = addon.createBuilder();
        this._doc = addon.builderOpenDoc(this._builder, observer);
        this._engine = undefined;
        this._version = 0;        // bumped by every staged change
        this._replayed = -1;      // the version the engine's results belong to
        this._flushing = null;    // pending flush() promise
        this.replays = 0;
    }
    get _dirty() { return this._version !== this._replayed; }
    /** Client.load / SnapshotLoader (client.ts:944-952): resume from a summary ITree before applyMsg. */
    load(summary) { this.summary = summary; this.messages = []; this.pending = []; this._version++; }
    applyMsg(msg) { this.pending.push(msg); this._version++; }
    /** Stage a batch of sequenced messages at once (one replay serves them all). */
    applyMsgs(msgs) { for (const m of msgs) this.pending.push(m); this._version++; }
    _check(version) {
        const [code, seq] = this._engine.docStatus(0);
        if (code === DocStatus.InsertFailed) throw new Error(`MergeTree insert failed at seq ${seq}`);
        if (code !== DocStatus.Ok) throw new Error(`replay failed (status ${code}) at seq ${seq}`);
        this._replayed = version;  // messages staged during an async flush keep the client dirty
        this.replays++;
    }
    _stage() {
        if (!this._engine) {
            this._engine = new BatchedMergeEngine(this.options);
            addon.retain(this._engine._engine, true);
        }
        if (this.summary !== undefined) {  // SnapshotLoader + suffix, staged whole per read (the replay continues)
            for (const m of this.pending) this.messages.push(m);
            this.pending = [];
            this._engine.load([{ observer: this.observer, messages: this.messages.slice(), summary: this.summary }]);
        } else {
            if (this.pending.length) {
                addon.builderAppendMessages(this._builder, this._doc, JSON.stringify(this.pending));
                this.pending = [];
            }
            this._engine._loadBuilder(this._builder);
        }
        return this._version;
    }
    _run() {
        if (this._flushing) throw new Error("MergeTreeClient: a flush() is still running; await it first");
        if (this._dirty) {
            const v = this._stage();
            this._engine.replay();
            this._check(v);
        }
        return this._engine;
    }
    /** Replay the staged messages off the event loop; resolves when outputs can be read. Reads while
     *  it is pending throw (the engine is not re-entrant); a second flush() waits for the first. */
    async flush() {
        while (this._flushing) await this._flushing.catch(() => {});
        if (!this._dirty) return;
        const v = this._stage();
        this._flushing = this._engine.replayAsync();
        try {
            await this._flushing;
        } finally {
            this._flushing = null;
        }
        this._check(v);
    }
    /** op records the last read continued past instead of replaying again */
    resumedOps() { this._run(); return this._engine.resumedOps(); }
    /** The whole text, or with start / end the range [start, end) of the current view
     *  (MergeTreeTextHelper.getText, textSegment.ts:154-186), read on the GPU. */
    getText(start, end) {
        const e = this._run();
        if (start === undefined && end === undefined) return e.getText(0);
        const s = start || 0;
        return e.views([{ doc: 0, refSeq: 0, client: 0, kind: ViewKind.Text, pos1: s,
            pos2: end === undefined ? 0xFFFFFFFF : Math.max(end, s) }])[0].text;
    }
    _locate(pos) { return this._run().views([{ doc: 0, refSeq: 0, client: 0, kind: ViewKind.Locate, pos1: pos }])[0]; }
    /** Client.getContainingSegment (client.ts:1022-1031): { segment: row of the segment table, offset },
     *  both undefined past the end. */
    getContainingSegment(pos) {
        const r = this._locate(pos);
        return r.status === ViewStatus.Ok ? { segment: r.row, offset: r.offset } : { segment: undefined, offset: undefined };
    }
    /** Client.getPropertiesAtPosition (client.ts:1012-1020): the segment's properties, or undefined. */
    getPropertiesAtPosition(pos) {
        const r = this._locate(pos);
        if (r.status !== ViewStatus.Ok) return undefined;
        const p = this._engine.viewProps(0, r.row);
        return p === null ? undefined : p;
    }
    /** Client.findTile (client.ts:1081-1084) in the current view, read on the GPU: { pos, row } -- row indexes
     *  the segment table -- or undefined. */
    findTile(pos, label, preceding = true) {
        const r = this._run().markers([{ doc: 0, kind: preceding ? MarkerQuery.TileBefore : MarkerQuery.TileAfter, pos1: pos, label }])[0];
        if (r.status === MarkerStatus.NotFound) return undefined;
        if (r.status !== MarkerStatus.Ok) throw new Error(`findTile: marker status ${r.status}`);
        return { pos: r.pos, row: r.row };
    }
    /** SharedString.getTextAndMarkers (sharedString.ts:207-210), read on the GPU: { parallelText,
     *  parallelMarkers }, each marker { pos, row, properties }. */
    getTextAndMarkers(label) {
        const e = this._run();
        const r = e.markers([{ doc: 0, kind: MarkerQuery.Paragraphs, label }])[0];
        if (r.status !== MarkerStatus.Ok) throw new Error(`getTextAndMarkers: marker status ${r.status}`);
        return { parallelText: r.pieces.map((p) => p.text),
            parallelMarkers: r.pieces.map((p) => ({ pos: p.pos, row: p.row, properties: e.viewProps(0, p.row) })) };
    }
    /** Client.getPosition (client.ts:295-300) of segment table row `row`: the start of the first visible
     *  row at or after it (found by locating positions: O(log length) queries). */
    getPosition(row) {
        const e = this._run();
        let lo = 0, hi = e.views([{ doc: 0, refSeq: 0, client: 0, kind: ViewKind.Length }])[0].length;
        while (lo < hi) {
            const mid = (lo + hi) >>> 1;
            const r = e.views([{ doc: 0, refSeq: 0, client: 0, kind: ViewKind.Locate, pos1: mid }])[0];
            if (r.row >= row) hi = mid; else lo = mid + 1;
        }
        return lo;
    }
    /** MergeTree.getLength(refSeq, clientId) (mergeTree.ts:1577-1584) for a long client id. */
    getLengthAt(refSeq, clientId) {
        const e = this._run();
        const r = e.views([{ doc: 0, refSeq, client: e.clientSlot(0, clientId), kind: ViewKind.Length }])[0];
        if (r.status !== ViewStatus.Ok) throw new Error(`getLengthAt: view status ${r.status}`);
        return r.length;
    }
    /** Client.getLength (client.ts:1057): markers count 1, unlike getText().length. */
    getLength() { return this._run().getLength(0); }
    /** Client.snapshot (client.ts:907-942): SnapshotV1, or SnapshotLegacy with its catch-up messages
     *  when the options say newMergeTreeSnapshotFormat: false. */
    snapshot() {
        const e = this._run();
        return e.legacyFormat ? e.snapshotLegacy(0, this.options.catchUpBlobName) : e.snapshotV1(0);
    }
}

module.exports = {
    BatchedMergeEngine, MergeTreeClient, DocStatus, ViewKind, ViewStatus, VIEW_NO_CLIENT, VIEW_F_REMOVED,
    MatrixQuery, MatrixStatus, MarkerQuery, MarkerStatus,
    abiVersion: addon.abiVersion, buildInfo: addon.buildInfo,
    createBuilder: addon.createBuilder, builderAddDoc: addon.builderAddDoc, builderDocCount: addon.builderDocCount,
    builderOpenDoc: addon.builderOpenDoc, builderAppendMessages: addon.builderAppendMessages,
    builderAddDocFromSummary: addon.builderAddDocFromSummary, builderAddContainerLog: addon.builderAddContainerLog,
    builderAddMatrixLog: addon.builderAddMatrixLog,
    builderAddMatrixFromSummary: addon.builderAddMatrixFromSummary,
    /** rank 0: the RCCL id (Buffer) to send to every rank; rcclCommDestroy(comm) releases a communicator */
    rcclUniqueId: addon.rcclUniqueId, rcclCommDestroy: addon.rcclCommDestroy,
    /** low level: (engine handle, rank, world, comm) -> Buffer of 32-byte records */
    gatherSummariesRaw: addon.gatherSummaries, rcclCommCreateRaw: addon.rcclCommCreate,
};
