// Type declarations for @fluidframework/merge-tree-native (see index.js).
import { ISequencedDocumentMessage, ITree } from "@fluidframework/protocol-definitions";

export declare const DocStatus: { Ok: 0; InsertFailed: 1; SequenceOrder: 2; Capacity: 3; Unsupported: 4 };

/** View queries (BatchedMergeEngine.views): what to read, and how each query ended. */
export declare const ViewKind: { Length: 0; Locate: 1; Text: 2 };
export declare const ViewStatus: { Ok: 0; PastEnd: 1; OutOfWindow: 2; DocFailed: 3; BadQuery: 4 };
/** `client` of a view for a client that owns no slot of the document (all its ops at or below minSeq). */
export declare const VIEW_NO_CLIENT: number;
export declare const VIEW_F_REMOVED: number;
/** One positional read in the view (refSeq, client) of a document. client: a short id (clientSlot), 0 or
 *  omitted = the observer (refSeq unused), VIEW_NO_CLIENT. pos2 (Text only) defaults to the view's end. */
export interface ViewQuery { doc: number; refSeq: number; client?: number; kind: 0 | 1 | 2; pos1?: number; pos2?: number; }
/** Length: length = MergeTree.getLength(refSeq, client). Locate: row (index in the segment table) / offset /
 *  length of getContainingSegment(pos1), curPos = Client.getPosition of that segment, removed = it is
 *  removed in the current view (the position then maps to curPos, else to curPos + offset); status PastEnd
 *  (length = the view's length) when pos1 is not inside the view. Text: text =
 *  MergeTreeTextHelper.getText(refSeq, client, "", pos1, pos2). status OutOfWindow: refSeq outside
 *  [minSeq, currentSeq]; DocFailed; BadQuery. */
export interface ViewResult { status: number; row: number; offset: number; length: number; curPos: number;
    removed: boolean; text?: string; }

/** SharedMatrix reads (BatchedMergeEngine.matrixCells): what to read, and how each query ended. */
export declare const MatrixQuery: { Shape: 0; Cell: 1; Rect: 2 };
export declare const MatrixStatus: { Ok: 0; OutOfRange: 1; DocFailed: 2; BadQuery: 3 };
/** One IMatrixReader read of the matrix whose rows / cols vectors are documents rowsDoc / colsDoc (a
 *  { matrix } entry of load()). Cell: getCell(row, col). Rect: the nRows x nCols getCells from (row, col). */
export interface MatrixCellQuery { rowsDoc: number; colsDoc: number; kind: 0 | 1 | 2; row?: number; col?: number;
    nRows?: number; nCols?: number; }
/** rowCount / colCount: every kind. Cell: value (undefined: no cell, or an unallocated row / col), rowHandle,
 *  colHandle (0 = unallocated); status OutOfRange past either count. Rect: values, an array of nRows rows;
 *  status OutOfRange (every value undefined) when the rectangle is not wholly inside the matrix. */
export interface MatrixCellResult { status: number; rowCount: number; colCount: number; value?: unknown;
    rowHandle?: number; colHandle?: number; values?: unknown[][]; }

export interface ReplayStats { docs: number; ops: number; messages: number; failedDocs: number; kernelMs: number; }
export interface DocSummary {
    checksum: bigint | string; ops: number; length: number; segments: number;
    snapshotBytes: number; status: number; docId: number;
}
/** summary: a SnapshotV1 ITree to resume from (SnapshotLoader); messages then are the catch-up suffix. */
export interface DocLog { observer?: string; messages?: ISequencedDocumentMessage[]; summary?: ITree | string;
    /** SharedMatrix messages: this entry loads as two documents, the rows then the cols vector; with
     *  `summary` (a SharedMatrix summary ITree, SharedMatrix.loadCore) they are the suffix after it */
    matrix?: ISequencedDocumentMessage[]; }

/** Marker queries (BatchedMergeEngine.markers): what to read, and how each query ended. */
export declare const MarkerQuery: { readonly TileBefore: 0; readonly TileAfter: 1; readonly Paragraphs: 2 };
export declare const MarkerStatus: { readonly Ok: 0; readonly NotFound: 1; readonly Unsupported: 2; readonly DocFailed: 3;
    readonly BadQuery: 4 };
export interface MarkerQueryRecord {
    doc: number;
    kind: number;
    pos1?: number;
    /** Paragraphs: the range's end; undefined = to the end */
    pos2?: number;
    label: string;
}
export interface MarkerPiece { row: number; pos: number; text: string }
export interface MarkerResult {
    status: number;
    /** TileBefore / TileAfter: the tile's row of the segment table, its position, and whether it is removed */
    row?: number;
    pos?: number;
    removed?: boolean;
    /** Paragraphs: one piece per tile of the range */
    pieces?: MarkerPiece[];
}

export declare class BatchedMergeEngine {
    constructor(options?: { device?: number; chunkSize?: number; newMergeTreeSnapshotFormat?: boolean });
    load(docs: DocLog[]): void;
    generate(kind: 2 | 3 | 5, nDocs: number, nOps: number, nClients?: number, seed?: number): void;
    replay(): ReplayStats;
    /** mte_replay on a worker thread (N-API async work); other calls on the engine throw meanwhile. */
    replayAsync(): Promise<ReplayStats>;
    docStatus(doc: number): [number, number];
    getText(doc: number): string;
    /** Client.getLength: the observer's visible length, markers counting 1. */
    getLength(doc: number): number;
    snapshotV1(doc: number): ITree;
    /** A { matrix } entry of load() adds two documents: its rows then its cols PermutationVector. */
    snapshotMatrix(rowsDoc: number, colsDoc: number): ITree;
    /** After a replay with newMergeTreeSnapshotFormat: false. */
    snapshotLegacy(doc: number, catchUpBlobName?: string): ITree;
    summaries(): DocSummary[];
    /** Multi-GPU collective: every rank's summaries in rank order, all-gathered over RCCL (mte_gather_summaries).
     *  comm: this engine's communicator (rcclCommCreate), or null when world is 1. */
    gatherSummaries(rank: number, world: number, comm?: RcclComm | null): DocSummary[];
    /** This rank's RCCL communicator on the engine's device, from rank 0's rcclUniqueId(). */
    rcclCommCreate(id: Buffer, rank: number, world: number): RcclComm;
    /** mte_retain: keep each document's state, so a load of logs extending the last pass's replays
     *  only their new ops (Client.applyMsg's incremental cost). */
    retain(on?: boolean): void;
    /** op records the last replay continued past instead of replaying (mte_get_info "resumed_ops") */
    resumedOps(): number;
    /** mte_get_info: routing and counters of the last pass ("resumed_docs", "rows", "solo", ...;
     *  "downloaded": 1 once a whole-batch read such as getText(doc) has copied the results to the host) */
    getInfo(key: string): number;
    /** mte_views: many positional reads, any document, any client's view, answered on the GPU from the last
     *  replay's rows in one call, without copying the batch's results to the host. results[i] answers queries[i]. */
    views(queries: ViewQuery[]): ViewResult[];
    /** mte_client_slot: the short id of a long client id in a document, VIEW_NO_CLIENT when it has none. */
    clientSlot(doc: number, clientId: string): number;
    /** mte_view_props: the properties of segment table row `row` of a document, or null. */
    viewProps(doc: number, row: number): Record<string, unknown> | null;
    /** mte_matrix_cells: rowCount / colCount, getCell and dense ranges of the replayed matrices, many matrices a
     *  call, answered on the GPU without the summary blob. results[i] answers queries[i]. */
    matrixCells(queries: MatrixCellQuery[]): MatrixCellResult[];
    /** mte_markers: findTile and getTextAndMarkers in the observer's current view, answered on the GPU from the
     *  last replay's rows and their property maps. */
    markers(queries: MarkerQueryRecord[]): MarkerResult[];
    /** mte_value_text: the canonical JSON text of a value id of the loaded batch. */
    valueText(id: number): string;
}

/** An RCCL communicator handle (released by rcclCommDestroy or when collected). */
export type RcclComm = { readonly __rcclComm: unique symbol };
/** Rank 0 makes the id (MTE_RCCL_ID_BYTES = 128 bytes) and sends it to every rank. */
export declare function rcclUniqueId(): Buffer;
export declare function rcclCommDestroy(comm: RcclComm): void;

/** Client-shaped facade (merge-tree client.ts:42) for one document, incremental like
 *  Client.applyMsg (client.ts:805-836): a read after new messages replays only them on the GPU,
 *  continuing the document's state from the previous read (see index.js). */
export declare class MergeTreeClient {
    constructor(observer?: string, options?: { device?: number; chunkSize?: number });
    load(summary: ITree | string): void;
    applyMsg(msg: ISequencedDocumentMessage): void;
    applyMsgs(msgs: ISequencedDocumentMessage[]): void;
    /** Replay the staged messages off the event loop. */
    flush(): Promise<void>;
    /** The whole text; with start / end, the range [start, end) of the current view. */
    getText(start?: number, end?: number): string;
    getLength(): number;
    /** Client.getContainingSegment: segment = the row of the segment table; both undefined past the end. */
    getContainingSegment(pos: number): { segment: number | undefined; offset: number | undefined };
    /** Client.findTile: { pos, row } -- row indexes the segment table -- or undefined */
    findTile(pos: number, label: string, preceding?: boolean): { pos: number; row: number } | undefined;
    /** SharedString.getTextAndMarkers */
    getTextAndMarkers(label: string): { parallelText: string[];
        parallelMarkers: { pos: number; row: number; properties: Record<string, unknown> | null }[] };
    /** Client.getPropertiesAtPosition */
    getPropertiesAtPosition(pos: number): Record<string, unknown> | undefined;
    /** Client.getPosition of segment table row `row` */
    getPosition(row: number): number;
    /** MergeTree.getLength(refSeq, clientId), clientId the long id */
    getLengthAt(refSeq: number, clientId: string): number;
    snapshot(): ITree;
    /** op records the last read did not replay again */
    resumedOps(): number;
    /** GPU passes run so far (one per read after new messages) */
    readonly replays: number;
}

export declare function abiVersion(): number;
export declare function buildInfo(): string;

/** Low-level builder (the addon's own surface): container logs split per SharedString channel. */
export declare function createBuilder(): unknown;
/** An open document (its log grows by builderAppendMessages); returns its index in the batch. */
export declare function builderOpenDoc(builder: unknown, observer: string): number;
export declare function builderAppendMessages(builder: unknown, doc: number, messagesJson: string): void;
export declare function builderAddContainerLog(builder: unknown, observer: string, containerMessagesJson: string): string[];
