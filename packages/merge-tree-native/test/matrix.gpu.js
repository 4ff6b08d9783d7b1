// GPU: the SharedMatrix reads through the addon. argv[2] names a JSON file { observer, matrices:
// [messages[]] }: the logs are replayed as one batch (each a rows and a cols document), then one
// matrixCells() call reads every matrix's shape, a second its full grid as one Rect and its corner cells as
// Cells. Prints one JSON line for the caller to compare (tests/test_napi_matrix_reads.py).
"use strict";
const fs = require("fs");
const { BatchedMergeEngine, MatrixQuery } = require("..");
const input = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const e = new BatchedMergeEngine({ newMergeTreeSnapshotFormat: true });
e.load(input.matrices.map((matrix) => ({ observer: input.observer, matrix })));
e.replay();
const pair = (i) => ({ rowsDoc: 2 * i, colsDoc: 2 * i + 1 });
const shapes = e.matrixCells(input.matrices.map((_, i) => ({ ...pair(i), kind: MatrixQuery.Shape })));
const q = [];
shapes.forEach((s, i) => {
    q.push({ ...pair(i), kind: MatrixQuery.Rect, row: 0, col: 0, nRows: s.rowCount, nCols: s.colCount });
    q.push({ ...pair(i), kind: MatrixQuery.Cell, row: 0, col: 0 });
    q.push({ ...pair(i), kind: MatrixQuery.Cell, row: s.rowCount - 1, col: s.colCount - 1 });
    q.push({ ...pair(i), kind: MatrixQuery.Cell, row: s.rowCount, col: 0 });
    q.push({ ...pair(i), kind: MatrixQuery.Rect, row: 1, col: 0, nRows: s.rowCount, nCols: 1 });
});
const r = e.matrixCells(q);
const nul = (v) => (v === undefined ? null : v);
const out = shapes.map((s, i) => ({
    rowCount: s.rowCount, colCount: s.colCount, status: r.slice(5 * i, 5 * i + 5).map((x) => x.status),
    grid: r[5 * i].values.map((row) => row.map(nul)), first: nul(r[5 * i + 1].value), last: nul(r[5 * i + 2].value),
    handles: [r[5 * i + 1].rowHandle, r[5 * i + 1].colHandle, r[5 * i + 2].rowHandle, r[5 * i + 2].colHandle],
    outside: r[5 * i + 4].values.map((row) => row.map(nul)),
}));
console.log(JSON.stringify({ matrices: out, downloaded: e.getInfo("downloaded"), built: e.getInfo("mx_tables_built"),
    nullText: e.valueText(0) }));
