// GPU: the marker queries through the addon. argv[2] names a JSON file { observer, logs: [messages[]],
// queries: [{ doc, kind, pos1, pos2, label }], facade: messages[], facadeLabel, facadeProbes: [pos] }: the
// logs are replayed as one batch, every query answered in one markers() call, and the facade's findTile /
// getTextAndMarkers run on `facade`. Prints one JSON line for the caller to compare
// (tests/test_napi_markers.py).
"use strict";
const fs = require("fs");
const { BatchedMergeEngine, MergeTreeClient } = require("..");
const input = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const e = new BatchedMergeEngine({ newMergeTreeSnapshotFormat: true });
e.load(input.logs.map((messages) => ({ observer: input.observer, messages })));
e.replay();
const results = e.markers(input.queries);
const downloaded = e.getInfo("downloaded");
const c = new MergeTreeClient(input.observer, { newMergeTreeSnapshotFormat: true });
for (const m of input.facade) c.applyMsg(m);
const tile = (t) => (t === undefined ? null : t);
const facade = { before: input.facadeProbes.map((p) => tile(c.findTile(p, input.facadeLabel))),
    after: input.facadeProbes.map((p) => tile(c.findTile(p, input.facadeLabel, false))),
    paragraphs: c.getTextAndMarkers(input.facadeLabel) };
console.log(JSON.stringify({ results, downloaded, facade }));
