// GPU: the view queries through the addon. argv[2] names a JSON file { observer, logs: [messages[]],
// queries: [{ doc, refSeq, client (long id, "" = the observer, null = no client), kind, pos1, pos2 }],
// facade: messages[] }: the logs are replayed as one batch, every query answered in one views() call
// (long ids mapped by clientSlot), and the facade's positional reads run on `facade`. Prints one JSON
// line for the caller to compare (tests/test_napi_views.py).
"use strict";
const fs = require("fs");
const { BatchedMergeEngine, MergeTreeClient, VIEW_NO_CLIENT } = require("..");
const input = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const e = new BatchedMergeEngine({ newMergeTreeSnapshotFormat: true });
e.load(input.logs.map((messages) => ({ observer: input.observer, messages })));
e.replay();
const slot = (q) => (q.client === null ? VIEW_NO_CLIENT : q.client === "" ? 0 : e.clientSlot(q.doc, q.client));
const results = e.views(input.queries.map((q) => ({ doc: q.doc, refSeq: q.refSeq, client: slot(q), kind: q.kind,
    pos1: q.pos1, pos2: q.pos2 })));
const downloaded = e.getInfo("downloaded");
const rows = [0, 1].map((r) => e.viewProps(0, r));
const c = new MergeTreeClient(input.observer, { newMergeTreeSnapshotFormat: true });
for (const m of input.facade) c.applyMsg(m);
const n = c.getLength();
const facade = { props: [], segment: [], position: [c.getPosition(0), c.getPosition(1)], text: c.getText(6, 11),
    all: c.getText(), tail: c.getText(6), lengthAt: c.getLengthAt(1, "s1"), past: c.getContainingSegment(n) };
for (let p = 0; p <= n; p++) {
    const pr = c.getPropertiesAtPosition(p);
    facade.props.push(pr === undefined ? null : pr);
    const s = c.getContainingSegment(p);
    facade.segment.push(s.segment === undefined ? null : [s.segment, s.offset]);
}
console.log(JSON.stringify({ results, downloaded, rows, facade,
    noSlot: e.clientSlot(0, "nobody-by-this-name") === VIEW_NO_CLIENT }));
