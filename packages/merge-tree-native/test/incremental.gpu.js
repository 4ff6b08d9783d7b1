// GPU: a MergeTreeClient that starts from a summary (Client.load) reads incrementally. A first client
// edits a string (three writers, refSeq = seq - 1, minSeq 16 behind) and snapshots it after 400
// messages; a second one loads that SnapshotV1 tree and applies 600 more, reading every 100: each read
// equals the edited string, and every read after the first continued from the read before it
// (resumedOps() > 0: the block engine's checkpoint, mte_retain) instead of replaying from the summary.
"use strict";
const assert = require("assert");
const { MergeTreeClient } = require("..");
const msg = (c, s, r, contents, msn = 0) => ({ clientId: c, sequenceNumber: s, referenceSequenceNumber: r,
    minimumSequenceNumber: msn, type: "op", contents });
let text = "", rnd = 4242;
const rand = (n) => { rnd = (rnd * 1103515245 + 12345) & 0x7fffffff; return rnd % n; };
function next(seq) {
    let c;
    if (text.length > 0 && rand(10) < 4) {
        const a = rand(text.length), b = Math.min(text.length, a + 1 + rand(5));
        c = { pos1: a, pos2: b, type: 1 };
        text = text.slice(0, a) + text.slice(b);
    } else {
        const p = rand(text.length + 1), sg = "abcdef".slice(0, 1 + rand(6));
        c = { pos1: p, seg: sg, type: 0 };
        text = text.slice(0, p) + sg + text.slice(p);
    }
    return msg("w" + rand(3), seq, seq - 1, c, Math.max(0, seq - 16));
}
const first = new MergeTreeClient("obs", { newMergeTreeSnapshotFormat: true });
for (let seq = 1; seq <= 400; seq++) first.applyMsg(next(seq));
assert.strictEqual(first.getText(), text);
const tree = first.snapshot();
const c = new MergeTreeClient("obs", { newMergeTreeSnapshotFormat: true });
c.load(tree);
const resumed = [];
for (let seq = 401; seq <= 1000; seq++) {
    c.applyMsg(next(seq));
    if (seq % 100 === 0) {
        assert.strictEqual(c.getText(), text, `read at seq ${seq}`);
        assert.strictEqual(c.getLength(), text.length);
        resumed.push(c.resumedOps());
        if (resumed.length > 1) assert.ok(resumed[resumed.length - 1] > 0, `read at seq ${seq} replayed from the summary`);
    }
}
assert.strictEqual(c.replays, 6);
// each read skipped more than the one before: the prefix grows by 100 messages a read
for (let i = 2; i < resumed.length; i++) assert.ok(resumed[i] >= resumed[i - 1] + 100, JSON.stringify(resumed));
console.log(JSON.stringify({ reads: resumed.length, resumed, length: text.length }));
