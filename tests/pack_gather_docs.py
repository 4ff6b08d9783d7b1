"""TEST INFRASTRUCTURE: the hand-made documents of the fused-pack tests (tests/test_reg_pack_gather_cpu.py,
tests/test_pack_gather_native.py, tests/test_gpu_pack_gather.py), as message lists for mte.Builder."""
import random

from tests.oplog import ins, msg, rem

# The generated documents the GPU file replays on k_solo: (kind, ops, clients, global id, seed).
SOLO_DOCS = [(2, 3000, 8, 1, 17), (5, 2000, 8, 0, 1000), (3, 2000, 8, 7, 1000), (2, 1200, 33, 3, 1000)]


def tombstone_log():
    """One writer. Twelve two-letter inserts at the end with the MSN held at 0 (nothing settles: twelve
    segments, two leaf blocks after the 4+4 split, height 2), then the second segment of the first block is
    removed, then the MSN follows the sequence numbers: the first block (text, tombstone, text, text) is
    popped; its first scour drops the tombstone and joins slots 2 and 3, the block is left with 2 < 4
    children and packs, and the pack's own pass over it joins the text on the two sides of the dropped
    tombstone (pack_self_changed)."""
    msgs, seq = [], 0

    def put(contents, msn):
        nonlocal seq
        seq += 1
        msgs.append(msg("a", seq, seq - 1, contents, msn))

    for i in range(12):
        put(ins(2 * i, "%c%c" % (65 + i, 97 + i)), 0)
    put(rem(2, 4), 0)
    for i in range(12):
        put(ins(22 + i, "."), seq)
    return msgs


def long_insert_log(seed=0, n=1500):
    """Three writers, inserts of 1..600 characters and removes of up to 400 (the generator of
    tests/test_reg_pack_fused_cpu.py test_serial_walk_inside_a_pack): packs with a joining slot longer than
    GRANULARITY (256), which need scourNode's serial walk, beside packs without one."""
    from oracle import OracleDoc
    from tests.oplog import dumps

    rng = random.Random(300 + seed)
    d = OracleDoc()
    msgs, refs, seq, order = [], {c: 0 for c in "abc"}, 0, []
    for _ in range(n):
        c = rng.choice("abc")
        refs[c] = rng.randint(max(refs[c], seq - 6), seq)
        if c not in order:
            order.append(c)
        L = d.length_at(refs[c], order.index(c) + 1)
        if L == 0 or rng.random() < 0.5:
            k = rng.choice([1, 2, 5, 40, 250, 257, 300, 600])
            contents = ins(rng.randint(0, L), "".join(rng.choice("xyz") for _ in range(k)))
        else:
            a = rng.randint(0, L - 1)
            contents = rem(a, min(L, a + rng.randint(1, 400)))
        seq += 1
        m = msg(c, seq, refs[c], contents, min(refs.values()))
        msgs.append(m)
        d.apply_json(dumps([m]))
    return msgs
