"""TEST INFRASTRUCTURE: the generated documents of the round-13 tests (engine state in one register set,
DESIGN 3.12), shared by tests/test_reg_state_regs_cpu.py, tests/test_state_regs_native.py and
tests/test_gpu_state_regs.py: (kind, global id, ops, writers, seed). The CPU test asserts, from the
engine's event counters, which of the restated places each one reaches."""

# lean engine: three and more rows (more than 16 leaf blocks), resolves hitting in either row buffer, block
# splits whose new block starts the next row, a heap past 64 entries, packs with every kk and with a
# remainder, cascades into pack_internal
LEAN = (2, 1, 3000, 8, 17)
# PROPS + WIDE engine, properties and annotates
FULL = (3, 7, 2000, 8, 1000)
# 33 writers (the WIDE engine): a heap past 127 entries, pops on the serial sift
W33 = (2, 3, 1200, 33, 1000)
# 31 writers on the lean engine: the heap passes 127 entries and the serial sift runs there too, then room()
# refuses op 1255 and the document hands over between two ops
HANDOFF = (2, 0, 4000, 31, 17)
HANDOFF_AT = 1255
