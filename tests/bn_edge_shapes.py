"""The shapes tests/test_gpu_bn_edges.py places on the work-split edges of
csrc/bn/batchnorm.hip, each with the property it was chosen for as ``bn_plan``
keys.  tests/test_bn_plan_cpu.py checks the properties without a GPU; the GPU
file checks them again before it relies on them."""
import torch

BF16, F32 = torch.bfloat16, torch.float32

# Channel split at a small M: (C, dtype, expected bn_plan entries)
CHANNEL_M = 37
CHANNEL_SPLIT = [
    (8, BF16, dict(cv=1, tc=1, rpi=256, idle=0, cchunks=1)),
    (24, BF16, dict(tc=3, rpi=85, idle=1, cchunks=1)),
    (96, BF16, dict(tc=12, rpi=21, idle=4, cchunks=1)),
    (2048, BF16, dict(cv=256, tc=256, rpi=1, idle=0, cchunks=1, last_chunk_lanes=256)),
    (2056, BF16, dict(cv=257, rpi=1, cchunks=2, last_chunk_lanes=1)),
    (4104, BF16, dict(cv=513, rpi=1, cchunks=3, last_chunk_lanes=1)),
    (4, F32, dict(cv=1, tc=1, rpi=256, idle=0, cchunks=1)),
    (24, F32, dict(tc=6, rpi=42, idle=4, cchunks=1)),
    (1028, F32, dict(cv=257, rpi=1, cchunks=2, last_chunk_lanes=1)),
    (4096, F32, dict(cv=1024, rpi=1, cchunks=4, last_chunk_lanes=256)),
]

# Row loops: (C, dtype, rpi, M whose last row block holds one single row, or None).
# With rpi = 256 (C = 8) a block never gets fewer than 2041 rows once there are
# two blocks, and there are at most 1024 blocks, so no M leaves a one-row block;
# its shortest last slab is the 8*rpi+1 case of row_loop_ms.
ROW_LOOPS = [
    (8, BF16, 256, None),
    (96, BF16, 21, 28057),
    (2048, BF16, 1, 57),
    (24, F32, 42, 112561),
]


def row_loop_ms(rpi):
    """Row counts around the 4-rows-in-flight loop of the moments kernel and the
    2-row loop of the apply kernel, for a block that walks rpi rows per pass."""
    ms = [1, rpi - 1, rpi, rpi + 1, 2 * rpi, 2 * rpi + 1, 4 * rpi - 1, 4 * rpi, 4 * rpi + 1, 8 * rpi + 1]
    return sorted({m for m in ms if m > 0})


# Partial reduce: (M, C, dtype, row_blocks, reduce_chunks, cchunks).  More than
# 256 row blocks: the producer zeroes the sums and the reduce adds with atomics.
PARTIAL_REDUCE = [
    (2048, 2048, BF16, 256, 1, 1),    # the store path's last value
    (2049, 2048, BF16, 257, 2, 1),    # the first atomic value; the second chunk holds one row
    (4100, 2048, BF16, 513, 3, 1),    # the third chunk holds one row
    (16384, 2048, BF16, 1024, 4, 1),  # four full chunks
    (65544, 64, BF16, 257, 2, 1),
    (524296, 8, BF16, 257, 2, 1),
    (2056, 1024, F32, 257, 2, 1),
    (2056, 2056, BF16, 257, 2, 2),    # two reduce chunks and two channel chunks
]

# Non-temporal instantiations: M*C*2 >= 256 MiB, and the largest M that is not.
STREAMING = (131072, 1024)
NOT_STREAMING = (131071, 1024)

# Real-valued data and dead channels: one block with idle lanes, the atomic
# reduce, two channel chunks in fp32.
REAL_SHAPES = [(37, 96, BF16), (2049, 2048, BF16), (300, 1028, F32)]
DEAD_SHAPES = [(37, 96, BF16), (37, 24, F32)]

# The SyncBN contract: shard sizes of one batch, an empty and a one-row shard among them.
SHARDS = (5, 0, 1, 300, 31)
SHARD_CASES = [(96, BF16), (2056, BF16), (24, F32)]


def check_plan(plan, m, c, dtype, **expect):
    """Assert bn_plan(m, c, dtype) has the expected entries; returns the plan."""
    g = plan(m, c, dtype)
    got = {k: g[k] for k in expect}
    assert got == expect, f"bn_plan({m}, {c}, {dtype}) = {g}: expected {expect}"
    return g
