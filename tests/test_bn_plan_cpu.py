"""Every shape tests/test_gpu_bn_edges.py names has the property it was chosen
for, read from the host's own work split (``bn_plan`` launches nothing, so it
answers without a GPU): a shape that drifted off its edge is found here."""
import pytest

from distributed_model_parallel_amd import _native
from tests import bn_edge_shapes as S


@pytest.fixture(scope="module")
def plan():
    C = _native.native()
    if C is None:
        pytest.skip("the native extension is not built")
    return C.bn_plan


def test_keys_and_their_relations(plan):
    g = plan(37, 24, S.BF16)
    assert set(g) == {"vec", "cv", "tc", "rpi", "idle", "cchunks", "last_chunk_lanes", "row_blocks",
                      "rows_per_block", "last_block_rows", "reduce_chunks", "zeroed", "streaming"}
    for m, c, dt in [(37, 24, S.BF16), (2049, 2048, S.BF16), (524296, 8, S.BF16), (300, 1028, S.F32)]:
        g = plan(m, c, dt)
        assert g["vec"] == (8 if dt == S.BF16 else 4) and g["cv"] * g["vec"] == c
        assert g["idle"] == 256 - g["tc"] * g["rpi"] and 0 <= g["idle"] < g["tc"]
        assert (g["cchunks"] - 1) * g["tc"] + g["last_chunk_lanes"] == g["cv"]
        assert (g["row_blocks"] - 1) * g["rows_per_block"] + g["last_block_rows"] == m
        assert 1 <= g["last_block_rows"] <= g["rows_per_block"]
        assert g["reduce_chunks"] == -(-g["row_blocks"] // 256)
        assert g["zeroed"] == (g["row_blocks"] > 256)


@pytest.mark.parametrize("c,dtype,expect", S.CHANNEL_SPLIT)
def test_channel_split_shapes(plan, c, dtype, expect):
    g = S.check_plan(plan, S.CHANNEL_M, c, dtype, **expect)
    assert g["zeroed"] == 0 and g["streaming"] == 0


@pytest.mark.parametrize("c,dtype,rpi,m_one_row", S.ROW_LOOPS)
def test_row_loop_shapes(plan, c, dtype, rpi, m_one_row):
    ms = S.row_loop_ms(rpi)
    for m in ms:
        g = S.check_plan(plan, m, c, dtype, rpi=rpi)
        assert g["cchunks"] == 1
    per_lane = lambda g: -(-g["rows_per_block"] // rpi)  # row passes of a block's first lanes
    # no pass, one (tail only), the 2-row loop alone and with the single-row tail, the 4-row loop
    # alone and with its tail, two blocks with a short last slab
    assert plan(1, c, dtype)["rows_per_block"] == 1
    assert {per_lane(plan(m, c, dtype)) for m in ms} >= {1, 2, 3, 4, 5}
    g = plan(8 * rpi + 1, c, dtype)
    assert g["row_blocks"] == 2 and g["last_block_rows"] < g["rows_per_block"]
    if rpi > 1:  # a slab with fewer rows than the block has lane rows
        assert plan(rpi - 1, c, dtype)["rows_per_block"] < rpi
    if m_one_row is not None:
        g = S.check_plan(plan, m_one_row, c, dtype, rpi=rpi, last_block_rows=1)
        assert g["row_blocks"] >= 2


@pytest.mark.parametrize("m,c,dtype,rb,chunks,cchunks", S.PARTIAL_REDUCE)
def test_partial_reduce_shapes(plan, m, c, dtype, rb, chunks, cchunks):
    S.check_plan(plan, m, c, dtype, row_blocks=rb, reduce_chunks=chunks, cchunks=cchunks, zeroed=int(rb > 256))


def test_streaming_shapes(plan):
    for dt in (S.BF16, S.F32):
        assert plan(*S.STREAMING, dt)["streaming"] == 1
        assert plan(*S.NOT_STREAMING, dt)["streaming"] == 0
    assert S.STREAMING[0] * S.STREAMING[1] == 2 ** 27


def test_real_dead_and_shard_shapes(plan):
    m, c, dt = S.REAL_SHAPES[0]
    assert plan(m, c, dt)["idle"] > 0 and plan(m, c, dt)["row_blocks"] == 1
    m, c, dt = S.REAL_SHAPES[1]
    assert plan(m, c, dt)["zeroed"] == 1
    m, c, dt = S.REAL_SHAPES[2]
    assert plan(m, c, dt)["cchunks"] == 2 and plan(m, c, dt)["row_blocks"] > 1
    assert 0 in S.SHARDS and 1 in S.SHARDS and len(set(S.SHARDS)) == len(S.SHARDS)
    for c, dt in S.SHARD_CASES:  # the full batch and the largest shard split their rows differently
        full, big = plan(sum(S.SHARDS), c, dt), plan(max(S.SHARDS), c, dt)
        assert full["rows_per_block"] != big["rows_per_block"] or full["row_blocks"] != big["row_blocks"]


def test_plan_refuses_what_the_kernels_refuse(plan):
    with pytest.raises(RuntimeError, match="multiple of 8"):
        plan(4, 12, S.BF16)
    with pytest.raises(RuntimeError, match="M >= 1"):
        plan(0, 8, S.BF16)
