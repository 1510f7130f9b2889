"""What tests/test_gpu_conv_walk.py covers, without a GPU: on 256 compute units its case table reaches, on 32- and on 64-column tiles, one chunk of K, two and an odd
count of three or more, and one, two, three, four or more tiles per workgroup and an uneven share.  The width rule and the grid rule are the ones that file
restates; if one of them or a shape changes, this tells that the table has stopped covering a class before anyone runs it on a card."""
import math

from test_gpu_conv_walk import CASES, _columns, _per_workgroup


def _tile_classes(counts):
    c = {'1' if n == 1 else '2' if n == 2 else '3' if n == 3 else '4+' for n in counts}
    return c | ({'uneven'} if len(counts) > 1 else set())


def _chunk_class(chunks):
    return '1' if chunks == 1 else '2' if chunks == 2 else 'odd>=3' if chunks >= 3 and chunks % 2 else None


def test_the_table_states_what_the_rules_give():
    for (B, H, W, Ci, Co), columns, chunks, counts in CASES:
        assert _columns(B, H, W, Co) == columns, (B, H, W, Ci, Co)
        assert Ci / 16 == chunks and math.ceil(chunks) == (Ci + 15) // 16, (B, H, W, Ci, Co)
        assert _per_workgroup(B, H, W, Co) == counts, (B, H, W, Ci, Co)
        assert Ci % 8 == 0 and Co % 32 == 0                              # (what the launch entries accept: one segment, whole 32-column blocks)


def test_the_table_covers_every_class_for_both_widths():
    chunk_classes, tile_classes, half, ragged, two_column_tiles = {32: set(), 64: set()}, {32: set(), 64: set()}, set(), set(), set()
    for (B, H, W, Ci, Co), columns, chunks, counts in CASES:
        chunk_classes[columns].add(_chunk_class(math.ceil(chunks)))
        tile_classes[columns] |= _tile_classes(counts)
        if chunks < 1:
            half.add(columns)
        if H % 16 and W % 32:
            ragged.add(columns)
        if Co > columns:
            two_column_tiles.add(columns)
    for columns in (32, 64):
        assert chunk_classes[columns] == {'1', '2', 'odd>=3'}, (columns, chunk_classes[columns])
        assert tile_classes[columns] == {'1', '2', '3', '4+', 'uneven'}, (columns, tile_classes[columns])
    assert half == {32} and ragged == {32, 64} and two_column_tiles == {64}
