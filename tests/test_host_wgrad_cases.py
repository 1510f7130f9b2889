"""What tests/test_gpu_wgrad_tiles.py covers, without a GPU: on 256 compute units its case table reaches all eight (scheme, output tile) instantiations of the 3x3
weight-gradient kernel (csrc/wgrad_s.h) and, for each of them, every class of pixel tiles per workgroup -- one, two, three, four or more, and an uneven share.  The
rules are the ones that file restates (dispatch, tile heights, pixel splits); if one of them or a shape changes, this tells that the table has stopped covering a
class before anyone runs it on a card."""
from test_gpu_wgrad_tiles import CASES, TH, _classes, _inst, _per_workgroup, _tile

INSTANCES = {'x3': {(2, 2, 2, 1), (2, 1, 3, 1), (1, 2, 2, 1), (1, 1, 4, 1)}, 'h2': {(2, 2, 2, 2), (2, 1, 3, 1), (1, 2, 3, 1), (1, 1, 4, 1)}}


def test_the_cases_reach_all_eight_instantiations_and_every_tiles_per_workgroup_class():
    got = {}
    for name, schemes, (B, H, W), (Co, C1, C2), inst, counts in CASES:
        assert set(inst) == set(schemes), name
        for s in schemes:
            assert _inst(s, Co, C1 + C2) == inst[s], (name, s)
            assert _per_workgroup(s, B, H, W, Co, C1 + C2, 256) == counts, (name, s)
            got.setdefault((s, inst[s]), set()).update(_classes(counts))
    assert set(got) == {(s, i) for s in INSTANCES for i in INSTANCES[s]}
    for key, classes in got.items():
        assert classes == {'1', '2', '3', '4+', 'uneven'}, (key, classes)


def test_the_cases_stay_small_and_include_a_two_tensor_input_and_a_ragged_map():
    """Maps of at most 64 x 128 pixels, 32 / 64 channels, one output tile (so a case has one slab per compute unit); a two-tensor input whose boundary lies inside
    the N tile and a ragged map (H no multiple of the tile height, W no multiple of 32) for each scheme."""
    two, ragged = set(), set()
    for name, schemes, (B, H, W), (Co, C1, C2), inst, counts in CASES:
        assert H <= 64 and W <= 128 and Co in (32, 64) and C1 + C2 in (32, 64) and C1 in (32, 64) and C2 in (0, 32), name
        for s in schemes:
            t = _tile(Co, C1 + C2)
            assert (Co // t[0]) * ((C1 + C2) // t[1]) == 1, name
            if C2 and C1 < t[1]:
                two.add(s)
            if H % TH[s][t] and W % 32:
                ragged.add(s)
    assert two == {'x3', 'h2'} and ragged == {'x3', 'h2'}
