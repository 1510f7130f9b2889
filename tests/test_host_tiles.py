"""The tile geometry of pnnp_amd/tiles.py (TileGrid) against index maps recorded from the real reference
(tests/golden/make_golden_tiles.py: SynBase_Dataset.eval_crop / eval_merge on arange frames).  No GPU."""
import json
import os

import numpy as np
import pytest

from pnnp_amd._lib import PnnpError
from pnnp_amd.tiles import TileGrid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
META = json.load(open(os.path.join(GOLDEN, 'tiles.json')))['cases']
RUN = [m for m in META if not m['raises']]


@pytest.fixture(scope='module')
def maps():
    return np.load(os.path.join(GOLDEN, 'tiles.npz'))


def test_golden_covers_the_cases_of_the_issue():
    got = {(m['h'], m['w'], m['P'], m['base'], m['c'], m['raises']) for m in META}
    assert got == {(80, 150, 48, 16, 4, False), (64, 96, 48, 16, 4, False), (32, 32, 48, 16, 4, False), (33, 47, 48, 16, 4, False),
                   (40, 200, 64, 32, 4, False), (33, 47, 48, 16, 8, False), (31, 40, 48, 16, 4, True)}


@pytest.mark.parametrize('m', RUN, ids=[m['tag'] for m in RUN])
def test_crop_and_merge_index_equal_the_reference(m, maps):
    g = TileGrid(m['h'], m['w'], m['P'], m['base'])
    c, h, w, P = m['c'], m['h'], m['w'], m['P']
    assert (g.nh, g.nw, g.T) == (m['nh'], m['nw'], m['nh'] * m['nw'])
    ci = g.crop_index()
    assert ci.shape == (g.T, P, P)
    want = maps[m['tag'] + '_crop']                                    # [T, c, P, P]: index into the frame's c*h*w elements
    assert np.array_equal(ci[:, None] + (np.arange(c) * h * w)[None, :, None, None], want)
    mi = g.merge_index()
    assert mi.shape == (h, w)
    want = maps[m['tag'] + '_merge']                                   # [1, c, h, w]: index into the batch's T*c*P*P elements
    t, rc = mi // (P * P), mi % (P * P)
    assert np.array_equal((t[None] * c + np.arange(c)[:, None, None]) * P * P + rc[None], want[0])
    # the split is lossless: the tile element a frame pixel takes was read from that pixel
    assert np.array_equal(ci.reshape(-1)[mi], np.arange(h * w).reshape(h, w))


@pytest.mark.parametrize('m', RUN, ids=[m['tag'] for m in RUN])
def test_owner_rule_is_a_partition_over_any_chunking(m):
    g = TileGrid(m['h'], m['w'], m['P'], m['base'])
    for tb in (None, 1, 2, 4, 7, g.T):
        chunks = g.chunks(tb)
        assert [t0 for t0, _ in chunks] == list(range(0, g.T, g.T if tb is None else tb)) and sum(nt for _, nt in chunks) == g.T
        count = np.zeros((g.h, g.w), np.int64)
        for t0, nt in chunks:
            count += g.owned(t0, nt)
        assert (count == 1).all()
    # every owned pixel lies in its owner's interior [d, d + l)
    mi = g.merge_index() % (g.patch_size ** 2)
    r, c = mi // g.patch_size, mi % g.patch_size
    assert r.min() >= g.d and r.max() < g.d + g.l and c.min() >= g.d and c.max() < g.d + g.l


def test_refusals():
    bad = [m for m in META if m['raises']]
    assert len(bad) == 1 and (bad[0]['h'], bad[0]['w']) == (31, 40)
    with pytest.raises(PnnpError):                                     # h < l: the reference raises there (recorded)
        TileGrid(bad[0]['h'], bad[0]['w'], bad[0]['P'], bad[0]['base'])
    for args in [(40, 31, 48, 16),                                     # w < l
                 (32, 32, 48, 15), (32, 32, 48, 0), (32, 32, 48, -2), (32, 32, 48, 48), (32, 32, 48, 50),     # base odd, <= 0, >= patch_size
                 (8, 64, 24, 16), (64, 8, 24, 16)]:                    # d >= h, d >= w (l = 8 fits, the reflection by 8 does not)
        with pytest.raises(PnnpError):
            TileGrid(*args)
    TileGrid(9, 9, 24, 16)                                             # d = 8 < 9: legal
    with pytest.raises(PnnpError):                                     # the network paths need patch_size % 16 == 0
        TileGrid(80, 150, 40, 16, network=True)
    TileGrid(80, 150, 40, 16)
    TileGrid(80, 150, 48, 16, network=True)
    with pytest.raises(PnnpError):
        TileGrid(80, 150, 48, 16).chunks(0)


def test_public_functions_refuse_host_tensors():
    import torch
    from pnnp_amd import evaluate, tiles
    with pytest.raises(PnnpError):
        tiles.eval_crop(torch.zeros(1, 4, 80, 150), 48, 16)
    with pytest.raises(PnnpError):
        tiles.eval_merge(torch.zeros(15, 4, 48, 48), 80, 150, 16)
    with pytest.raises(PnnpError):
        evaluate.forward_tiled(None, torch.zeros(1, 4, 80, 150), 48, 16)
