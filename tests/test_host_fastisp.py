"""tests/_fastisp_ref.py, the restatement csrc/demosaic.hip is tested against, without a GPU: against the real FastISP's recorded outputs
(tests/golden/fastisp.npz: the mosaic its cvtColor received, its float64 result, the levels), against demosaic values written out by hand,
and against properties of the demosaic that do not depend on the restatement."""
import os

import numpy as np
import pytest

from tests import _fastisp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ['a', 'b', 'c', 'd', 'e', 'q']


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'fastisp.npz')))


@pytest.mark.parametrize('tag', CASES)
def test_restatement_equals_the_reference(gold, tag):
    x, wb, ccm = gold[tag + '_x'], gold.get(tag + '_wb'), gold.get(tag + '_ccm')
    assert (tag == 'b') == (wb is None)                                             # the defaults case stores neither
    mosaic = R.front(x, wb)
    assert mosaic.dtype == np.uint16 and np.array_equal(mosaic, gold[tag + '_mosaic'])
    out = R.fastisp(x, wb, ccm)
    assert out.dtype == np.float64 and np.array_equal(out.view(np.uint64), gold[tag + '_out'].view(np.uint64))
    assert np.array_equal(R.levels(out), gold[tag + '_u8'])
    s = 255 * gold[tag + '_out']                                                    # the levels can be compared exactly: no value next to a threshold
    assert not ((np.abs(s - np.rint(s)) < 1e-9) & (s != 0) & (s != 255)).any()


def test_front_nan_is_zero():
    x = np.full((4, 2, 2), 0.5, np.float32)
    x[1, 0, 1] = np.nan
    m = R.front(x, [2.0, 1, 1.0, 1])
    assert m[0, 3] == 0 and m[0, 0] == 16383 and m[1, 1] == 8191


# A 4 x 4 frame: the interior is 2 x 2 and everything else is border.
#   (1,1) B site: |50 - 70| = |20 - 40|, a tie, takes the horizontal pair: G = (50 + 70 + 1) >> 1 = 60 (vertical would give 30);
#                 R = (10 + 33 + 93 + 111 + 2) >> 2 = 249 >> 2 = 62
#   (1,2) G site, odd row: B = (61 + 81 + 1) >> 1 = 71 horizontally, R = (33 + 111 + 1) >> 1 = 72 vertically
#   (2,1) G site, even row: R = (93 + 111 + 1) >> 1 = 102 horizontally, B = (61 + 141 + 1) >> 1 = 101 vertically
#   (2,2) R site: |40 - 121| = 81 > |70 - 150| = 80, gradients one apart, takes the vertical pair: G = (70 + 150 + 1) >> 1 = 110
#                 (horizontal would give 81); B = (61 + 81 + 141 + 167 + 2) >> 2 = 452 >> 2 = 113
HAND4 = np.array([[10, 20, 33, 44],
                  [50, 61, 70, 81],
                  [93, 40, 111, 121],
                  [130, 141, 150, 167]], np.uint16)
P11, P12, P21, P22 = (62, 60, 61), (72, 70, 71), (102, 40, 101), (111, 110, 113)
WANT4 = np.array([[P11, P11, P12, P12],
                  [P11, P11, P12, P12],
                  [P21, P21, P22, P22],
                  [P21, P21, P22, P22]], np.uint16)

# A 6 x 6 frame.  By hand, interior rows y = 1..4, columns x = 1..4:
#   (1,1) B: |60 - 22| = 38 > |10 - 30| = 20: vertical, G = (10 + 30 + 1) >> 1 = 20;  R = (100 + 104 + 110 + 120 + 2) >> 2 = 109
#   (1,2) G: B = (200 + 204 + 1) >> 1 = 202;  R = (104 + 120 + 1) >> 1 = 112
#   (1,3) B: 3 vs 21: horizontal, G = (22 + 25 + 1) >> 1 = 24;  R = (104 + 108 + 120 + 131 + 2) >> 2 = 465 >> 2 = 116
#   (1,4) G: B = (204 + 208 + 1) >> 1 = 206;  R = (108 + 131 + 1) >> 1 = 120
#   (2,1) G: R = (110 + 120 + 1) >> 1 = 115;  B = (200 + 210 + 1) >> 1 = 205
#   (2,2) R: 3 vs 21: G = (30 + 33 + 1) >> 1 = 32;  B = (200 + 204 + 210 + 221 + 2) >> 2 = 837 >> 2 = 209
#   (2,3) G: R = (120 + 131 + 1) >> 1 = 126;  B = (204 + 221 + 1) >> 1 = 213
#   (2,4) R: 3 vs 22: G = (33 + 36 + 1) >> 1 = 35;  B = (204 + 208 + 221 + 230 + 2) >> 2 = 865 >> 2 = 216
#   (3,1) B: 3 vs 20: G = (40 + 43 + 1) >> 1 = 42;  R = (110 + 120 + 140 + 150 + 2) >> 2 = 522 >> 2 = 130
#   (3,2) G: B = (210 + 221 + 1) >> 1 = 216;  R = (120 + 150 + 1) >> 1 = 135
#   (3,3) B: |43 - 47| = 4, |33 - 38| = 5, one apart the other way: horizontal, G = (43 + 47 + 1) >> 1 = 45 (vertical would give 36);
#            R = (120 + 131 + 150 + 161 + 2) >> 2 = 141
#   (3,4) G: B = (221 + 230 + 1) >> 1 = 226;  R = (131 + 161 + 1) >> 1 = 146
#   (4,1) G: R = (140 + 150 + 1) >> 1 = 145;  B = (210 + 240 + 1) >> 1 = 225
#   (4,2) R: 12 vs 21: G = (50 + 38 + 1) >> 1 = 44;  B = (210 + 221 + 240 + 250 + 2) >> 2 = 923 >> 2 = 230
#   (4,3) G: R = (150 + 161 + 1) >> 1 = 156;  B = (221 + 250 + 1) >> 1 = 236
#   (4,4) R: 20 vs 21: G = (38 + 58 + 1) >> 1 = 48;  B = (221 + 230 + 250 + 65535 + 2) >> 2 = 66238 >> 2 = 16559 (a sum past 16 bits)
HAND6 = np.array([[100, 10, 104, 12, 108, 14],
                  [60, 200, 22, 204, 25, 208],
                  [110, 30, 120, 33, 131, 36],
                  [40, 210, 43, 221, 47, 230],
                  [140, 50, 150, 38, 161, 58],
                  [60, 240, 64, 250, 68, 65535]], np.uint16)
INNER6 = np.array([[(109, 20, 200), (112, 22, 202), (116, 24, 204), (120, 25, 206)],
                   [(115, 30, 205), (120, 32, 209), (126, 33, 213), (131, 35, 216)],
                   [(130, 42, 210), (135, 43, 216), (141, 45, 221), (146, 47, 226)],
                   [(145, 50, 225), (150, 44, 230), (156, 38, 236), (161, 48, 16559)]], np.uint16)
WANT6 = np.pad(INNER6, ((1, 1), (1, 1), (0, 0)), mode='edge')      # every border pixel copies the nearest interior pixel


def test_demosaic_hand_values():
    got = R.demosaic_ea(HAND4)
    assert got.dtype == np.uint16 and got.shape == (4, 4, 3) and np.array_equal(got, WANT4)
    assert np.array_equal(R.demosaic_ea(HAND6), WANT6)
    both = R.demosaic_ea(np.stack([HAND6, np.full_like(HAND6, 7)]))                # a batch is its frames
    assert both.shape == (2, 6, 6, 3) and np.array_equal(both[0], WANT6) and (both[1] == 7).all()


def _mosaic_of(fields):
    """three colour fields [H,W] -> the RGGB mosaic that samples them"""
    Rf, Gf, Bf = fields
    m = Gf.copy()
    m[0::2, 0::2] = Rf[0::2, 0::2]
    m[1::2, 1::2] = Bf[1::2, 1::2]
    return m.astype(np.uint16)


def test_demosaic_flat_colour_and_no_overflow():
    H, W = 8, 10
    a, b, c = 1000, 20000, 65535
    out = R.demosaic_ea(_mosaic_of([np.full((H, W), v, np.int64) for v in (a, b, c)]))
    assert (out == np.array([a, b, c], np.uint16)).all()
    assert (R.demosaic_ea(np.full((H, W), 65535, np.uint16)) == 65535).all()


def test_demosaic_reproduces_linear_ramps():
    H, W = 10, 12
    yy, xx = np.mgrid[0:H, 0:W]
    fields = [100 + 4 * yy + 6 * xx, 3000 + 10 * yy + 2 * xx, 500 + 2 * yy + 8 * xx]
    out = R.demosaic_ea(_mosaic_of(fields))
    for ch in range(3):
        assert np.array_equal(out[1:-1, 1:-1, ch], fields[ch][1:-1, 1:-1])


def test_demosaic_stripes_pick_the_pair_along_them():
    H, W = 8, 8
    v = np.array([5, 900, 70, 3000, 411, 20000, 1234, 40000], np.uint16)
    yy, xx = np.mgrid[1:H - 1, 1:W - 1]
    colour = ((yy ^ xx) & 1) == 0
    rows = np.repeat(v[:, None], W, axis=1)                                         # horizontal stripes: the value depends on the row
    g = R.demosaic_ea(rows)[1:-1, 1:-1, 1]
    assert np.array_equal(g[colour], rows[1:-1, 1:-1][colour])                      # the horizontal pair: this row's own value
    vertical_mean = ((rows[:-2, 1:-1].astype(np.int64) + rows[2:, 1:-1] + 1) >> 1)[colour]
    assert (vertical_mean != rows[1:-1, 1:-1][colour]).all()                        # ... which the vertical pair would not have given
    cols = rows.T.copy()                                                            # vertical stripes
    g = R.demosaic_ea(cols)[1:-1, 1:-1, 1]
    assert np.array_equal(g[colour], cols[1:-1, 1:-1][colour])
