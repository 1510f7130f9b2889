"""Pin the restatement of the sRGB -> raw unprocessing (tests/_unprocess_ref.py) to the reference's own outputs (tests/golden/unprocess.npz,
written by tests/golden/make_golden_unprocess.py): the float64 restatement lies inside the recorded E_abs / E_rel of every case, the float32
restatement inside the agreement rule (it equalled the reference on the generating host), and the restated gathers equal the golden ones."""
import json
import os

import numpy as np
import pytest

from tests import _unprocess_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ['a', 'b', 'c', 'd', 'e', 'quad', 'nan']


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'unprocess.npz')))


@pytest.fixture(scope='module')
def meta():
    return json.load(open(os.path.join(HERE, 'golden', 'unprocess.json')))['cases']


@pytest.mark.parametrize('tag', CASES)
def test_float64_restatement_inside_the_recorded_errors(gold, meta, tag):
    x, m, gains, ref = gold[tag + '_x'], gold[tag + '_m'], gold[tag + '_gains'], gold[tag + '_ref']
    for i in range(len(x)):                                      # the stored gains are the reference's float32 tensor ops on the stored draws
        assert np.array_equal(R.gains_f32(*gold[tag + '_g'][i]).view(np.uint32), gains[i].view(np.uint32))
    e_abs, e_rel = R.errors(ref, R.batch_f64(x, m, gains))
    assert e_abs <= meta[tag]['E_abs'] * (1 + 1e-9) and e_rel <= meta[tag]['E_rel'] * (1 + 1e-9), (e_abs, e_rel, meta[tag])
    mine = np.stack([R.unprocess_f32(x[i], m[i], gains[i]) for i in range(len(x))])
    R.assert_within(mine, R.batch_f64(x, m, gains), meta[tag]['E_abs'], meta[tag]['E_rel'], f'{tag} float32 restatement')


def test_seeded_cases_restated(gold, meta):
    for cam in ('IMX686', 'SonyA7S2'):
        for kind in ('3d', '4d'):
            key = f'f_{cam}_{kind}'
            x, ref = gold[key + '_x'], gold[key + '_ref']
            gains = R.gains_f32(gold[key + '_rgb_gain'], gold[key + '_red_gain'], gold[key + '_blue_gain'])
            flat = x.reshape((-1,) + x.shape[-3:])
            want = R.batch_f64(flat, R.CCMS[cam], gains).reshape(x.shape)
            e_abs, e_rel = R.errors(ref, want)
            assert e_abs <= meta[key]['E_abs'] * (1 + 1e-9) and e_rel <= meta[key]['E_rel'] * (1 + 1e-9), key
            assert np.allclose(gold[key + '_cam2rgb'] @ R.CCMS[cam], np.eye(3), atol=1e-6)


def test_highlight_case_spans_the_mask(gold, meta):
    lo, hi = meta['c']['gray']
    assert lo < 0.9 and hi >= 1.0
    assert (gold['c_x'] == 1.0).any() and (gold['c_x'] < 0.9).any()


def test_nan_goes_through_the_matrix(gold):
    bad = np.isnan(gold['nan_ref'])
    assert np.isnan(gold['nan_x']).sum() == 1 and bad.sum() == 3 and bad[0, 1, 5].all()


def test_restated_gathers_equal_the_golden_ones(gold):
    assert np.array_equal(R.mosaic(gold['g_x']), gold['g_rggb']) and np.array_equal(R.mosaic(gold['g_x'], gbrg=True), gold['g_gbrg'])
    assert gold['g_rggb'].shape == (2, 2, 3, 4, 4)
    idx = np.arange(4 * 6 * 3, dtype=np.float32).reshape(4, 6, 3)                # index maps: a tensor that holds its own flat index
    assert np.array_equal(R.mosaic(idx), gold['g_idx_rggb']) and np.array_equal(R.mosaic(idx, gbrg=True), gold['g_idx_gbrg'])
    assert gold['g_idx_rggb'][0, 0].tolist() == [0.0, 4.0, 23.0, 19.0]           # R (0,0), Gr (0,1), B (1,1), Gb (1,0)
    assert gold['g_idx_gbrg'][0, 0].tolist() == [18.0, 22.0, 1.0, 5.0]           # R (1,0), Gr (1,1), Gb (0,0), B (0,1)
    p = R.packed(gold['g_x'][0])
    assert p.shape == (2, 4, 3, 4) and np.array_equal(p[:, 2], gold['g_x'][0][:, 1::2, 1::2, 2])


def test_agreement_rule_refuses_what_it_must():
    want = np.array([0.5, 0.25, 1e-3])
    ulp = float(np.spacing(np.float32(0.5)))
    R.assert_within(want + np.array([ulp, 0, 0]), want, 0.0, 0.0)                # one ulp passes an exact case
    with pytest.raises(AssertionError):
        R.assert_within(want + np.array([3 * ulp, 0, 0]), want, 0.0, 0.0)
    R.assert_within(want + np.array([3.9e-7, 0, 0]), want, 1e-7, 1e-6)
    with pytest.raises(AssertionError):
        R.assert_within(want + np.array([4.1e-7, 0, 0]), want, 1e-7, 1e-6)       # beyond 4 x E_abs
    with pytest.raises(AssertionError):
        R.assert_within(want + np.array([0, 0, 1e-8]), want, 1e-7, 1e-6)         # inside E_abs, beyond 4 x E_rel of a small value
    with pytest.raises(AssertionError):
        R.assert_within(np.array([0.5, np.nan, 1e-3]), want, 1.0, 1.0)           # a NaN where float64 has none


def test_golden_files_are_small_and_described(meta):
    assert set(CASES) <= set(meta) and 'rt' in meta
    assert meta['a']['shape'] == [1, 64, 66, 3] and meta['b']['shape'] == [3, 34, 130, 3] and meta['quad']['shape'] == [1, 2, 2, 3]
    assert os.path.getsize(os.path.join(HERE, 'golden', 'unprocess.npz')) < 1 << 20
