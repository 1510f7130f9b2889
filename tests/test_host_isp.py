"""The packed-raw -> sRGB render without a device: the restatement (tests/_isp_ref.py) against the reference's own outputs
(tests/golden/isp.npz, written by tests/golden/make_golden_isp.py) under the agreement rule, the coverage of the boundary-dense case, and the
argument checks of the Python surface that raise before anything touches a device."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _isp_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'isp.npz')))


def case_input(gold, tag):
    x = gold[tag + '_x']
    return np.repeat(x, 4, axis=1) if tag == 'd' else x                  # case d stores plane R only: R = G1 = B = G2


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e'])
def test_restatement_against_the_reference(gold, tag):
    """float32 CPU restatement (exact on the generating host) and the round-once restatement, both under the agreement rule"""
    x, wb, ccm, k = case_input(gold, tag), gold[tag + '_wb'], gold[tag + '_ccm'], gold[tag + '_k']
    pre = R.process_pre(x, wb, ccm)
    R.assert_agrees(R.process_levels(x, wb, ccm), k, pre, f'{tag} float32')
    n = R.assert_agrees(R.process_levels(x, wb, ccm, once=True), k, pre, f'{tag} round-once')
    assert n <= R.CAP / 2 * k.size                                       # what the generator asserted before it wrote the file


def test_gamma_and_raw2rgb_v2_restatement(gold):
    R.assert_agrees(R.levels(gold['g_x']), gold['g_k'], R.pre(gold['g_x']), 'gamma float32')
    R.assert_agrees(R.levels_once(gold['g_x']), gold['g_k'], R.pre(gold['g_x']), 'gamma round-once')
    x = gold['v2_x'][None]
    got = R.process_levels(x, R.SONY_WB, R.SONY_CCM, once=True)[0].transpose(1, 2, 0)
    R.assert_agrees(got, gold['v2_k'], R.process_pre(x, R.SONY_WB, R.SONY_CCM)[0].transpose(1, 2, 0), 'raw2rgb_v2 round-once')


@pytest.mark.parametrize('tag,args,add', [('f_sid', ('f_sid_lr', 'f_sid_pred', 'f_sid_hr'), False), ('f_nf', ('f_nf_hr', 'f_nf_sample', 'f_nf_lr'), True)])
def test_preview_restatement(gold, tag, args, add):
    lin = R.preview_linear(*[gold[a] for a in args], gold['f_wb'], add_inputs_to_output=add)
    assert lin.shape == gold[tag + '_u8'].shape == (32, 120, 3)
    R.assert_agrees(R.levels_once(lin, floor=False), gold[tag + '_u8'], R.pre(lin, floor=False), tag)


def test_boundary_dense_case_straddles_every_threshold(gold):
    k = gold['d_k'].astype(np.int64)
    assert (k[:, 0] == k[:, 1]).all() and (k[:, 0] == k[:, 2]).all()     # identity matrix, equal planes
    per_level = k[:, 0].reshape(255, 64)                                 # row i: the 64 values around the threshold of level i + 1
    for i in range(255):
        assert (per_level[i] == i).any() and (per_level[i] == i + 1).any(), f'level {i + 1} is not straddled'
    near = np.abs(R.pre(gold['d_x']) - np.rint(R.pre(gold['d_x']))) <= R.PRE_TOL
    assert near.mean() > 0.5                                             # the case is dense in values the exception could apply to


def test_saturated_case_holds_both_row_sums(gold):
    lin = R.linear(gold['c_x'], gold['c_wb'], gold['c_ccm']).numpy()
    top = np.float32(1) - np.float32(2.0 ** -24)
    assert set(np.unique(lin[..., :32]).tolist()) <= {float(top), 1.0}   # all channels at 1: a row of the matrix sums to 1 or 1 - 2^-24
    assert (gold['c_k'][..., :32] == 255).all()                          # ... and both render as 255
    assert set(np.unique(gold['c_k'])) == {254, 255}
    assert R.levels(np.array([top, np.float32(1) - np.float32(2.0 ** -23)]))[1] == 254


def test_golden_files_are_small_and_described():
    meta = json.load(open(os.path.join(HERE, 'golden', 'isp.json')))
    assert [c['tag'] for c in meta['cases']] == ['a', 'b', 'c', 'd', 'e', 'f_sid', 'f_nf']
    assert all(c['shape'][-1] <= 120 and c['shape'][-2] <= 120 for c in meta['cases'])
    assert os.path.getsize(os.path.join(HERE, 'golden', 'isp.npz')) < 1 << 20


def test_agreement_rule_refuses_what_it_must():
    pre = np.array([100.00001, 100.4, 100.00001])
    assert R.disagreements([100, 100, 100], [100, 100, 100], pre) == (0, 0)
    assert R.disagreements([99, 100, 100], [100, 100, 100], pre) == (1, 0)           # one level, next to an integer: excused
    assert R.disagreements([100, 99, 100], [100, 100, 100], pre) == (1, 1)           # one level, mid-level: not excused
    assert R.disagreements([98, 100, 100], [100, 100, 100], pre) == (1, 1)           # two levels: never excused
    with pytest.raises(AssertionError):
        R.assert_agrees(np.full(100, 99), np.full(100, 100), np.full(100, 100.00001))   # all excusable, but far over the cap


def test_argument_checks_raise_without_a_device():
    from pnnp_amd import process as P
    from pnnp_amd._lib import PnnpError
    x = torch.zeros(1, 4, 4, 4)
    wb, ccm = torch.ones(1, 4), torch.eye(3)[None]
    with pytest.raises(PnnpError, match='unsupported'):
        P.process(x, wb, ccm, gamma=2.4)
    with pytest.raises(PnnpError, match='unsupported'):
        P.gamma_compression(torch.zeros(1, 3, 4, 4), gamma=1.0)
    with pytest.raises(PnnpError):
        P.process(x, wb, ccm)                                            # a host tensor: there is no CPU implementation
    with pytest.raises(PnnpError):
        P.process(torch.zeros(1, 3, 4, 4), wb, ccm)                      # not four planes
    with pytest.raises(PnnpError):
        P.gamma_compression(torch.zeros(1, 3, 4, 4))
    with pytest.raises(PnnpError):
        P.gamma_compression(torch.zeros(1, 4, 4, 4))
    for fn, a in ((P.apply_gains, (x, wb)), (P.apply_ccms, (torch.zeros(1, 3, 4, 4), ccm)), (P.raw2LRGB, (x,))):
        with pytest.raises(PnnpError):
            fn(*a)
    with pytest.raises(PnnpError):
        P.preview_strip(x[0], x[0], x[0], [2.13, 1, 1.57, 1])
    with pytest.raises(PnnpError):
        P.preview_strip(torch.zeros(3, 4, 4), x[0], x[0], [2.13, 1, 1.57, 1])
    with pytest.raises(PnnpError):
        P.isp_rows(torch.ones(3, 4), ccm, 2, device='cpu')               # neither one row nor one per image
    rows = P.isp_rows(np.array([2.0, 1.0, 1.5, 1.0]), np.arange(9.0).reshape(3, 3), 2, device='cpu')
    assert rows.shape == (2, P.ISP_NPARAM) and rows.dtype == torch.float32
    assert rows[1, :4].tolist() == [2.0, 1.0, 1.5, 1.0] and rows[1, 4:13].tolist() == list(range(9)) and rows[:, 13:].abs().sum() == 0
