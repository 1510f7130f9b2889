"""Host half of the paired-data preprocess branch (Mix_Dataset / IMX686_Mix_Dataset / IMX686_SFRN_Raw_Dataset), no device needed:
* ``process.get_aug_param_torch`` against the reference's own outputs (tests/golden/mix.*), bit for bit, with the RNG states it leaves;
* ``process.sna_rows``: the K draws (active crops only, in crop order) and the active flags against the reference's preprocess loop;
* ``runfile.preprocess_branch``: which branch a `dst_train` section selects."""
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'mix.npz')), json.load(open(os.path.join(golden_dir, 'mix.json')))


def test_fixture_covers_what_it_must(G):
    _, meta = G
    for scheme in ('augv2', 'augv5'):
        mine = [c for c in meta['aug'] if scheme in c['command']]
        assert {c['randint4_nonzero'] for c in mine} == {False, True} and {c['b'] for c in mine} == {1, 6}
    assert any(c['renorm'] for c in meta['aug'] if 'augv5' in c['command'])
    assert any('augv' not in c['command'] and c['randint4_nonzero'] for c in meta['aug'])
    pre = meta['preprocess']
    assert {c['ori'] for c in pre} == {False, True} and {repr(c['clip']) for c in pre} == {'False', 'True', '2'}
    assert {c['black_lr'] for c in pre} == {False, True}
    assert any(any(c['active']) and not all(c['active']) for c in pre) and any(not any(c['active']) for c in pre)


def test_get_aug_param_torch_equals_the_reference(G):
    from pnnp_amd import process as P
    g, meta = G
    for c in meta['aug']:
        wb = torch.from_numpy(g[c['tag'] + '_wb'])
        np.random.seed(c['seed']); torch.manual_seed(c['seed'])
        out = P.get_aug_param_torch({'wb': wb.clone()}, b=c['b'], command=c['command'], camera_type=c['camera_type'])
        assert all(torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (c['b'],) for t in out), c['tag']
        assert np.array_equal(np.stack([t.numpy() for t in out]), g[c['tag'] + '_t']), c['tag']
        assert [int(v) for v in np.random.get_state()[1][:4]] == c['np_state'], c['tag']
        assert [int(v) for v in torch.get_rng_state()[:16]] == c['torch_state'], c['tag']
        np.random.seed(c['seed']); torch.manual_seed(c['seed'])
        out = P.get_aug_param_torch({'wb': wb.clone()}, b=c['b'], command=c['command'], numpy=True, camera_type=c['camera_type'])
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and list(a.shape) == c['numpy_shape'] for a in out), c['tag']
        assert np.array_equal(np.stack(out), g[c['tag'] + '_n']), c['tag']
        if 'augv' not in c['command'] or not c['randint4_nonzero']:
            assert not np.stack(out).any()                                     # no scheme, or the 1-in-4 "leave it" draw: gains stay zero


def _aug_of(case, g):
    from pnnp_amd import process as P
    wb = torch.from_numpy(g[case['tag'] + '_wb_in'])
    np.random.seed(case['seed']); torch.manual_seed(case['seed'])
    if case['sfrn']:
        return torch.zeros(6, 4), True, 6, False
    ar, ag, ab = P.get_aug_param_torch({'wb': wb}, b=6, command=case['command'], camera_type=case['camera_type'])
    return torch.stack((ar, ag, ab, ag), dim=1), case['black_lr'], case['crop_per_image'], True


RATIO = {'SonyA7S2': [100., 250., 300., 150., 200., 120.], 'IMX686': [1., 2., 4., 8., 16., 2.]}      # make_golden_mix.py
ISO = {'SonyA7S2': [800, 1600, 3200], 'IMX686': [100, 6400, 6400]}


def test_sna_rows_draws_K_like_the_reference(G):
    from pnnp_amd import process as P
    g, meta = G
    for c in meta['preprocess']:
        aug, black, per_image, add_dy = _aug_of(c, g)
        before = aug.clone()
        ratio = torch.tensor(RATIO[c['camera_type']])
        assert np.array_equal(g[c['tag'] + '_ratio'].reshape(-1), ratio.numpy())
        rows, K = P.sna_rows(aug, ratio, torch.tensor(ISO[c['camera_type']]), c['camera_type'], black, per_image, add_dy=add_dy, device='cpu')
        assert torch.equal(aug, before)                                       # the caller's gains are not modified
        rows = rows.numpy()
        assert rows.shape == (6, P.SNA_NPARAM) and rows.dtype == np.float32
        assert [bool(v) for v in rows[:, P.SNA_ACTIVE]] == c['active'], c['tag']
        assert [float(k) for k, a in zip(K, c['active']) if a] == c['K'], c['tag']          # the same numpy draws, exactly
        assert all(k == 0 for k, a in zip(K, c['active']) if not a)
        act = np.array(c['active'])
        assert np.array_equal(rows[act, P.SNA_K], np.array(c['K'], np.float32))
        assert [[int(r[P.SNA_WP]), int(r[P.SNA_BL])] for r in rows[act]] == c['wp_bl']
        assert np.array_equal(rows[:, P.SNA_RATIO], ratio.numpy())
        assert np.array_equal(rows[:, :4], before.numpy() + (1 if black else 0))
        assert (rows[:, P.SNA_BLACK_LR] == float(black)).all() and (rows[:, P.SNA_ADD_DY] == float(add_dy)).all()


def test_an_inactive_crop_consumes_no_draw():
    from pnnp_amd import process as P
    aug = torch.tensor([[0.2, 0.1, 0.0, 0.1], [0.0, 0.0, 0.0, 0.0], [0.0, 0.3, 0.0, 0.3]])
    ratio, iso = torch.tensor([100., 200., 300.]), [800, 1600, 3200]
    np.random.seed(4)
    _, K = P.sna_rows(aug, ratio, iso, 'SonyA7S2', False, 1, device='cpu')
    after_mixed = np.random.uniform()
    np.random.seed(4)
    u = [np.random.uniform(low=-0.01, high=+0.01) for _ in range(2)]
    assert after_mixed == np.random.uniform()                                 # two draws were taken, not three
    k800, k3200 = P.get_specific_noise_params('SonyA7S2', 800)['Kmax'], P.get_specific_noise_params('SonyA7S2', 3200)['Kmax']
    assert list(K) == [k800 * (1 + u[0]), 0.0, k3200 * (1 + u[1])]             # crop 2 takes the SECOND draw and its own ISO
    np.random.seed(4)
    _, K3 = P.sna_rows(aug + 1, ratio, iso, 'SonyA7S2', False, 1, device='cpu')
    np.random.seed(4)
    u3 = [np.random.uniform(low=-0.01, high=+0.01) for _ in range(3)]
    assert K3[1] == P.get_specific_noise_params('SonyA7S2', 1600)['Kmax'] * (1 + u3[1]) and K3[2] == k3200 * (1 + u3[2])
    # black_lr: the + 1 comes first, so an all-zero gain row is active
    np.random.seed(4)
    rows, _ = P.sna_rows(aug, ratio, iso, 'SonyA7S2', True, 1, device='cpu')
    assert rows[:, P.SNA_ACTIVE].tolist() == [1.0, 1.0, 1.0] and rows[1, :4].tolist() == [1.0, 1.0, 1.0, 1.0]
    # the ISO of crop i is iso[i // crop_per_image]
    np.random.seed(4)
    _, Kc = P.sna_rows(aug + 1, ratio, [800, 3200], 'SonyA7S2', False, 2, device='cpu')
    assert Kc[1] == k800 * (1 + u3[1]) and Kc[2] == k3200 * (1 + u3[2])


def test_rows_are_checked_before_the_upload():
    from pnnp_amd import process as P
    from pnnp_amd._lib import PnnpError
    one = np.ones((2, 4), np.float32)
    with pytest.raises(PnnpError):
        P.pack_sna_rows(one, [1.0, 0.0], 1023, 64, [2.0, 2.0], [True, True], device='cpu')            # K <= 0 on an active row
    with pytest.raises(PnnpError):
        P.pack_sna_rows(one, [1.0, 1.0], 1023, 64, [2.0, 0.0], [True, True], device='cpu')            # ratio <= 0 on an active row
    rows = P.pack_sna_rows(one, [1.0, 0.0], 1023, 64, [2.0, 0.0], [True, False], device='cpu')        # an inactive row carries no K
    assert rows[:, P.SNA_ACTIVE].tolist() == [1.0, 0.0]
    with pytest.raises(KeyError):
        P.sna_rows(torch.ones(1, 4), torch.tensor([2.0]), [123], 'IMX686', False, 1, device='cpu')    # uncalibrated ISO, like SNA_torch


def test_preprocess_branch():
    from pnnp_amd import runfile
    want = {'Mix_Dataset': 'mix', 'IMX686_Mix_Dataset': 'mix', 'IMX686_SFRN_Raw_Dataset': 'sfrn', 'NF_Syn_Dataset': 'proxy',
            'IMX686_NF_Syn_Dataset': 'proxy', 'Raw_Dataset': 'physics'}
    for name, branch in want.items():
        assert runfile.preprocess_branch({'dataset': name}) == branch, name
    here = os.path.dirname(os.path.abspath(__file__))
    for f, cmd, cpi in (('runfile_sony_pmn.yml', 'augv2', 2), ('runfile_imx686_pmn.yml', 'augv2', 3)):
        cfg = runfile.load(os.path.join(here, 'fixtures', f))
        assert runfile.preprocess_branch(cfg['dst_train']) == 'mix' and cmd in cfg['dst_train']['command']
        assert cfg['dst_train']['crop_per_image'] == cpi
    assert runfile.preprocess_branch(runfile.load(os.path.join(here, 'fixtures', 'runfile_sony.yml'))['dst_train']) == 'physics'
