"""The sRGB -> raw unprocessing without a device: the matrices, the host draws of ``unprocess`` and the RNG states they leave behind against
the reference's (tests/golden/unprocess.npz, case f), the parameter table with the reference's own float32 gains, the argument checks that
raise before anything touches a device, and the run-file branch that selects ``HipTrainStep.step_rgb``."""
import os

import numpy as np
import pytest
import torch

from tests import _unprocess_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, 'fixtures')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'unprocess.npz')))


def test_random_ccm_values():
    from pnnp_amd import unprocess as U
    for cam in ('IMX686', 'SonyA7S2'):
        m = U.random_ccm(cam)
        assert m.dtype == torch.float32 and m.shape == (3, 3) and np.array_equal(m.numpy(), R.CCMS[cam])
    assert np.array_equal(U.random_ccm().numpy(), R.CCMS['IMX686'])               # the reference's default camera
    assert np.allclose(U.random_ccm('IMX686').sum(dim=1).numpy(), 1.0, atol=1e-6)
    with pytest.raises(KeyError):
        U.random_ccm('Pixel')
    from pnnp_amd import augment
    assert U.random_gains is augment.random_gains


@pytest.mark.parametrize('cam', ['IMX686', 'SonyA7S2'])
def test_host_draws_and_rng_states_are_the_reference_s(gold, cam):
    from pnnp_amd import unprocess as U
    key = f'f_{cam}_3d'
    torch.manual_seed(11); np.random.seed(13)
    rgb2cam, cam2rgb, rgb_gain, red_gain, blue_gain = U.unprocess_draw(False, cam)
    assert np.array_equal(rgb2cam.numpy(), R.CCMS[cam])
    for name, t in (('cam2rgb', cam2rgb), ('rgb_gain', rgb_gain), ('red_gain', red_gain), ('blue_gain', blue_gain)):
        assert t.dtype == torch.float32 and t.shape == gold[f'{key}_{name}'].shape, name
        assert np.array_equal(t.numpy().view(np.uint32), gold[f'{key}_{name}'].view(np.uint32)), name
    assert np.array_equal(torch.get_rng_state().numpy(), gold[key + '_torch_state'])
    st = np.random.get_state()
    assert np.array_equal(st[1], gold[key + '_np_keys']) and st[2] == int(gold[key + '_np_pos'])
    # the 4-D case was recorded under the same seeds: one draw for the whole stack
    assert np.array_equal(gold[f'f_{cam}_4d_red_gain'], gold[key + '_red_gain']) and np.array_equal(gold[f'f_{cam}_4d_rgb_gain'], gold[key + '_rgb_gain'])
    # locked gains: taken as given, nothing drawn
    before = (torch.get_rng_state().clone(), np.random.get_state()[2])
    _, _, rgb_gain, red_gain, blue_gain = U.unprocess_draw(([1.], [2.1], [1.7]), cam)
    assert [t.tolist() for t in (rgb_gain, red_gain, blue_gain)] == [[1.0], [float(np.float32(2.1))], [float(np.float32(1.7))]]
    assert torch.equal(torch.get_rng_state(), before[0]) and np.random.get_state()[2] == before[1]


def test_rows_pack_the_reference_s_float32_gains(gold):
    from pnnp_amd import unprocess as U
    m, g, gains = gold['b_m'], gold['b_g'], gold['b_gains']
    rows = U.unprocess_rows(m, g[:, 0], g[:, 1], g[:, 2], 3, device='cpu')
    assert rows.shape == (3, U.UNP_NPARAM) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert np.array_equal(rows[:, :9].numpy().view(np.uint32), m.reshape(3, 9).view(np.uint32))
    assert np.array_equal(rows[:, 9:12].numpy().view(np.uint32), gains.view(np.uint32))          # bitwise the reference's `gains`
    assert rows[:, 12:].abs().sum() == 0
    # one shared matrix and one shared draw, tensors of shape [1] as random_gains returns them
    one = U.unprocess_rows(torch.from_numpy(m[0]), torch.tensor([g[1, 0]]), torch.tensor([g[1, 1]]), torch.tensor([g[1, 2]]), 2, device='cpu')
    assert one.shape == (2, U.UNP_NPARAM) and torch.equal(one[0], one[1])
    assert np.array_equal(one[0, 9:12].numpy().view(np.uint32), gains[1].view(np.uint32)) and np.array_equal(one[0, :9].numpy(), m[0].reshape(9))
    # the seeded case: the draws of `unprocess` give the gains the reference multiplied with
    key = 'f_IMX686_3d'
    row = U.unprocess_rows(R.CCMS['IMX686'], gold[key + '_rgb_gain'], gold[key + '_red_gain'], gold[key + '_blue_gain'], 1, device='cpu')
    want = R.gains_f32(gold[key + '_rgb_gain'], gold[key + '_red_gain'], gold[key + '_blue_gain'])
    assert np.array_equal(row[0, 9:12].numpy().view(np.uint32), want.view(np.uint32))
    from pnnp_amd._lib import PnnpError
    with pytest.raises(PnnpError):
        U.unprocess_rows(m[:2], g[:, 0], g[:, 1], g[:, 2], 3, device='cpu')      # neither one matrix nor one per image
    with pytest.raises(PnnpError):
        U.unprocess_rows(m, g[:2, 0], g[:, 1], g[:, 2], 3, device='cpu')


def test_argument_checks_raise_without_a_device():
    from pnnp_amd import unprocess as U
    from pnnp_amd._lib import PnnpError
    rows = torch.zeros(1, U.UNP_NPARAM)
    with pytest.raises(PnnpError, match='even'):
        U.unprocess_batch(torch.zeros(1, 5, 4, 3), rows, packed='RGGB')          # odd H
    with pytest.raises(PnnpError, match='even'):
        U.unprocess_batch(torch.zeros(1, 3, 4, 7), rows, layout='chw', packed='GBRG')   # odd W
    with pytest.raises(PnnpError):
        U.unprocess_batch(torch.zeros(1, 4, 4, 4), rows)                         # wrong channel count
    with pytest.raises(PnnpError):
        U.unprocess_batch(torch.zeros(1, 4, 4, 3), rows, layout='chw')           # channel-last data under 'chw'
    with pytest.raises(PnnpError):
        U.unprocess_batch(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), rows, layout='chw')
    with pytest.raises(PnnpError):
        U.unprocess_batch(torch.zeros(1, 4, 4, 3), rows, layout='nhwc')
    with pytest.raises(PnnpError):
        U.unprocess_batch(torch.zeros(1, 4, 4, 3), rows, packed='BGGR')
    with pytest.raises(PnnpError, match='no output'):
        U.unprocess_batch(torch.zeros(1, 4, 4, 3), rows, rgb=False)
    with pytest.raises(PnnpError):
        U.unprocess_batch(torch.zeros(1, 4, 4, 3), rows)                         # a host tensor: there is no CPU implementation
    state = (torch.get_rng_state().clone(), np.random.get_state()[2])
    for bad in (torch.zeros(2, 2, 2, 2, 4, 3), torch.zeros(4, 3), torch.zeros(4, 4, 4)):          # more than 5 dimensions, fewer than 3, not RGB
        with pytest.raises(PnnpError):
            U.unprocess(bad)
    assert torch.equal(torch.get_rng_state(), state[0]) and np.random.get_state()[2] == state[1]  # refused before anything is drawn
    for fn in (U.mosaic, U.mosaic_GBRG):
        with pytest.raises(PnnpError, match='even'):
            fn(torch.zeros(3, 4, 3))
        with pytest.raises(PnnpError):
            fn(torch.zeros(4, 4, 4))
        with pytest.raises(PnnpError):
            fn(torch.zeros(4, 4, 3))                                             # a host tensor
    for fn, a in ((U.inverse_smoothstep, (torch.zeros(4, 4, 3),)), (U.gamma_expansion, (torch.zeros(4, 4, 3),)),
                  (U.apply_ccm, (torch.zeros(4, 4, 3), torch.eye(3))),
                  (U.safe_invert_gains, (torch.zeros(4, 4, 3), torch.ones(1), torch.ones(1), torch.ones(1)))):
        with pytest.raises(PnnpError):
            fn(*a)


def test_step_rgb_refuses_bad_crops_without_a_device():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.trainer import HipTrainStep
    step = HipTrainStep.__new__(HipTrainStep)                                    # the checks run before any state is touched
    step.camera_type = 'SonyA7S2'
    state = (torch.get_rng_state().clone(), np.random.get_state()[2])
    with pytest.raises(PnnpError, match='even'):
        step.step_rgb(torch.zeros(2, 6, 7, 3))
    with pytest.raises(PnnpError):
        step.step_rgb(torch.zeros(2, 4, 8, 8))
    with pytest.raises(PnnpError, match='CUDA'):
        step.step_rgb(torch.zeros(2, 8, 8, 3))
    assert torch.equal(torch.get_rng_state(), state[0]) and np.random.get_state()[2] == state[1]


def test_preprocess_branch_of_the_run_files():
    from pnnp_amd import runfile
    cfg = runfile.load(os.path.join(FIXTURES, 'runfile_sony_img.yml'))
    assert cfg['dst_train']['dataset'] == 'Img_Dataset' and runfile.preprocess_branch(cfg['dst_train']) == 'rgb'
    unchanged = {'runfile_sony.yml': 'physics', 'runfile_sony_pmn.yml': 'mix', 'runfile_imx686_pmn.yml': 'mix', 'runfile_imx686_nf.yml': 'proxy',
                 'runfile_noiseflow.yml': 'physics'}
    for name, branch in unchanged.items():
        c = runfile.load(os.path.join(FIXTURES, name))
        assert runfile.preprocess_branch(c.get('dst_train', c.get('dst'))) == branch, name
    assert runfile.preprocess_branch({'dataset': 'IMX686_SFRN_Raw_Dataset'}) == 'sfrn' and runfile.preprocess_branch(None) == 'physics'
