"""The paired-data preprocess branch on the device (Mix_Dataset / IMX686_Mix_Dataset / IMX686_SFRN_Raw_Dataset; trainer_SID.py:430-447,481-485,
trainer_LRID.py:367-397): ``process.sna_batch`` (csrc/noise.hip: sna_batch_kernel), ``HipTrainStep.make_noisy_mix`` / ``step_paired`` and the
run files that select them.

The batched pass is held BIT-EQUAL to the per-crop entry ``pnnp_sna_f32`` followed by the trainer's torch ops; that entry is held to the C oracle
and to the reference's moments by test_gpu_sna.py, so the draw's correctness carries over.  Against the reference's own preprocess
(tests/golden/mix.*): everything deterministic exact, the noise by its per-plane mean (5 sigma of the sampling error of two independent means,
the bar of test_gpu_sna.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# [3,4,6,10]: W % 4 != 0; [2,4,32,32]: every quad inside a row; [2,4,5,7]: H*W % 4 != 0, quads straddle planes
SHAPES = [(3, 4, 6, 10), (2, 4, 32, 32), (2, 4, 5, 7)]
AUG = np.array([0.5, 0.25, 1.0, 0.75], np.float32)
WP, BL = 1023.0, 64.0
INACTIVE = 1                                               # the middle crop of three, the last of two


def _batch(shape, offset_elems=0):
    """hr: a squared ramp per plane (rates 0, (0,10) and >= 10 in every plane of every active crop, asserted); lr: hr / ratio + noise around zero,
    so that both clamps bite.  ``offset_elems``: the tensors start that many floats past a 16-byte boundary (the kernel's element-wise path)."""
    B, Cc, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + H * W)
    ramp = torch.linspace(0, 1.15, H * W) ** 2
    hr = torch.stack([torch.stack([ramp.roll(3 * c + b) for c in range(Cc)]) for b in range(B)]).reshape(shape).float()
    K = np.array([2.0, 1.5, 0.75][:B], np.float64)
    ratio = np.array([4.0, 2.0, 8.0][:B], np.float32)
    lr = hr / torch.from_numpy(ratio).view(B, 1, 1, 1) + 0.05 * torch.randn(shape, generator=g) - 0.01
    active = np.array([i != INACTIVE for i in range(B)])
    for i in range(B):
        lam = hr[i].reshape(Cc, -1).numpy() * np.float32(WP - BL) / ratio[i] * AUG[:, None] / np.float32(K[i])
        assert all((l == 0).any() and ((l > 0) & (l < 10)).any() and (l >= 10).any() for l in lam), 'the ramp must cover all three Poisson paths'

    def dev(t):
        buf = torch.empty(t.numel() + 4, device='cuda')
        assert buf.data_ptr() % 16 == 0
        v = buf[offset_elems:offset_elems + t.numel()].view(t.shape)
        v.copy_(t)
        return v
    return dev(lr), dev(hr), K, ratio, active


def _rows(K, ratio, active, black_lr, add_dy):
    from pnnp_amd import process as P
    B = len(K)
    return P.pack_sna_rows(np.tile(AUG, (B, 1)), np.where(active, K, 0.0), WP, BL, ratio, active, black_lr=black_lr, add_dy=add_dy)


def _composition(lr, hr, K, ratio, active, black_lr, add_dy, ori, clip, seed, offset, crop_base):
    """The loop the batched pass replaces: pnnp_sna_f32 per active crop, then torch's mul / add / clamp (trainer_SID.py:436-447,481-485)."""
    from pnnp_amd import _lib
    B, Cc, H, W = lr.shape
    lo, ho = torch.empty_like(lr), torch.empty_like(hr)
    aug = (C.c_float * 4)(*[float(v) for v in AUG])
    rt = torch.from_numpy(ratio).cuda()
    for i in range(B):
        l = lr[i] if ori else lr[i] * rt[i]
        h = hr[i]
        if active[i]:
            gt = hr[i].contiguous()
            dn, dy = torch.empty_like(gt), torch.empty_like(gt)
            _lib.check(_lib.lib().pnnp_sna_f32(_lib.ptr(gt), _lib.ptr(dn), _lib.ptr(dy), Cc, H, W, aug, C.c_float(float(K[i])), C.c_float(WP),
                                               C.c_float(BL), C.c_float(float(ratio[i])), int(black_lr), int(ori), C.c_uint64(seed),
                                               C.c_uint64(offset), C.c_uint32(crop_base + i), _lib.stream()), 'sna')
            l = l + dn
            if add_dy:
                h = h + dy
        lo[i], ho[i] = l, h
    if clip:
        lo = lo.clamp(max=1) if clip == 2 else lo.clamp(0, 1)
        ho = ho.clamp(0, 1)
    return lo, ho


@pytest.mark.parametrize('crop_base', [0, 5])
@pytest.mark.parametrize('shape,offset_elems', [(s, 0) for s in SHAPES] + [(SHAPES[0], 1), (SHAPES[1], 3)])
def test_batched_pass_is_bit_equal_to_the_per_crop_path(shape, offset_elems, crop_base):
    from pnnp_amd import process as P
    lr, hr, K, ratio, active = _batch(shape, offset_elems)
    lr0, hr0 = lr.clone(), hr.clone()
    bit = {False: False, True: False}
    for ori in (False, True):
        for clip in (False, True, 2):
            for black_lr in (False, True):
                for add_dy in (False, True):
                    got_l, got_h = P.sna_batch(lr, hr, _rows(K, ratio, active, black_lr, add_dy), ori, clip, seed=77, offset=9, crop_base=crop_base)
                    ref_l, ref_h = _composition(lr, hr, K, ratio, active, black_lr, add_dy, ori, clip, 77, 9, crop_base)
                    what = (ori, clip, black_lr, add_dy)
                    assert torch.equal(got_l, ref_l), what
                    assert torch.equal(got_h, ref_h), what
                    if clip:
                        assert float(got_l.max()) <= 1 and float(got_h.max()) <= 1 and float(got_h.min()) >= 0
                        assert (float(got_l.min()) < 0) == (clip == 2), what          # HALF_CLIP keeps the negative pixels
                        bit[ori] |= bool((got_l == 1).any())
                    if not add_dy:
                        assert torch.equal(got_h, hr.clamp(0, 1) if clip else hr)
    assert bit[False]                                                             # the upper clamp really bites (brightened crops)
    assert torch.equal(lr, lr0) and torch.equal(hr, hr0)                          # the inputs are not written


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_outputs_may_alias_their_inputs(shape):
    from pnnp_amd import process as P
    lr, hr, K, ratio, active = _batch(shape)
    rows = _rows(K, ratio, active, True, True)
    want_l, want_h = P.sna_batch(lr, hr, rows, False, 2, seed=3, offset=4)
    l2, h2 = lr.clone(), hr.clone()
    got_l, got_h = P.sna_batch(l2, h2, rows, False, 2, seed=3, offset=4, out_lr=l2, out_hr=h2)
    assert got_l is l2 and got_h is h2 and torch.equal(l2, want_l) and torch.equal(h2, want_h)


@pytest.mark.parametrize('shape', SHAPES[:2])
def test_a_shard_equals_its_rows_of_the_whole_batch(shape):
    from pnnp_amd import process as P
    lr, hr, K, ratio, active = _batch(shape)
    rows = _rows(K, ratio, active, False, True)
    B = shape[0]
    for base in (0, 5):
        whole_l, whole_h = P.sna_batch(lr, hr, rows, False, False, seed=3, offset=4, crop_base=base)
        part_l, part_h = P.sna_batch(lr[1:B], hr[1:B], rows[1:B].contiguous(), False, False, seed=3, offset=4, crop_base=base + 1)
        assert torch.equal(part_l, whole_l[1:B]) and torch.equal(part_h, whole_h[1:B])
        first_l, _ = P.sna_batch(lr[:1], hr[:1], rows[:1].contiguous(), False, False, seed=3, offset=4, crop_base=base)
        assert torch.equal(first_l, whole_l[:1])


@pytest.mark.parametrize('shape', SHAPES[:2])
@pytest.mark.parametrize('ori', [False, True])
def test_same_counters_same_sample(shape, ori):
    from pnnp_amd import process as P
    lr, hr, K, ratio, active = _batch(shape)
    rows = _rows(K, ratio, active, False, True)
    a_l, a_h = P.sna_batch(lr, hr, rows, ori, False, seed=3, offset=4)
    b_l, b_h = P.sna_batch(lr, hr, rows, ori, False, seed=3, offset=4)
    c_l, c_h = P.sna_batch(lr, hr, rows, ori, False, seed=3, offset=5)
    assert torch.equal(a_l, b_l) and torch.equal(a_h, b_h)
    assert torch.equal(a_h, c_h)                                                  # the signal change carries no noise
    rt = torch.from_numpy(ratio).cuda().view(-1, 1, 1, 1)
    for i in range(shape[0]):
        if active[i]:
            assert not torch.equal(a_l[i], c_l[i])
        else:
            assert torch.equal(a_l[i], lr[i] if ori else (lr * rt)[i]) and torch.equal(c_l[i], a_l[i]) and torch.equal(a_h[i], hr[i])
    # the module's own counter advances like noise_sample's
    P.manual_seed(3, offset=4)
    d_l, _ = P.sna_batch(lr, hr, rows, ori, False)
    assert torch.equal(d_l, a_l) and P.get_rng_state() == (3, 5)


class _Net:                                                # make_noisy_mix never touches the network
    engine = None


@pytest.fixture(scope='module')
def G(golden_dir):
    return np.load(os.path.join(golden_dir, 'mix.npz')), json.load(open(os.path.join(golden_dir, 'mix.json')))


RATIO = {'SonyA7S2': [[100., 250.], [300., 150.], [200., 120.]], 'IMX686': [[1., 2.], [4., 8.], [16., 2.]]}      # make_golden_mix.py
ISO = {'SonyA7S2': [800, 1600, 3200], 'IMX686': [100, 6400, 6400]}


@pytest.mark.parametrize('tag', ['sid_mixed', 'sid_black', 'lrid_v5', 'lrid_idle', 'sfrn'])
def test_make_noisy_mix_against_the_reference(G, tag):
    from pnnp_amd.trainer import HipTrainStep
    g, meta = G
    c = next(x for x in meta['preprocess'] if x['tag'] == tag)
    cam = c['camera_type']
    lr, hr = torch.from_numpy(g[f'in_{cam}_lr']).cuda(), torch.from_numpy(g['in_hr']).cuda()
    data = dict(ratio=torch.tensor(RATIO[cam]), ISO=torch.tensor(ISO[cam]), wb=torch.from_numpy(g[tag + '_wb_in']),
                black_lr=torch.tensor([c['black_lr']] * 3))
    wb_before = data['wb'].clone()
    ts = HipTrainStep(_Net(), camera_type=cam, ori=c['ori'], clip=c['clip'], seed=21)
    ts.step_count = 3
    kw = dict(command=c['command'], crop_per_image=c['crop_per_image'], sfrn=c['sfrn'])
    np.random.seed(c['seed']); torch.manual_seed(c['seed'])
    noisy, hr_aug, ratio, info = ts.make_noisy_mix(lr, hr, data, **kw)
    assert torch.equal(data['wb'], wb_before) and torch.equal(hr.cpu(), torch.from_numpy(g['in_hr']))        # nothing of the caller's is modified
    want_hr = g['in_hr'] if c['hr_out_is_input'] else g[tag + '_hr_out']
    assert np.array_equal(hr_aug.cpu().numpy(), want_hr)
    assert ratio.is_cuda and np.array_equal(ratio.cpu().numpy(), g[tag + '_ratio'])
    if c['sfrn']:
        assert 'wb' not in info and 'rgb_gain' not in info
    else:
        assert str(info['wb'].dtype) == c['wb_dtype'] and np.array_equal(info['wb'].numpy(), g[tag + '_wb'])
        assert np.array_equal(info['rgb_gain'].numpy(), g[tag + '_rgb_gain'].reshape(-1))
    assert [float(k) for k, a in zip(info['K'], c['active']) if a] == c['K']
    rt = torch.tensor(RATIO[cam]).view(6, 1, 1, 1).cuda()
    scaled = lr if c['ori'] else lr * rt
    clamp = (lambda t: t) if not c['clip'] else ((lambda t: t.clamp(max=1)) if c['clip'] == 2 else (lambda t: t.clamp(0, 1)))
    for i in range(6):
        if not c['active'][i]:
            assert torch.equal(noisy[i], clamp(scaled[i])), i
    # the noise itself, with clip off, from the same host draws
    ts.clip = False
    np.random.seed(c['seed']); torch.manual_seed(c['seed'])
    noisy, _, _, _ = ts.make_noisy_mix(lr, hr, data, **kw)
    diff = (noisy - scaled).double().reshape(6, 4, -1).cpu().numpy()
    n = diff.shape[-1]
    mean_ref, var_ref = g[tag + '_dmean'], g[tag + '_dvar']
    for i in range(6):
        for p in range(4):
            if not c['active'][i] or var_ref[i, p] == 0.0:
                assert mean_ref[i, p] == 0.0 and not diff[i, p].any(), (i, p)
            else:
                assert abs(diff[i, p].mean() - mean_ref[i, p]) < 5 * np.sqrt(2 * var_ref[i, p] / n), (i, p, diff[i, p].mean(), mean_ref[i, p])


def _tiny_net(seed=3):
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    torch.manual_seed(seed)
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=8, in_nc=4, out_nc=4))
    initialize_weights(net)
    return net.cuda()


@pytest.mark.parametrize('ori', [False, True])
def test_step_paired_is_make_noisy_mix_then_step(ori):
    from pnnp_amd import process as P
    from pnnp_amd.trainer import HipTrainStep
    from pnnp_amd._lib import PnnpError
    mix = dict(command='augv2, idremap', crop_per_image=2, sfrn=False)
    g = torch.Generator().manual_seed(8)
    hr = (torch.rand(2, 4, 32, 32, generator=g) * 0.8).cuda()
    data = dict(ratio=torch.tensor([[100., 250.]]), ISO=torch.tensor([1600]), wb=torch.tensor([[2.1, 1.0, 1.6, 1.0]]), black_lr=torch.tensor([True]))
    lr_in = hr / data['ratio'].view(2, 1, 1, 1).cuda() + 1e-4 * torch.randn(2, 4, 32, 32, generator=g).cuda()
    results = []
    for paired in (True, False):
        net = _tiny_net()
        ts = HipTrainStep(net, lr=1e-3, camera_type='SonyA7S2', ori=ori, clip=2, seed=5, mix=mix)
        np.random.seed(0); torch.manual_seed(0)
        if paired:
            loss = ts.step_paired(lr_in, hr, data)
            assert set(ts.mix_info) == {'wb', 'rgb_gain', 'K'}
        else:
            noisy, hr_aug, ratio, _ = ts.make_noisy_mix(lr_in, hr, data, **mix)
            loss = ts.step(hr_aug, noisy=noisy, ratio=ratio)
            # sampler level: the batch as two half-batches, crop_base by hand (world = 1, global_batch = None)
            np.random.seed(0); torch.manual_seed(0)
            aug = torch.stack([t for t in P.get_aug_param_torch(data, b=2, command=mix['command'])] , dim=1)[:, [0, 1, 2, 1]]
            rows, _ = P.sna_rows(aug, data['ratio'].view(-1), data['ISO'], 'SonyA7S2', True, 2)
            halves = [P.sna_batch(lr_in[i:i + 1], hr[i:i + 1], rows[i:i + 1].contiguous(), ori, 2, seed=5, offset=0, crop_base=i) for i in range(2)]
            assert torch.equal(torch.cat([h[0] for h in halves]), noisy) and torch.equal(torch.cat([h[1] for h in halves]), hr_aug)
        assert ts.step_count == 1 and bool(torch.isfinite(loss).all())
        results.append((loss.clone(), net.engine.params.flat.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    with pytest.raises(PnnpError):
        HipTrainStep(_tiny_net(), clip=2).step_paired(lr_in, hr, data)                 # no mix= settings


@pytest.mark.parametrize('fixture', ['runfile_sony_pmn.yml', 'runfile_imx686_pmn.yml'])
def test_paired_run_files_run(fixture, capsys):
    from pnnp_amd import runfile
    path = os.path.join(HERE, 'fixtures', fixture)
    cfg = runfile.load(path)
    step = runfile.build(cfg)[1]
    assert step.mix == dict(command=cfg['dst_train']['command'], crop_per_image=cfg['dst_train']['crop_per_image'], sfrn=False)
    assert step.proxy_net is None
    assert runfile.main([path, '--synthetic', '--patch', '32', '--epochs', '1', '--steps', '2']) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('Epoch')][-1]
    loss = float(line.split('| loss')[1].split('|')[0])
    assert np.isfinite(loss) and loss > 0, line


def test_errors():
    from pnnp_amd import process as P
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.trainer import HipTrainStep
    lr, hr, K, ratio, active = _batch(SHAPES[0])
    rows = _rows(K, ratio, active, False, True)
    with pytest.raises(PnnpError):
        P.sna_batch(lr.cpu(), hr, rows, False, False)                                   # no CPU path
    with pytest.raises(PnnpError):
        P.sna_batch(lr, hr, rows.cpu(), False, False)
    with pytest.raises(PnnpError):
        P.sna_batch(lr, hr, rows[:2].contiguous(), False, False)                        # one row per crop
    with pytest.raises(PnnpError):
        P.pack_sna_rows(np.tile(AUG, (3, 1)), [1.0, 0.0, 1.0], WP, BL, ratio, [True, True, True])      # an active row with K <= 0
    with pytest.raises(PnnpError):
        P.pack_sna_rows(np.tile(AUG, (3, 1)), [1.0, -2.0, 1.0], WP, BL, ratio, [True, True, True])
    data = dict(ratio=torch.tensor([2., 2., 2.]), ISO=torch.tensor([123]), wb=torch.tensor([[2.1, 1.0, 1.6, 1.0]]), black_lr=torch.tensor([True]))
    ts = HipTrainStep(_Net(), camera_type='IMX686', clip=False)
    with pytest.raises(KeyError):
        ts.make_noisy_mix(lr, hr, data, command='augv2', crop_per_image=3)              # not a calibrated ISO: dict lookup, like SNA_torch
    with pytest.raises(PnnpError):
        ts.make_noisy_mix(lr.cpu(), hr.cpu(), dict(data, ISO=torch.tensor([6400])), command='augv2', crop_per_image=3)
