#!/usr/bin/env python3
"""Generate tests/golden/mix.npz + mix.json by running the REAL reference: the paired-data branches of Trainer.preprocess
(trainer_SID.py:430-447, trainer_LRID.py:367-397) and get_aug_param_torch (process.py:415-445).

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_mix.py

Part 1, get_aug_param_torch under fixed np.random.seed / torch.manual_seed: 'augv2', 'augv5' and a command naming neither, b = 1 and 6,
tensor and numpy=True returns, and the global RNG states left behind.  The seeds are SEARCHED so that, per scheme, both outcomes of
randint(4) occur and (augv5) the renormalisation `daug < 0` occurs; the generator asserts this coverage before it writes anything.

Part 2, the preprocess branch itself.  Both trainer modules import under the stubs, so the real ``preprocess`` of ``SID_Trainer`` and
``IMX686_Trainer`` is called UNBOUND on a stand-in ``self`` (device 'cpu', use_gpu True, the `dst` dictionary of the case); no loop of
our own stands in for it.  Batch: 3 images x 2 crops of 4x32x32.  Cases cover ori both ways, clip in {False, True, 2}, black_lr both
ways, the IMX686_SFRN_Raw_Dataset branch, a batch whose six crops are all inactive (augv2 on the randint(4) == 0 path, black_lr False)
and a MIXED batch (augv2 clamps all three gains of a crop to zero with probability 1/8: the seed is searched for a batch with active
and inactive crops; the SFRN branch cannot supply one, its gains are all one).  Every case is run a second time from the same seeds with
clip off for the moments of `lr_out - lr_scaled` per crop and plane.  K of the active crops is read from the parameter dictionaries
SNA_torch fills in.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def rng_marks():
    import torch
    return [int(v) for v in np.random.get_state()[1][:4]], [int(v) for v in torch.get_rng_state()[:16]]


def first_draws(seed):
    np.random.seed(seed)
    return int(np.random.randint(2)), int(np.random.randint(4))


def gen_aug(proc, out, meta):
    import torch
    wbs = {1: torch.tensor([[2.13, 1.0, 1.57, 1.0]]), 6: torch.tensor([[2.13, 1.0, 1.57, 1.0]]).repeat(6, 1) * torch.linspace(0.9, 1.1, 6).view(6, 1)}
    cases = []
    seen = {}
    for command, cam in (('augv2, idremap, HB', 'SonyA7S2'), ('alldg, augv5', 'SonyA7S2'), ('alldg, augv5', 'IMX686'), ('idremap, HB', 'SonyA7S2')):
        scheme = 'augv5' if 'augv5' in command else ('augv2' if 'augv2' in command else 'none')
        for b in (1, 6):
            want = {('r4', False), ('r4', True)} | ({('renorm', True)} if scheme == 'augv5' else set())
            for seed in range(200):
                if not want:
                    break
                r4 = first_draws(seed)[1] != 0
                flag = {}
                orig_min = torch.min

                def spy(*a, **k):
                    res = orig_min(*a, **k)
                    flag['renorm'] = bool((res[0] < 0).any())
                    return res
                np.random.seed(seed); torch.manual_seed(seed)
                torch.min = spy
                try:
                    data = {'wb': wbs[b].clone()}
                    ar, ag, ab = proc.get_aug_param_torch(data, b=b, command=command, camera_type=cam)
                finally:
                    torch.min = orig_min
                marks = rng_marks()
                hit = {('r4', r4)} | ({('renorm', True)} if flag['renorm'] else set())
                if not (hit & want):
                    continue
                want -= hit
                np.random.seed(seed); torch.manual_seed(seed)
                nr, ng, nb = proc.get_aug_param_torch({'wb': wbs[b].clone()}, b=b, command=command, numpy=True, camera_type=cam)
                tag = f'aug{len(cases)}'
                out[tag + '_wb'] = wbs[b].numpy()
                out[tag + '_t'] = np.stack([ar.numpy(), ag.numpy(), ab.numpy()])
                out[tag + '_n'] = np.stack([np.asarray(nr), np.asarray(ng), np.asarray(nb)])
                cases.append(dict(tag=tag, command=command, camera_type=cam, b=b, seed=seed, randint4_nonzero=r4, renorm=flag['renorm'],
                                  numpy_shape=list(np.shape(nr)), np_state=marks[0], torch_state=marks[1]))
                seen.setdefault(scheme, set()).update(hit)
            assert not want, (command, b, want)
    assert {('r4', False), ('r4', True)} <= seen['augv2'] and {('r4', False), ('r4', True), ('renorm', True)} <= seen['augv5']
    assert {('r4', False), ('r4', True)} <= seen['none']
    meta['aug'] = cases


def run_preprocess(trainer_cls, proc_mod, dataset, dst, data, seed):
    """The reference's preprocess, unbound, on a stand-in self.  -> (lr_out, hr_out, ratio, data after, K of the active crops)"""
    import torch
    me = types.SimpleNamespace(device='cpu', use_gpu=True, dst_train=None, dst_eval=None, dst=dict(dst), args={'dst_train': {'dataset': dataset}})
    captured = []
    orig = proc_mod.get_specific_noise_params

    def spy(*a, **k):
        p = orig(*a, **k)
        captured.append(p)
        return p
    proc_mod.get_specific_noise_params = spy
    d = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in data.items()}
    np.random.seed(seed); torch.manual_seed(seed)
    try:
        lr, hr, ratio = trainer_cls.preprocess(me, d, mode='train', preprocess=True)
    finally:
        proc_mod.get_specific_noise_params = orig
    return lr, hr, ratio, d, [float(p['K']) for p in captured], [(int(p['wp']), int(p['bl'])) for p in captured]


def gen_preprocess(proc, out, meta):
    import torch
    import trainer_LRID
    import trainer_SID
    # SNA_torch looks get_specific_noise_params up in ITS module's globals: the spy goes there
    rng = np.random.RandomState(77)
    hr = (np.round(rng.rand(3, 2, 4, 32, 32) ** 2 * 1024) / 1024).astype(np.float32)          # [0, 1], 10-bit values
    inputs = {}
    for cam, ratios, isos in (('SonyA7S2', [[100., 250.], [300., 150.], [200., 120.]], [800, 1600, 3200]),
                              ('IMX686', [[1., 2.], [4., 8.], [16., 2.]], [100, 6400, 6400])):
        ratio = torch.tensor(ratios)
        lr = torch.from_numpy(hr) / ratio.view(3, 2, 1, 1, 1) + torch.from_numpy(rng.randn(3, 2, 4, 32, 32).astype(np.float32)) * 0.02 / ratio.view(3, 2, 1, 1, 1)
        inputs[cam] = dict(lr=lr.float(), ratio=ratio, ISO=torch.tensor(isos))
        out[f'in_{cam}_lr'] = lr.float().numpy().reshape(6, 4, 32, 32)
    out['in_hr'] = hr.reshape(6, 4, 32, 32)
    wb3 = torch.tensor([[2.13, 1.0, 1.57, 1.0], [1.9, 1.0, 1.7, 1.0], [2.3, 1.0, 1.4, 1.0]])

    def find_seed(command, black, pred):
        """first seed whose six crops satisfy pred(active flags)"""
        for seed in range(500):
            np.random.seed(seed); torch.manual_seed(seed)
            ar, ag, ab = proc.get_aug_param_torch({'wb': wb3[:1].clone()}, b=6, command=command)
            aug = torch.stack((ar, ag, ab, ag), dim=1).numpy() + (1 if black else 0)
            act = np.abs(aug).max(axis=1) != 0
            if pred(act):
                return seed
        raise AssertionError('no seed found')

    mixed = lambda a: a.any() and not a.all() and not a[0] and a[1]        # noqa: E731  (an inactive crop FIRST: its K draw must not happen)
    spec = [
        # tag, trainer, dataset, camera, command, ori, clip, black_lr, wb, seed
        ('sid_mixed', trainer_SID.SID_Trainer, 'Mix_Dataset', 'SonyA7S2', 'augv2, idremap, darkshading2++, HB', False, False, False, wb3, ('find', mixed)),
        ('sid_black', trainer_SID.SID_Trainer, 'Mix_Dataset', 'SonyA7S2', 'augv2, idremap, darkshading2++, HB', True, 2, True, wb3, ('r4',)),
        ('lrid_v5', trainer_LRID.IMX686_Trainer, 'IMX686_Mix_Dataset', 'IMX686', 'alldg, augv5', False, True, False, wb3[:1], ('r4',)),
        ('lrid_idle', trainer_LRID.IMX686_Trainer, 'IMX686_Mix_Dataset', 'IMX686', 'alldg, darkshading2++, augv2, HB', True, False, False, wb3,
         ('find', lambda a: not a.any())),
        ('sfrn', trainer_LRID.IMX686_Trainer, 'IMX686_SFRN_Raw_Dataset', 'IMX686', 'alldg', False, 2, False, wb3, ('fixed', 5)),
    ]
    cases = []
    for tag, cls, dataset, cam, command, ori, clip, black, wb, how in spec:
        if how[0] == 'find':
            seed = find_seed(command, black, how[1])
        elif how[0] == 'r4':                                      # the randint(4) != 0 path: gains are drawn
            seed = next(s for s in range(100) if first_draws(s)[1] != 0)
        else:
            seed = how[1]
        I = inputs[cam]
        data = dict(hr=torch.from_numpy(hr), lr=I['lr'], ratio=I['ratio'], ISO=I['ISO'], wb=wb, black_lr=torch.tensor([black] * 3))
        dst = dict(command=command, ori=ori, clip=clip, crop_per_image=2, camera_type=cam)
        lr_o, hr_o, ratio_o, d, Ks, spans = run_preprocess(cls, proc, dataset, dst, data, seed)
        # the same draws with clip off: moments of the added noise per crop and plane
        lr_n, hr_n, _, _, Ks2, _ = run_preprocess(cls, proc, dataset, dict(dst, clip=False), data, seed)
        assert Ks == Ks2
        rr = I['ratio'].view(-1, 1, 1, 1)
        lr_scaled = I['lr'].reshape(6, 4, 32, 32) if ori else I['lr'].reshape(6, 4, 32, 32) * rr
        diff = (lr_n - lr_scaled).numpy().astype(np.float64).reshape(6, 4, -1)
        hr_in = torch.from_numpy(hr).reshape(6, 4, 32, 32)
        active = [bool((diff[i] != 0).any() or not torch.equal(hr_n[i], hr_in[i])) for i in range(6)]
        assert sum(active) == len(Ks), (tag, active, Ks)
        if tag == 'sid_mixed':
            assert any(active) and not all(active)
        if tag == 'lrid_idle':
            assert not any(active) and torch.equal(hr_o, hr_in)
        if tag != 'lrid_idle':
            out[tag + '_hr_out'] = hr_o.numpy()
        out[tag + '_ratio'] = ratio_o.numpy()
        out[tag + '_wb_in'] = wb.numpy()
        sfrn = dataset == 'IMX686_SFRN_Raw_Dataset'
        if not sfrn:
            out[tag + '_wb'] = d['wb'].numpy()
            out[tag + '_rgb_gain'] = d['rgb_gain'].numpy()
        out[tag + '_dmean'] = diff.mean(-1)
        out[tag + '_dvar'] = diff.var(-1)
        cases.append(dict(tag=tag, trainer=cls.__module__, dataset=dataset, camera_type=cam, command=command, ori=ori, clip=clip,
                          black_lr=black, crop_per_image=2, seed=seed, sfrn=sfrn, active=active, K=Ks, wp_bl=[list(s) for s in spans],
                          hr_out_is_input=tag == 'lrid_idle', wb_dtype=str(d['wb'].dtype) if not sfrn else None))
    assert {c['ori'] for c in cases} == {False, True} and {repr(c['clip']) for c in cases} == {'False', 'True', '2'}
    assert {c['black_lr'] for c in cases} == {False, True} and any(not all(c['active']) for c in cases)
    meta['preprocess'] = cases


def main():
    archs, proc, isp, losses, data_process, base_trainer = import_reference()
    out, meta = {}, {}
    gen_aug(proc, out, meta)
    gen_preprocess(proc, out, meta)
    np.savez_compressed(os.path.join(HERE, 'mix.npz'), **out)
    json.dump(meta, open(os.path.join(HERE, 'mix.json'), 'w'), indent=1)
    print('mix fixtures written:', os.path.getsize(os.path.join(HERE, 'mix.npz')), 'bytes')


if __name__ == '__main__':
    main()
