"""csrc/unprocess.hip on the device: the reference's own outputs (tests/golden/unprocess.npz) under the agreement rule of
tests/_unprocess_ref.py (every element within max(4 x the reference's own error against float64, one float32 ulp), absolutely and
relatively; no element excepted), the three input kinds, both Bayer patterns, the vector and the element paths, ``unprocess`` / ``mosaic``
with the reference's signatures, the round trip through the render kernel, ``HipTrainStep.step_rgb`` and the run file that selects it.

Observed on the MI355X (profiles/r7/unprocess.txt), largest error against float64, kernel | reference (the bar is 4 x the reference's):
    case   abs                    rel
    a      3.66e-7 | 4.54e-7      6.92e-7 | 9.85e-7
    b      7.80e-7 | 7.80e-7      1.40e-6 | 6.17e-4
    c      9.89e-7 | 9.89e-7      1.32e-6 | 1.24e-6
    d      8.43e-9 | 6.47e-9      2.95e-7 | 1.39e-4
    e      9.39e-8 | 1.20e-7      3.60e-7 | 5.85e-5
    quad   1.82e-8 | 1.82e-8      8.80e-8 | 1.19e-7
    nan    6.73e-8 | 4.67e-8      1.77e-7 | 2.02e-7
    f      IMX686 3-D 1.05e-7 | 1.05e-7, 2.67e-7 | 4.55e-7;  4-D 8.49e-8 | 1.02e-7, 2.39e-7 | 2.82e-7;
           SonyA7S2 3-D 9.30e-8 | 9.05e-8, 2.90e-7 | 1.38e-5;  4-D 6.65e-8 | 1.12e-7, 2.74e-7 | 2.37e-6
Round trip 5.845e-3, the reference's own figure (its 8-bit step)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import _unprocess_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'unprocess.npz')))


@pytest.fixture(scope='module')
def meta():
    return json.load(open(os.path.join(HERE, 'golden', 'unprocess.json')))['cases']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def case_rows(gold, tag):
    from pnnp_amd import unprocess as U
    g = gold[tag + '_g']
    rows = U.unprocess_rows(gold[tag + '_m'], g[:, 0], g[:, 1], g[:, 2], len(g))
    assert np.array_equal(rows[:, 9:12].cpu().numpy().view(np.uint32), gold[tag + '_gains'].view(np.uint32))
    return rows


def some_rows(n, seed=0):
    from pnnp_amd import unprocess as U
    rng = np.random.RandomState(seed)
    m = np.stack([R.CCMS['IMX686'] * np.float32(1 + 0.03 * i) for i in range(n)]).astype(np.float32)
    return U.unprocess_rows(m, 1 + 0.4 * rng.rand(n), 1.5 + rng.rand(n), 1.4 + rng.rand(n), n)


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e', 'quad', 'nan'])
def test_golden_cases(gold, meta, tag):
    from pnnp_amd import unprocess as U
    x = gold[tag + '_x']
    xd, rows = dev(x), case_rows(gold, tag)
    keep = xd.clone()
    rgb, packed = U.unprocess_batch(xd, rows, rgb=True, packed='RGGB')
    assert rgb.shape == x.shape and rgb.dtype == torch.float32 and rgb.is_cuda and packed.shape == (x.shape[0], 4, x.shape[1] // 2, x.shape[2] // 2)
    assert torch.equal(xd.view(torch.int32), keep.view(torch.int32))                # the input is not modified
    want = R.batch_f64(x, gold[tag + '_m'], gold[tag + '_gains'])
    R.assert_within(rgb.cpu().numpy(), want, meta[tag]['E_abs'], meta[tag]['E_rel'], tag)
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), R.packed(rgb.cpu().numpy()).view(np.uint32))
    again = U.unprocess_batch(xd, rows, rgb=True, packed='RGGB')                    # bitwise repeatable
    assert torch.equal(again[0].view(torch.int32), rgb.view(torch.int32)) and torch.equal(again[1].view(torch.int32), packed.view(torch.int32))
    if tag == 'nan':                                                                # one NaN channel: the pixel's three channels, nothing else
        bad = torch.isnan(rgb).cpu().numpy()
        assert bad.sum() == 3 and bad[0, 1, 5].all()
    if tag == 'd':                                                                  # below x ~ 6e-8 the reference sits on its floor; the kernel does not
        tiny = rgb.cpu().numpy()[0, 0, 12:16]                                       # x = 1e-9
        assert (tiny > 100 * gold['d_ref'][0, 0, 12:16]).all()


# W / 2 = 1, 33, 65 (element path, W = 2 mod 4), the vector path (W % 4 == 0), one quad, a single row pair, more than one workgroup
SHAPES = [(1, 2, 2), (2, 4, 2), (1, 6, 66), (1, 4, 130), (1, 2, 8), (3, 6, 12), (1, 64, 100), (2, 10, 132)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_input_kinds_patterns_and_paths(shape):
    from pnnp_amd import unprocess as U
    B, H, W = shape
    rng = np.random.RandomState(sum(shape))
    u8 = rng.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    u8[0, 0, 0] = (0, 255, 128)
    x = (torch.from_numpy(u8).float() / 255).numpy()                                # the division on the CPU: the device's `/ scalar` multiplies by the reciprocal
    x2 = (rng.rand(B, H, W, 3) * 1.3 - 0.1).astype(np.float32)
    rows = some_rows(B, seed=H)
    for data in (x, x2):
        xd = dev(data)
        rgb, rggb = U.unprocess_batch(xd, rows, rgb=True, packed='RGGB')
        _, gbrg = U.unprocess_batch(xd, rows, rgb=True, packed='GBRG')
        host = rgb.cpu().numpy()
        assert not np.isnan(host).any() and host.min() >= 0 and host.max() <= 1
        # the packed planes are bitwise the gathers of the RGB output of the same launch, in both patterns and plane orders
        assert np.array_equal(rggb.cpu().numpy().view(np.uint32), R.packed(host).view(np.uint32))
        assert np.array_equal(gbrg.cpu().numpy().view(np.uint32), R.packed(host, gbrg=True).view(np.uint32))
        # packed only (the gain on the Bayer channel alone) is the same bits
        for pat, both in (('RGGB', rggb), ('GBRG', gbrg)):
            none, only = U.unprocess_batch(xd, rows, rgb=False, packed=pat)
            assert none is None and torch.equal(only.view(torch.int32), both.view(torch.int32))
        # planes in, planes out: bitwise the channel-last result
        chw, pk = U.unprocess_batch(xd.permute(0, 3, 1, 2).contiguous(), rows, layout='chw', rgb=True, packed='RGGB')
        assert chw.shape == (B, 3, H, W) and torch.equal(chw.permute(0, 2, 3, 1).contiguous().view(torch.int32), rgb.view(torch.int32))
        assert torch.equal(pk.view(torch.int32), rggb.view(torch.int32))
        assert torch.equal(U.unprocess_batch(xd.permute(0, 3, 1, 2).contiguous(), rows, layout='chw', rgb=False, packed='GBRG')[1].view(torch.int32),
                           gbrg.view(torch.int32))
        # a pointwise map: a crop of the result is the result of the crop (other row starts, other paths, other lanes)
        if W >= 8:
            part = U.unprocess_batch(xd[:, :H - 2 if H > 2 else H, 2:W - 2].contiguous(), rows, rgb=True)[0]
            assert torch.equal(part.view(torch.int32), rgb[:, :H - 2 if H > 2 else H, 2:W - 2].contiguous().view(torch.int32))
        # every image with its own row: the batch is the single launches
        for i in range(B):
            one = U.unprocess_batch(xd[i:i + 1], rows[i:i + 1].contiguous(), rgb=True, packed='GBRG')
            assert torch.equal(one[0].view(torch.int32), rgb[i:i + 1].view(torch.int32)) and torch.equal(one[1].view(torch.int32), gbrg[i:i + 1].view(torch.int32))
    # 8-bit in (an extension): bitwise the float32 path fed v / 255
    f_rgb, f_pk = U.unprocess_batch(dev(x), rows, rgb=True, packed='RGGB')
    b_rgb, b_pk = U.unprocess_batch(dev(u8), rows, rgb=True, packed='RGGB')
    assert b_rgb.dtype == torch.float32 and torch.equal(b_rgb.view(torch.int32), f_rgb.view(torch.int32)) and torch.equal(b_pk.view(torch.int32), f_pk.view(torch.int32))
    assert torch.equal(U.unprocess_batch(dev(u8), rows, rgb=False, packed='GBRG')[1].view(torch.int32),
                       U.unprocess_batch(dev(x), rows, rgb=False, packed='GBRG')[1].view(torch.int32))
    # an odd size has no packed output but has an RGB one
    if W >= 8:
        odd = U.unprocess_batch(dev(x2)[:, :H - 1, :W - 3].contiguous(), rows, rgb=True)[0]
        full = U.unprocess_batch(dev(x2), rows, rgb=True)[0]
        assert torch.equal(odd.view(torch.int32), full[:, :H - 1, :W - 3].contiguous().view(torch.int32))


def test_three_rows_are_three_parameter_sets(gold):
    """case b's three images under each other's rows differ: the row of the image is the one applied"""
    from pnnp_amd import unprocess as U
    xd, rows = dev(gold['b_x']), case_rows(gold, 'b')
    out = U.unprocess_batch(xd, rows)[0]
    swapped = U.unprocess_batch(xd, rows[[1, 2, 0]].contiguous())[0]
    for i in range(3):
        assert not torch.equal(out[i], swapped[i])
        alone = U.unprocess_batch(xd[i:i + 1], rows[i:i + 1].contiguous())[0]
        assert torch.equal(alone[0].view(torch.int32), out[i].view(torch.int32))


def test_grid_stride_loop_beyond_the_grid_cap():
    """2 x 1032 x 1028 pixels are 530 448 lane items, more than the 2048 x 256 a capped grid covers in one pass: bitwise the two images alone"""
    from pnnp_amd import unprocess as U
    g = torch.Generator(device='cuda').manual_seed(4)
    u8 = torch.randint(0, 256, (2, 1032, 1028, 3), device='cuda', generator=g, dtype=torch.uint8)
    rows = some_rows(2)
    both = U.unprocess_batch(u8, rows, rgb=False, packed='RGGB')[1]
    for i in range(2):
        alone = U.unprocess_batch(u8[i:i + 1], rows[i:i + 1].contiguous(), rgb=False, packed='RGGB')[1]
        assert torch.equal(alone.view(torch.int32), both[i:i + 1].view(torch.int32))
    assert float(both.min()) >= 0 and float(both.max()) <= 1 and float(both.std()) > 0.05


def test_offsets_past_2_to_the_31():
    """3 x 16384 x 16384 x 3 bytes are 2.4 GB: the last image's input bytes straddle offset 2^31 and the packed output ends past 2^31 bytes;
    its planes are bitwise those of the image alone (whose offsets are small)"""
    from pnnp_amd import unprocess as U
    g = torch.Generator(device='cuda').manual_seed(6)
    u8 = torch.randint(0, 256, (3, 16384, 16384, 3), device='cuda', generator=g, dtype=torch.uint8)
    assert u8.numel() > 1 << 31
    rows = some_rows(3)
    both = U.unprocess_batch(u8, rows, rgb=False, packed='GBRG')[1]
    alone = U.unprocess_batch(u8[2:3], rows[2:3].contiguous(), rgb=False, packed='GBRG')[1]
    assert torch.equal(alone.view(torch.int32), both[2:3].view(torch.int32))
    # ... and hold the gather of the small RGB launch of a corner that lies past the offset
    corner = U.unprocess_batch(u8[2:3, 16000:, 16000:].contiguous(), rows[2:3].contiguous(), rgb=True)[0]
    assert np.array_equal(both[2:3, :, 8000:, 8000:].cpu().numpy().view(np.uint32), R.packed(corner.cpu().numpy(), gbrg=True).view(np.uint32))


def test_alignment_and_refusals_at_the_c_entry():
    from pnnp_amd import _lib, unprocess as U
    rng = np.random.RandomState(3)
    x = dev((rng.rand(1, 8, 12, 3) * 1.3 - 0.1).astype(np.float32))
    rows = some_rows(1)
    want_rgb, want_pk = U.unprocess_batch(x, rows, rgb=True, packed='RGGB')
    # contiguous, W % 4 == 0, but the storage starts 4 bytes off a 16-byte boundary: element accesses, same bits
    flat = torch.empty(x.numel() + 1, device='cuda')
    off = flat[1:].view(1, 8, 12, 3)
    off.copy_(x)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    got_rgb, got_pk = U.unprocess_batch(off, rows, rgb=True, packed='RGGB')
    assert torch.equal(got_rgb.view(torch.int32), want_rgb.view(torch.int32)) and torch.equal(got_pk.view(torch.int32), want_pk.view(torch.int32))
    entry = _lib.lib().pnnp_unprocess_f32
    out, pk = torch.empty_like(x), torch.empty(1, 4, 4, 6, device='cuda')
    call = lambda p, kind, H, W, r, flags, o, q: entry(C.c_void_p(p), kind, 1, H, W, C.c_void_p(r), C.c_uint(flags), C.c_void_p(o), C.c_void_p(q), _lib.stream())
    P, Rw, O, Q = x.data_ptr(), rows.data_ptr(), out.data_ptr(), pk.data_ptr()
    assert call(P, 0, 8, 12, Rw, 0, O, Q) == 0 and torch.equal(out.view(torch.int32), want_rgb.view(torch.int32))
    assert call(P, 0, 7, 12, Rw, 0, O, Q) == -1 and call(P, 0, 8, 11, Rw, 0, O, Q) == -1            # odd H / W with a packed output
    assert call(P, 0, 7, 11, Rw, 0, O, 0) == 0                                                       # ... fine without one
    assert call(P + 2, 0, 8, 12, Rw, 0, O, Q) == -1 and call(P, 0, 8, 12, Rw, 0, O + 2, Q) == -1     # float arrays off a 4-byte boundary
    assert call(P, 0, 8, 12, Rw, 0, O, Q + 1) == -1 and call(P, 0, 8, 12, Rw + 2, 0, O, Q) == -1
    assert call(P, 3, 8, 12, Rw, 0, O, Q) == -1 and call(P, 0, 8, 12, Rw, 2, O, Q) == -1             # unknown kind / flag
    assert call(P, 0, 8, 12, Rw, 0, 0, 0) == -1 and call(0, 0, 8, 12, Rw, 0, O, Q) == -1 and call(P, 0, 8, 12, 0, 0, O, Q) == -1
    assert call(P, 0, 0, 12, Rw, 0, O, Q) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize('cam', ['IMX686', 'SonyA7S2'])
def test_unprocess_seeded_like_the_reference(gold, meta, cam):
    from pnnp_amd import unprocess as U
    for kind in ('3d', '4d'):
        key = f'f_{cam}_{kind}'
        x = gold[key + '_x']
        gains = R.gains_f32(gold[key + '_rgb_gain'], gold[key + '_red_gain'], gold[key + '_blue_gain'])
        want = R.batch_f64(x.reshape((-1,) + x.shape[-3:]), R.CCMS[cam], gains).reshape(x.shape)
        outs = []
        for on_device in (True, False):
            torch.manual_seed(11); np.random.seed(13)
            out, md = U.unprocess(dev(x) if on_device else torch.from_numpy(x), camera_type=cam, use_gpu=on_device)
            assert out.is_cuda == on_device and out.shape == x.shape and out.dtype == torch.float32
            assert set(md) == {'cam2rgb', 'rgb_gain', 'red_gain', 'blue_gain'}
            for k, v in md.items():
                assert v.is_cuda == on_device and np.array_equal(v.cpu().numpy().view(np.uint32), gold[f'{key}_{k}'].view(np.uint32)), k
            assert np.array_equal(torch.get_rng_state().numpy(), gold[key + '_torch_state']) and np.random.get_state()[2] == int(gold[key + '_np_pos'])
            R.assert_within(out.cpu().numpy(), want, meta[key]['E_abs'], meta[key]['E_rel'], f'{key} device={on_device}')
            outs.append(out.cpu())
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # locked gains and the identity matrix: case e through the function
    out, md = U.unprocess(dev(gold['e_x'][0]), lock_wb=([1.], [2.1], [1.7]), camera_type='SonyA7S2')
    assert not md['red_gain'].is_cuda and md['red_gain'].tolist() == [float(np.float32(2.1))]
    R.assert_within(out.cpu().numpy()[None], R.batch_f64(gold['e_x'], gold['e_m'], gold['e_gains']), meta['e']['E_abs'], meta['e']['E_rel'], 'e via unprocess')
    u8 = torch.randint(0, 256, (4, 6, 3), dtype=torch.uint8)
    a, _ = U.unprocess(u8.cuda(), lock_wb=([1.], [2.1], [1.7]))
    b, _ = U.unprocess((u8.float() / 255).cuda(), lock_wb=([1.], [2.1], [1.7]))
    assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_mosaic_bit_exact_on_a_stack(gold):
    from pnnp_amd import unprocess as U
    xd = dev(gold['g_x'])
    for fn, want in ((U.mosaic, gold['g_rggb']), (U.mosaic_GBRG, gold['g_gbrg'])):
        got = fn(xd)
        assert got.is_cuda and got.shape == (2, 2, 3, 4, 4) and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    idx = torch.arange(4 * 6 * 3, dtype=torch.float32).reshape(4, 6, 3).cuda()
    assert np.array_equal(U.mosaic(idx).cpu().numpy(), gold['g_idx_rggb']) and np.array_equal(U.mosaic_GBRG(idx).cpu().numpy(), gold['g_idx_gbrg'])


def test_round_trip_through_the_render_kernel(gold, meta):
    """unprocess -> packed -> process.process with the inverse gains and cam2rgb -> smoothstep on the host returns x as closely as the reference's
    own round trip on the same data (its 8-bit quantisation): 4 x the recorded figure"""
    from pnnp_amd import process as P, unprocess as U
    x = gold['rt_x']
    lock = gold['rt_lock']
    rgb2cam, cam2rgb, rgb_gain, red_gain, blue_gain = U.unprocess_draw(tuple(lock.tolist()), 'IMX686')
    assert np.array_equal(cam2rgb.numpy().view(np.uint32), gold['rt_cam2rgb'].view(np.uint32))
    rows = U.unprocess_rows(rgb2cam, rgb_gain, red_gain, blue_gain, 1)
    rgb, packed = U.unprocess_batch(dev(x[None]), rows, rgb=True, packed='RGGB')
    assert float(rgb.max()) < 1 and float(rgb.min()) > 0                             # no clamp binds
    back = P.process(packed, dev(gold['rt_wb']), dev(gold['rt_cam2rgb'][None])).cpu().numpy()[0].transpose(1, 2, 0).astype(np.float64)
    err = float(np.abs(3 * back ** 2 - 2 * back ** 3 - x[::2, ::2]).max())
    print(f'round trip: {err:.3e} (reference {meta["rt"]["E_roundtrip"]:.3e})')
    assert err <= 4 * meta['rt']['E_roundtrip']


def _tiny_net(seed=3):
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    torch.manual_seed(seed)
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=8, in_nc=4, out_nc=4))
    initialize_weights(net)
    return net.cuda()


@pytest.mark.parametrize('layout', ['hwc', 'chw'])
def test_step_rgb_is_draws_then_unprocess_batch_then_step(layout):
    from pnnp_amd import unprocess as U
    from pnnp_amd.trainer import HipTrainStep
    g = torch.Generator().manual_seed(8)
    rgb = torch.rand(2, 128, 128, 3, generator=g).cuda()
    if layout == 'chw':
        rgb = rgb.permute(0, 3, 1, 2).contiguous()
    results = []
    for fused in (True, False):
        net = _tiny_net()
        ts = HipTrainStep(net, lr=1e-3, camera_type='IMX686', clip=2, seed=5)
        np.random.seed(0); torch.manual_seed(0)
        if fused:
            loss, info = ts.step_rgb(rgb, layout=layout)
        else:
            draws = [U.unprocess_draw(False, 'IMX686') for _ in range(2)]
            rows = U.unprocess_rows(torch.stack([d[0] for d in draws]), *[torch.cat([d[k] for d in draws]) for k in (2, 3, 4)], 2)
            hr = U.unprocess_batch(rgb, rows, layout=layout, rgb=False, packed='RGGB')[1]
            assert hr.shape == (2, 4, 64, 64)
            loss = ts.step(hr)
            # the info tensors in the convention of the reference's metadata: wb = (red, 1, blue), ccm = cam2rgb
            assert set(info) == {'wb', 'ccm', 'rgb_gain'} and info['wb'].shape == (2, 3) and info['ccm'].shape == (2, 3, 3)
            for i, d in enumerate(draws):
                assert info['wb'][i].tolist() == [float(d[3]), 1.0, float(d[4])] and torch.equal(info['ccm'][i], d[1]) and float(info['rgb_gain'][i]) == float(d[2])
            assert float(draws[0][3]) != float(draws[1][3])                          # one draw per crop
        assert ts.step_count == 1 and bool(torch.isfinite(loss).all())
        results.append((loss.clone(), net.engine.params.flat.clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_img_run_file_runs(capsys):
    from pnnp_amd import runfile
    path = os.path.join(HERE, 'fixtures', 'runfile_sony_img.yml')
    assert runfile.main([path, '--synthetic', '--epochs', '1', '--steps', '2', '--patch', '64']) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('Epoch')][-1]
    loss = float(line.split('| loss')[1].split('|')[0])
    assert np.isfinite(loss) and loss > 0, line
