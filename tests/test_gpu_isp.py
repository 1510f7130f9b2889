"""csrc/isp.hip on the device: the reference's own renders (tests/golden/isp.npz) through ``process``, ``raw2rgb_v2``, ``gamma_compression``
and ``preview_strip`` under the agreement rule of tests/_isp_ref.py (equal to the golden, or one level apart where the float64 value before
truncation lies within 1e-4 of an integer; at most 0.5 % of a case may use the exception), the vector / scalar paths against the round-once
restatement, and ``evaluate(render=...)``.

Observed on the MI355X (profiles/r7/isp_render.txt): cases a, b, c, e, gamma_compression, raw2rgb_v2 and both preview strips exactly equal; case d
45 of 48 960 values (0.092 %) one level apart, all inside the rule -- the same 45 in which the reference differs from the round-once float64 power."""
import os

import numpy as np
import pytest
import torch

from tests import _isp_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PWB = [2.13, 1.0, 1.57, 1.0]


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'isp.npz')))


def case_input(gold, tag):
    x = gold[tag + '_x']
    return np.repeat(x, 4, axis=1) if tag == 'd' else x


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e'])
def test_process_golden(gold, tag):
    from pnnp_amd import process as P
    x, wb, ccm, k = case_input(gold, tag), gold[tag + '_wb'], gold[tag + '_ccm'], gold[tag + '_k']
    xd = dev(x)
    keep = xd.clone()
    out = P.process(xd, dev(wb), dev(ccm))
    assert out.shape == (x.shape[0], 3) + x.shape[2:] and out.dtype == torch.float32 and out.is_cuda
    assert torch.equal(xd, keep)                                                    # the input is not modified
    R.assert_agrees(R.to_levels(out.cpu().numpy()), k, R.process_pre(x, wb, ccm), f'process {tag}')
    # both outputs of one launch: the float planes are bitwise uint8 / 255; RGB and BGR orders
    rows = P.isp_rows(wb, ccm, x.shape[0])
    f, u = P.isp_render(xd, rows, f32=True, u8=True)
    assert torch.equal(f, out) and u.shape == (x.shape[0],) + x.shape[2:] + (3,) and u.dtype == torch.uint8
    assert torch.equal(u.cpu().permute(0, 3, 1, 2).float() / 255, f.cpu())          # (on the CPU: the device's `/ scalar` multiplies by the reciprocal)
    _, ub = P.isp_render(xd, rows, f32=False, u8=True, bgr=True)
    assert torch.equal(ub, u.flip(-1))
    assert torch.equal(P.process(xd, dev(wb), dev(ccm)), out)                       # bitwise repeatable


def test_raw2rgb_v2_and_gamma_golden(gold):
    from pnnp_amd import process as P
    x = gold['v2_x']
    pre = R.process_pre(x[None], R.SONY_WB, R.SONY_CCM)[0].transpose(1, 2, 0)
    out = P.raw2rgb_v2(x, R.SONY_WB, R.SONY_CCM)                                    # numpy in -> numpy [H,W,3] float32, like the reference
    assert isinstance(out, np.ndarray) and out.shape == (16, 20, 3) and out.dtype == np.float32
    R.assert_agrees(R.to_levels(out), gold['v2_k'], pre, 'raw2rgb_v2')
    d = P.raw2rgb_v2(dev(x), R.SONY_WB, R.SONY_CCM, device_out=True)
    assert d.is_cuda and np.array_equal(d.cpu().numpy(), out)
    u = P.raw2rgb_v2(dev(x), R.SONY_WB, R.SONY_CCM, device_out=True, u8=True)
    assert u.dtype == torch.uint8 and np.array_equal(u.cpu().numpy(), R.to_levels(out))
    ub = P.raw2rgb_v2(x, R.SONY_WB, R.SONY_CCM, u8=True, bgr=True)
    assert isinstance(ub, np.ndarray) and np.array_equal(ub, u.cpu().numpy()[..., ::-1])
    g = gold['g_x']
    gd = dev(g)
    got = P.gamma_compression(gd)
    assert got.shape == g.shape and np.array_equal(gd.cpu().numpy(), g)
    R.assert_agrees(R.to_levels(got.cpu().numpy()), gold['g_k'], R.pre(g), 'gamma_compression')


@pytest.mark.parametrize('tag,args,add', [('f_sid', ('f_sid_lr', 'f_sid_pred', 'f_sid_hr'), False), ('f_nf', ('f_nf_hr', 'f_nf_sample', 'f_nf_lr'), True)])
def test_preview_strip_golden(gold, tag, args, add):
    from pnnp_amd import process as P
    a = [gold[n] for n in args]
    lin = R.preview_linear(*a, gold['f_wb'], add_inputs_to_output=add)
    t = [dev(v) for v in a]
    got = P.preview_strip(t[0], t[1], t[2], gold['f_wb'], add_inputs_to_output=add)
    assert got.shape == (32, 120, 3) and got.dtype == torch.uint8 and got.is_cuda
    R.assert_agrees(got.cpu().numpy(), gold[tag + '_u8'], R.pre(lin, floor=False), f'preview {tag}')
    batched = P.preview_strip(t[0][None].repeat(2, 1, 1, 1), t[1][None], t[2][None], torch.from_numpy(gold['f_wb']), add_inputs_to_output=add)
    assert torch.equal(batched, got)                                                # [B,4,H,W]: image 0
    for v, orig in zip(t, a):
        assert np.array_equal(v.cpu().numpy(), orig)


def test_preview_strip_scalar_path_and_clip():
    """W % 4 != 0 (element accesses) against the restatement, on data outside [0,1]: always clipped before the power"""
    from pnnp_amd import process as P
    rng = np.random.RandomState(5)
    a = [(rng.rand(4, 5, 7) * 1.6 - 0.3).astype(np.float32) for _ in range(3)]
    for add in (False, True):
        lin = R.preview_linear(*a, PWB, add_inputs_to_output=add)
        got = P.preview_strip(*[dev(v) for v in a], PWB, add_inputs_to_output=add).cpu().numpy()
        assert got.shape == (5, 21, 3)
        R.assert_agrees(got, R.levels_once(lin, floor=False), R.pre(lin, floor=False), f'preview 5x7 add={add}')


# vector path (W % 4 == 0), the tail, rows that start off a 16-byte boundary, more than one workgroup, one long row
SHAPES = [(1, 4, 1, 4), (1, 4, 3, 5), (2, 4, 5, 7), (1, 4, 8, 12), (1, 4, 64, 100), (1, 4, 1, 2128)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shapes_and_per_image_parameters(shape):
    from pnnp_amd import process as P
    rng = np.random.RandomState(sum(shape))
    N = shape[0]
    x = (rng.rand(*shape) * 1.4 - 0.1).astype(np.float32)
    wb = (np.array([PWB] * N) * (1 + 0.1 * rng.rand(N, 4))).astype(np.float32)     # [N,4]: every image its own gains (extension)
    ccm = np.stack([R.SONY_CCM * np.float32(1 + 0.05 * i) for i in range(N)]).astype(np.float32)
    want, pre = R.process_levels(x, wb, ccm, once=True), R.process_pre(x, wb, ccm)
    xd = dev(x)
    f, u = P.isp_render(xd, P.isp_rows(wb, ccm, N), f32=True, u8=True)
    # against the round-once restatement the kernel restates: equal, or excused by the same rule
    R.assert_agrees(R.to_levels(f.cpu().numpy()), want, pre, f'shape {shape}')
    assert torch.equal(u.cpu().permute(0, 3, 1, 2).float() / 255, f.cpu())          # (on the CPU: the device's `/ scalar` multiplies by the reciprocal)
    assert torch.equal(P.process(xd, dev(wb), dev(ccm)), f)
    if N > 1:                                                                       # image 1 alone, with its own row, is image 1 of the batch
        assert torch.equal(P.process(xd[1:], dev(wb[1:]), dev(ccm[1:])), f[1:])


def test_non_contiguous_input_is_made_contiguous():
    from pnnp_amd import process as P
    rng = np.random.RandomState(9)
    big = dev((rng.rand(1, 4, 16, 24) * 1.4 - 0.1).astype(np.float32))
    view = big[:, :, ::2, 1:21]                                                     # strided rows, offset columns
    assert not view.is_contiguous()
    wb, ccm = dev(R.SONY_WB[None]), dev(R.SONY_CCM[None])
    assert torch.equal(P.process(view, wb, ccm), P.process(view.contiguous(), wb, ccm))
    chan_last = big.contiguous(memory_format=torch.channels_last)
    assert torch.equal(P.process(chan_last, wb, ccm), P.process(big, wb, ccm))
    # contiguous, W % 4 == 0, but the storage starts 4 bytes off a 16-byte boundary: element accesses, same result
    flat = torch.empty(4 * 8 * 12 + 1, device='cuda')
    off = flat[1:].view(1, 4, 8, 12)
    off.copy_(big[:, :, :8, :12])
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    assert torch.equal(P.process(off, wb, ccm), P.process(off.clone(), wb, ccm))


def test_process_against_the_on_device_composition():
    """apply_gains / raw2LRGB / apply_ccms / torch gamma as torch ops on the device, against the kernel, under the agreement rule"""
    from pnnp_amd import process as P
    rng = np.random.RandomState(11)
    x = (rng.rand(2, 4, 32, 48) * 1.4 - 0.1).astype(np.float32)
    xd, wb, ccm = dev(x), dev(R.SONY_WB[None]), dev(np.stack([R.SONY_CCM, R.SONY_CCM.T.copy()]))
    v = torch.clamp(P.apply_gains(xd, wb), min=0.0, max=1.0)
    v = torch.clamp(P.apply_ccms(P.raw2LRGB(v), ccm), min=0.0, max=1.0)
    comp = torch.clamp((torch.clamp(v, min=1e-8) ** (1 / 2.2) * 255).int(), min=0, max=255)
    got = P.process(xd, wb, ccm)
    pre = R.process_pre(x, R.SONY_WB, ccm.cpu().numpy())
    R.assert_agrees(R.to_levels(got.cpu().numpy()), comp.cpu().numpy().astype(np.int64), pre, 'process vs composition')


def test_levels_around_every_threshold_equal_the_round_once_power():
    """The kernel takes a float32 estimate of the power and the float64 power only where the estimate lies within 2e-3 of an integer.  Around every
    threshold k = 1..255, values whose scaled power s = 255 v^(1/2.2) lies at k + d for 512 offsets d spread over +-8e-3 (inside the margin, at
    it and up to four times beyond it, both sides), plus 1, 2 and 3 ulp on either side of the threshold itself: every level equals the
    round-once float64 power's, exactly.  The float32 CPU power may differ by one level under the rule."""
    from pnnp_amd import process as P
    d = np.linspace(-8e-3, 8e-3, 506)
    k = np.arange(1, 256, dtype=np.float64)
    v = (((k[:, None] + d[None, :]) / 255.0) ** 2.2).astype(np.float32)
    thr = ((k / 255.0) ** 2.2).astype(np.float32)
    near = np.stack([(thr.view(np.int32) + o).view(np.float32) for o in (-3, -2, -1, 1, 2, 3)], axis=1)
    v = np.concatenate([v, near], axis=1)                                           # 255 x 512
    assert v.shape == (255, 512)
    x = np.broadcast_to(v, (1, 3, 255, 512)).copy()
    got = R.to_levels(P.gamma_compression(dev(x)).cpu().numpy())
    want = R.levels_once(x)
    assert set(np.unique(want)) == set(range(0, 256))
    assert np.array_equal(got, want), f'{int((got != want).sum())} levels differ from the round-once power'
    R.assert_agrees(got, R.levels(x), R.pre(x), 'thresholds vs the float32 CPU power')


def test_nan_renders_as_zero():
    from pnnp_amd import process as P
    x = torch.full((1, 4, 2, 4), 0.5, device='cuda')
    x[0, 1, 0, 1] = float('nan')
    f, u = P.isp_render(x, P.isp_rows(R.SONY_WB, R.SONY_CCM, 1), f32=True, u8=True)
    assert (u[0, 0, 1] == 0).all() and (f[0, :, 0, 1] == 0).all() and (u[0, 1] > 0).all()


class _Net(torch.nn.Module):
    res = False

    def forward(self, x):
        return x * 0.9 + 0.01


def test_evaluate_render():
    from pnnp_amd import process as P
    from pnnp_amd.evaluate import EvalLoop, evaluate
    from pnnp_amd.metrics import quality_assess
    g = torch.Generator().manual_seed(3)
    hr = (torch.rand(1, 4, 32, 48, generator=g) ** 2.2).cuda()
    lr = (hr + 0.05 * torch.randn(1, 4, 32, 48, generator=g).cuda())
    net = _Net().cuda()
    render = dict(wb=R.SONY_WB, ccm=R.SONY_CCM)
    plain = evaluate(net, lr, hr)
    out = evaluate(net, lr, hr, render=render)
    assert set(plain) == {'dn', 'lr', 'metrics'} and set(out) == {'dn', 'lr', 'metrics', 'rgb', 'metrics_rgb'}
    assert torch.equal(out['dn'], plain['dn']) and torch.equal(out['lr'], plain['lr'])
    assert torch.equal(out['metrics'].view(torch.int32), plain['metrics'].view(torch.int32))
    for k, src in (('dn', out['dn']), ('lr', out['lr']), ('hr', hr)):
        want = P.raw2rgb_v2(src[0], R.SONY_WB, R.SONY_CCM, device_out=True, u8=True)
        assert out['rgb'][k].shape == (32, 48, 3) and torch.equal(out['rgb'][k], want)
    fl = {k: P.process(src, dev(R.SONY_WB[None]), dev(R.SONY_CCM[None])) for k, src in (('dn', out['dn']), ('lr', out['lr']), ('hr', hr))}
    want = torch.cat([quality_assess(fl['dn'], fl['hr']), quality_assess(fl['lr'], fl['hr'])])
    assert torch.equal(out['metrics_rgb'].view(torch.int32), want.view(torch.int32)) and torch.isfinite(want).all()
    bgr = evaluate(net, lr, hr, render=dict(render, bgr=True))
    assert torch.equal(bgr['rgb']['dn'], out['rgb']['dn'].flip(-1))

    loop = EvalLoop(net)
    loop.step('a', lr, hr)
    _, text_plain = loop.finish(epoch=3)
    m = plain['metrics'].tolist()
    assert text_plain == (f"Epoch 3: PSNR={m[0]:.2f}\npsnrs_lr={m[2]:.2f}, psnrs_dn={m[0]:.2f}\nssims_lr={m[3]:.4f}, ssims_dn={m[1]:.4f}")
    loop = EvalLoop(net)
    loop.step('a', lr, hr, render=render)
    loop.step('b', lr, hr)                                                          # a step that does not render does not count in the RGB meters
    _, text = loop.finish(epoch=3)
    r = out['metrics_rgb'].tolist()
    assert text == text_plain + f"\nrgb: psnrs_lr={r[2]:.2f}, psnrs_dn={r[0]:.2f}, ssims_lr={r[3]:.4f}, ssims_dn={r[1]:.4f}"
