"""GPU parity of the eval epilogue (row f1): IlluminanceCorrect vs the reference's golden output,
PSNR/SSIM vs the oracle restatement of the scikit-image definition (parity unpinned: skimage absent); then every kernel of
csrc/evalmetrics.hip against the float64 restatement of tests/_ssim_ref.py, at the shapes, values and switches where it can go wrong."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_illuminance_correct_golden(golden_dir):
    from pnnp_amd.metrics import IlluminanceCorrect
    g = np.load(os.path.join(golden_dir, 'misc.npz'))
    a = torch.from_numpy(g['psnr_a'])
    pred = (a[:1] * 1.3 - 0.1).cuda(); src = torch.from_numpy(g['ic_src']).cuda()
    out = IlluminanceCorrect()(pred, src)
    np.testing.assert_allclose(out.cpu().numpy(), g['ic_out'], rtol=2e-6, atol=1e-7)
    # batch of predictions against one source, like the reference's forward()
    outb = IlluminanceCorrect()(pred.repeat(2, 1, 1, 1), src)
    np.testing.assert_allclose(outb[1].cpu().numpy(), g['ic_out'][0], rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize('shape', [(4, 64, 64), (4, 70, 101), (4, 1424, 2128)])
def test_psnr_ssim_vs_oracle(shape):
    from oracle import metrics_np as M
    from pnnp_amd.metrics import quality_assess
    g = torch.Generator().manual_seed(shape[1])
    t = torch.rand(1, *shape, generator=g) ** 2
    o = (t + 0.03 * torch.randn(1, *shape, generator=g)).clamp(-0.1, 1.1)
    res = quality_assess(o.cuda(), t.cuda()).cpu().numpy()
    X, Y = M.tensor2im(o.numpy()), M.tensor2im(t.numpy())
    assert abs(res[0] - M.psnr(Y, X)) < 1e-3
    assert abs(res[1] - M.ssim(Y, X)) < 2e-5


# ---- the kernels of csrc/evalmetrics.hip against the float64 reference of tests/_ssim_ref.py (pinned by tests/test_host_ssim_ref.py)

def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _qa(o, t):
    from pnnp_amd.metrics import quality_assess
    return quality_assess(_dev(o), _dev(t)).cpu().numpy().astype(np.float64)


def _assert_bars(res, o, t):
    from tests import _ssim_ref as R
    p, s = R.psnr(o, t), R.ssim(o, t)
    print(f'psnr {res[0]:.6f} vs {p:.6f} ({abs(res[0] - p):.2e} dB), ssim {res[1]:.8f} vs {s:.8f} ({abs(res[1] - s):.2e})')
    assert abs(res[0] - p) < R.PSNR_BAR
    assert abs(res[1] - s) < R.SSIM_BAR


@pytest.mark.parametrize('hw', [(7, 7), (7, 40), (40, 7), (8, 9), (32, 32), (33, 33), (35, 35), (38, 38), (39, 39), (64, 65)])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_psnr_ssim_shape_edges_vs_float64(C, hw):
    """The valid-region edge H-3 / W-3 at each position relative to the 32-tile and to its 3-pixel halo; (7, 7) is one window per
    channel.  Another content per channel, both frames leaving [0, 1] (the clip matters)."""
    from tests import _ssim_ref as R
    o, t = R.well_conditioned(C, *hw)
    if hw[0] * hw[1] >= 280:
        assert (t < 0).any() and (o > 1).any()
    _assert_bars(_qa(o, t), o, t)


@pytest.mark.parametrize('idx', range(11))
def test_psnr_ssim_impulse_sweep(idx):
    """a == b but for one pixel of one channel: every window without the pixel is a bitwise-identical pair and scores exactly 1, so the
    mean is set by the <= 49 windows that hold it (tests/test_host_ssim_ref.py: the channel's own mean, scored here by a one-channel launch,
    moves by >= 2.19e-4, 10.9 bars; the two-channel figure by half of that, 5.5 bars at the two corner pixels).  The pixel on both sides of every tile seam, at the halo depth, on the first and last valid
    rows and columns; in channel 0 and in channel 1."""
    from tests import _ssim_ref as R
    pos = R.impulse_positions()[idx]
    for ch in (0, 1):
        a, b = R.impulse(pos, ch)
        res = _qa(a, b)
        _assert_bars(res, a, b)
        # channel weighting: the untouched channel counts 1, the other one what it scores alone
        s_ref = R.ssim_channels(a, b)
        assert s_ref[1 - ch] == 1.0
        assert abs(res[1] - (s_ref[ch] + (R.IMPULSE_SHAPE[0] - 1)) / R.IMPULSE_SHAPE[0]) < R.SSIM_BAR
        alone = _qa(a[ch:ch + 1], b[ch:ch + 1])
        _assert_bars(alone, a[ch:ch + 1], b[ch:ch + 1])              # the channel's own mean: a corner pixel's one window is 10.9 bars here
        assert abs(res[1] - (alone[1] + 1.0) / 2.0) <= 2.0 ** -23                      # two float32 results, each rounded once
        assert abs(res[0] - (alone[0] + 10.0 * np.log10(2.0))) < 1e-5                  # the same squared error over twice the elements


def _device_windows(o, t):
    from pnnp_amd.metrics import quality_assess
    od, td = _dev(o), _dev(t)
    return torch.stack([quality_assess(od[i], td[i]) for i in range(od.shape[0])]).cpu().numpy().astype(np.float64)[:, 1]


def test_ssim_per_window_conditioning():
    """One 7x7 window per launch, 200 draws per family: on a bright flat window the float32 variances sxx/49 - ux^2 cancel (65025-scale
    terms against C2 = 58.5), which the mean over a frame hides.  The bar is measured per family on the same draws: e_ref = max |oracle -
    float64| (oracle/metrics_np.ssim's per-window value: filter sums in float64, rounded once to float32), and the device must stay
    within 4 e_ref -- the kernel sums 49 float32 terms, which a CPU emulation puts at 1.7 - 2.4 e_ref; the rest is room for the
    compiler's contraction choices.

    Measured on an MI355X, max |device - float64| / e_ref (device, e_ref), equal to a float32 numpy emulation of the kernel's order:
        (0.95, 0.002)   2.09  (3.705e-4, 1.769e-4)
        (0.98, 0.0005)  1.88  (3.555e-4, 1.887e-4)
        (0.5,  0.005)   2.26  (1.023e-4, 4.518e-5)
        (0.2,  0.03)    1.51  (9.278e-6, 6.160e-6)
    (with floating-point contraction left on in the kernel: 1.82, 1.95, 2.09, 1.58)"""
    from tests import _ssim_ref as R
    worst = []
    for level, sigma in R.FLAT_FAMILIES + (R.DARK_FAMILY,):
        o, t = R.flat_family(level, sigma)
        ref, orc = R.window_errors(o, t)
        e_ref = np.abs(orc - ref).max()
        e_dev = np.abs(_device_windows(o, t) - ref).max()
        print(f'family ({level}, {sigma}): e_ref {e_ref:.3e}, device {e_dev:.3e}, ratio {e_dev / e_ref:.2f}')
        worst.append((level, sigma, e_dev, e_ref))
    for level, sigma, e_dev, e_ref in worst:
        assert e_dev <= 4.0 * e_ref, (level, sigma, e_dev, e_ref)


def test_ssim_bright_flat_frame_vs_float64():
    from tests import _ssim_ref as R
    o, t = R.flat_family(0.95, 0.002, shape=(4, 70, 101))
    _assert_bars(_qa(o, t), o, t)


@pytest.mark.parametrize('family', ['noisy', 'bright_flat', 'constant'])
def test_identical_images_give_inf_and_exactly_one(family):
    """bitwise-equal inputs: the squared error is 0 and every window has A1 == B1 and A2 == B2"""
    from tests import _ssim_ref as R
    a = {'noisy': lambda: R.well_conditioned(3, 39, 70)[0], 'bright_flat': lambda: R.flat_family(0.95, 0.002, shape=(4, 40, 70))[0],
         'constant': lambda: np.full((2, 33, 35), 0.4, np.float32)}[family]()
    res = _qa(a, a.copy())
    assert res[0] == np.inf and res[1] == 1.0, res
    assert R.psnr(a, a) == np.inf and R.ssim(a, a) == 1.0


def test_one_nan_pixel_gives_nan_metrics():
    from tests import _ssim_ref as R
    o, t = R.well_conditioned(3, 40, 70)
    for bad_in_output in (True, False):
        o2, t2 = o.copy(), t.copy()
        (o2 if bad_in_output else t2)[1, 20, 33] = np.nan
        res = _qa(o2, t2)
        assert np.isnan(res).all(), res
        assert np.isnan(R.psnr(o2, t2)) and np.isnan(R.ssim(o2, t2))


def test_infinities_clip_like_tensor2im():
    from tests import _ssim_ref as R
    o, t = R.well_conditioned(3, 40, 70)
    o[0, 5, 6] = np.inf; o[1, 34, 66] = -np.inf; t[2, 31, 32] = np.inf; t[0, 0, 0] = -np.inf
    res = _qa(o, t)
    assert np.isfinite(res).all()
    _assert_bars(res, o, t)
    _assert_bars(res, np.nan_to_num(o, posinf=1.0, neginf=0.0), np.nan_to_num(t, posinf=1.0, neginf=0.0))


def test_quality_assess_wrapper():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.metrics import quality_assess
    from tests import _ssim_ref as R
    o, t = R.well_conditioned(3, 33, 40)
    od, td = _dev(o), _dev(t)
    base = quality_assess(od, td)
    _assert_bars(base.cpu().numpy().astype(np.float64), o, t)
    assert torch.equal(quality_assess(od[None], td[None]), base)                    # [1,C,H,W] and [C,H,W]
    assert torch.equal(quality_assess(od[None], td), base)
    # a permuted (non-contiguous) view and its contiguous copy
    ov, tv = od.permute(0, 2, 1), td.permute(0, 2, 1)
    assert not ov.is_contiguous()
    res_v = quality_assess(ov, tv)
    assert torch.equal(res_v, quality_assess(ov.contiguous(), tv.contiguous()))
    _assert_bars(res_v.cpu().numpy().astype(np.float64), o.transpose(0, 2, 1), t.transpose(0, 2, 1))
    # float16 inputs are their .float()
    oh, th = od.half(), td.half()
    assert torch.equal(quality_assess(oh, th), quality_assess(oh.float(), th.float()))
    # below one window: an error, not a number
    for shape in ((3, 6, 40), (3, 40, 6), (1, 6, 6)):
        z = torch.zeros(shape, device='cuda')
        with pytest.raises(PnnpError):
            quality_assess(z, z)


@pytest.mark.parametrize('shape', [(4, 64, 65), (4, 70, 101)])
def test_psnr_ssim_is_bitwise_reproducible(shape):
    """'All reductions are two-stage with a fixed order': the same data, the same bits"""
    from pnnp_amd.metrics import quality_assess
    from tests import _ssim_ref as R
    o, t = R.well_conditioned(*shape)
    od, td = _dev(o), _dev(t)
    first = quality_assess(od, td)
    for _ in range(3):
        assert torch.equal(quality_assess(od, td), first)
    assert torch.equal(quality_assess(od.clone(), td.clone()), first)


def _illum_check(out, pred, src):
    """rtol 3e-7, atol 0: scale = (float)num / (float)den with float64 sums, then one product -- four float32 roundings, 4 x 2^-24 =
    2.4e-7.  An element clamped to 0 is exactly 0."""
    from tests import _ssim_ref as R
    ref = R.illuminance_correct(pred, src)
    out = out.astype(np.float64)
    zero = pred <= 0
    assert np.isfinite(ref).all() and (ref[~zero] > 0).all()
    assert (out[zero] == 0).all()
    rel = np.abs(out[~zero] / ref[~zero] - 1.0).max() if (~zero).any() else 0.0
    print(f'illuminance n = {pred.size}: max relative error {rel:.2e}')
    assert rel <= 3e-7


@pytest.mark.parametrize('n', [1, 255, 256, 257, 65535, 65536, 65537])
def test_illuminance_correct_element_counts_vs_float64(n):
    """either side of one block (256) and of the 256 x 256 threads of the partial grid, where the grid-stride loop takes a second turn"""
    from pnnp_amd.metrics import IlluminanceCorrect
    from tests import _ssim_ref as R
    pred, src = R.illum_inputs((1, 1, 1, n))
    if n == 1:
        pred[...] = 0.7; src[...] = 0.35
    else:
        assert abs((src == 1).mean() - 0.3) < 0.08 and (pred < 0).any() and (pred > 1).any()
    out = IlluminanceCorrect()(_dev(pred), _dev(src))
    assert out.shape == pred.shape and out.dtype == torch.float32
    _illum_check(out.cpu().numpy()[0], pred[0], src[0])


def test_illuminance_correct_frame_vs_float64_and_the_mask():
    from pnnp_amd.metrics import IlluminanceCorrect
    from tests import _ssim_ref as R
    pred, src = R.illum_inputs((1, 4, 70, 101))
    assert abs((src == 1).mean() - 0.3) < 0.02
    out = IlluminanceCorrect()(_dev(pred), _dev(src)).cpu().numpy()
    _illum_check(out[0], pred[0], src[0])
    # the mask is exercised: the unmasked scale is percents away
    p = np.clip(pred, 0, 1).astype(np.float64)
    unmasked = (p * src).sum() / (p * p).sum() * p
    assert np.abs(unmasked[pred > 0] / out[pred > 0] - 1).min() > 1e-2
    # a NaN under the mask (src == 1) stays where it is; one outside it reaches every element
    i_masked = tuple(np.argwhere(src == 1)[5]); i_open = tuple(np.argwhere(src != 1)[5])
    pm = pred.copy(); pm[i_masked] = np.nan
    om = IlluminanceCorrect()(_dev(pm), _dev(src)).cpu().numpy()
    assert np.isnan(om[i_masked]) and np.isnan(om).sum() == 1
    assert np.array_equal(np.delete(om.ravel(), np.ravel_multi_index(i_masked, pred.shape)), np.delete(out.ravel(), np.ravel_multi_index(i_masked, pred.shape)))
    po = pred.copy(); po[i_open] = np.nan
    assert np.isnan(IlluminanceCorrect()(_dev(po), _dev(src)).cpu().numpy()).all()


def test_illuminance_correct_degenerate_inputs_give_nan():
    """den == 0 is 0 / 0, as in torch"""
    from pnnp_amd.metrics import IlluminanceCorrect
    from tests import _ssim_ref as R
    pred, src = R.illum_inputs((1, 2, 20, 33))
    assert np.isnan(IlluminanceCorrect()(_dev(pred), _dev(np.ones_like(src))).cpu().numpy()).all()           # nothing outside the mask
    dark = -np.abs(pred); dark[0, 0, 0, 0] = 0.0
    assert np.isnan(IlluminanceCorrect()(_dev(dark), _dev(src)).cpu().numpy()).all()                          # pred all <= 0
    with np.errstate(all='ignore'):
        assert np.isnan(R.illuminance_correct(dark[0], src[0])).all()


def test_illuminance_correct_batches_and_repeats_are_bitwise():
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.metrics import IlluminanceCorrect
    from tests import _ssim_ref as R
    pred, src = R.illum_inputs((3, 4, 20, 33))
    pd, sd = _dev(pred), _dev(src)
    ic = IlluminanceCorrect()
    assert not np.array_equal(pred[0], pred[1]) and not np.array_equal(src[0], src[1])
    per = ic(pd, sd)                                                                  # 3 predictions, 3 sources
    one = ic(pd, sd[1:2])                                                             # 3 predictions, one source
    for i in range(3):
        assert torch.equal(per[i], ic(pd[i:i + 1], sd[i:i + 1])[0])
        assert torch.equal(one[i], ic(pd[i:i + 1], sd[1:2])[0])
        _illum_check(per[i].cpu().numpy(), pred[i], src[i])
        _illum_check(one[i].cpu().numpy(), pred[i], src[1])
    assert not torch.equal(per[0], one[0])
    for _ in range(3):
        assert torch.equal(ic(pd, sd), per)
    assert torch.equal(ic.correct(pd[:1], sd[:1]), per[:1])
    for shape in ((1, 1, 1, 0), (0, 4, 8, 8)):
        e = torch.empty(shape, device='cuda')
        with pytest.raises(PnnpError):
            ic(e, e)


@pytest.fixture(scope='module')
def small_eval():
    """the nf = 8 net and the 56 x 72 frame of test_gpu_eval_pipeline.py (72 % 16 = 8: the padded branch)"""
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    torch.manual_seed(4)
    net = UNetSeeInDark(dict(nframes=1, res=True, nf=8, in_nc=4, out_nc=4)); initialize_weights(net); net = net.cuda().eval()
    g = torch.Generator(device='cuda').manual_seed(5)
    hr = torch.rand(1, 4, 56, 72, device='cuda', generator=g)
    lr = hr / 5.0 + torch.randn(1, 4, 56, 72, device='cuda', generator=g) * 0.02
    return net, lr, hr


def test_evaluate_switches(small_eval):
    from pnnp_amd.evaluate import evaluate
    from pnnp_amd.metrics import IlluminanceCorrect, quality_assess
    net, lr, hr = small_eval
    kw = dict(ratio=5.0, ori=True)
    full = evaluate(net, lr, hr, **kw)
    plain = evaluate(net, lr, hr, brightness_correct=False, **kw)
    assert torch.isfinite(full['metrics']).all() and not torch.equal(full['dn'], plain['dn'])
    assert torch.equal(full['dn'], IlluminanceCorrect()(plain['dn'], hr))
    assert torch.equal(full['metrics'], torch.cat([quality_assess(full['dn'], hr), quality_assess(full['lr'], hr)]))
    # with_lr=False: the noisy frame is not scored, the denoised one is as before
    no_lr = evaluate(net, lr, hr, with_lr=False, **kw)
    assert torch.isnan(no_lr['metrics'][2:]).all() and torch.equal(no_lr['metrics'][:2], full['metrics'][:2])
    assert torch.equal(no_lr['lr'], full['lr'])
    # epoch >= 0 (validation while training): no correction
    ep0 = evaluate(net, lr, hr, epoch=0, **kw)
    assert torch.equal(ep0['dn'], plain['dn']) and torch.equal(ep0['metrics'], plain['metrics'])
    # a corrector that is passed in is the one that runs
    calls = []

    def halve(dn, src):
        calls.append((dn.clone(), src))
        return dn * 0.5

    sub = evaluate(net, lr, hr, corrector=halve, **kw)
    assert len(calls) == 1 and torch.equal(calls[0][0], plain['dn']) and calls[0][1] is hr
    assert torch.equal(sub['dn'], plain['dn'] * 0.5)
    assert torch.equal(sub['metrics'][:2], quality_assess(plain['dn'] * 0.5, hr))
    evaluate(net, lr, hr, corrector=halve, epoch=3, **kw)
    assert len(calls) == 1
