"""The float64 reference of the eval-metric kernel tests (tests/_ssim_ref.py), pinned without a GPU: it agrees with the project's
float32 restatement of scikit-image (oracle/metrics_np.py) where float32 is enough, and the input families of
tests/test_gpu_metrics.py do what that file relies on -- the bright flat windows are out of float32's reach per window (so the
per-window test measures something), and every impulse moves the mean SSIM by far more than the bar (so a missed or misplaced window
cannot pass)."""
import numpy as np
import pytest

from oracle import metrics_np as M
from tests import _ssim_ref as R


@pytest.mark.parametrize('shape', [(4, 64, 64), (4, 70, 101), (3, 33, 35), (1, 7, 7)])
def test_float64_reference_agrees_with_the_oracle_on_well_conditioned_frames(shape):
    o, t = R.existing_family(shape, seed=shape[1])
    X, Y = M.tensor2im(o), M.tensor2im(t)
    assert abs(R.psnr(o[0], t[0]) - M.psnr(Y, X)) < 1e-9
    assert abs(R.ssim(o[0], t[0]) - M.ssim(Y, X)) < 1e-6


def test_oracle_ssim_map_is_the_oracle_per_window():
    """the per-window restatement averages to oracle/metrics_np.ssim exactly (same statements, same order)"""
    o, t = R.well_conditioned(3, 33, 35)
    O, T = R.tensor2im(o), R.tensor2im(t)
    mine = np.mean([R.oracle_ssim_map(T[c], O[c]).mean(dtype=np.float64) for c in range(3)])
    assert mine == M.ssim(np.transpose(T, (1, 2, 0)), np.transpose(O, (1, 2, 0)))
    assert R.oracle_ssim_map(T[0], O[0]).shape == R.ssim_map(T[0], O[0]).shape == (27, 29)


def test_tensor2im_rounds_the_product_in_float32_and_clips():
    t = np.array([[[0.1, -0.5, 1.5, 0.4, np.inf, -np.inf]]], np.float32)
    got = R.tensor2im(t)
    assert got.dtype == np.float64
    assert np.array_equal(got[0, 0], [float(np.float32(0.1) * np.float32(255)), 0.0, 255.0, 102.0, 255.0, 0.0])
    assert np.isnan(R.tensor2im(np.array([np.nan], np.float32))[0])


@pytest.mark.parametrize('level,sigma', R.FLAT_FAMILIES)
def test_bright_flat_windows_are_ill_conditioned_in_float32(level, sigma):
    o, t = R.flat_family(level, sigma)
    ref, orc = R.window_errors(o, t)
    e_ref = np.abs(orc - ref).max()
    print(f'family ({level}, {sigma}): max |oracle - float64| per window = {e_ref:.3e}, median {np.median(np.abs(orc - ref)):.3e}')
    assert e_ref > R.SSIM_BAR


def test_dark_noisy_windows_are_well_conditioned_in_float32():
    o, t = R.flat_family(*R.DARK_FAMILY)
    ref, orc = R.window_errors(o, t)
    assert np.abs(orc - ref).max() < R.SSIM_BAR


@pytest.mark.parametrize('pos', R.impulse_positions())
def test_impulse_moves_the_mean_ssim_by_ten_bars(pos):
    """The mean SSIM here is the mean of the SSIM map of the channel that holds the pixel -- what ``ssim_map`` gives and what the kernel
    sums per channel -- and it is the figure of the one-channel launch that tests/test_gpu_metrics.py holds to the 2e-5 bar at every
    position.  Figures (float64, 40 x 70, one pixel of 0.4 raised by 0.2): a window that holds the pixel scores 0.5243, and 1 - mean
    is n x 2.186e-4 for a pixel that n of the 2176 windows hold: 2.19e-4 (10.9 bars) at the corners (0, 0) and (39, 69), which lie in
    ONE window; 1.97e-3 at (2, 2) (9 windows), 3.50e-3 at the positions in 16, 7.65e-3 in 35, 1.07e-2 in 49.  The two-channel figure
    moves by half of that, (s_0 + 1) / 2: 1.093e-4, 5.5 bars, at the corners -- not 10, and that is asserted here as what it is:
    exactly the channel's figure over C, so a dropped corner window misses the two-channel bar by 5 x and the one-channel bar by 10 x."""
    C = R.IMPULSE_SHAPE[0]
    for ch in (0, 1):
        a, b = R.impulse(pos, ch)
        s = R.ssim_channels(a, b)
        assert s[1 - ch] == 1.0                                  # the untouched channel: identical, exactly 1 in float64 too
        n_win = (min(pos[0], 33) - max(pos[0] - 6, 0) + 1) * (min(pos[1], 63) - max(pos[1] - 6, 0) + 1)
        m = R.ssim_map(R.tensor2im(a)[ch], R.tensor2im(b)[ch])
        assert int((m != 1.0).sum()) == n_win                    # exactly the windows that hold the pixel
        assert m.mean() == s[ch]
        print(f'impulse {pos} ch {ch}: {n_win} windows, 1 - mean of the map = {1.0 - m.mean():.4e}, 1 - ssim over {C} channels = {1.0 - s.mean():.4e}')
        assert 1.0 - m.mean() > 10 * R.SSIM_BAR
        assert abs((1.0 - s.mean()) - (1.0 - m.mean()) / C) < 1e-15 and 1.0 - s.mean() > 10 * R.SSIM_BAR / C


def test_illuminance_reference_masks_the_ones_and_scales():
    pred, src = R.illum_inputs((4, 70, 101))
    out = R.illuminance_correct(pred, src)
    p = np.clip(pred, 0, 1).astype(np.float64)
    m = src != 1
    assert 0.25 < 1.0 - m.mean() < 0.35
    k = (p * src * m).sum() / (p * p * m).sum()
    assert np.allclose(out, k * p, rtol=1e-14, atol=0) and (out[pred <= 0] == 0).all()
    # the mask matters: without it the scale is another one
    assert abs((p * src).sum() / (p * p).sum() / k - 1) > 1e-2
    # against the torch restatement the goldens pin (oracle/net_torch.illuminance_correct), float32
    import torch
    from oracle import net_torch as O
    ref = O.illuminance_correct(torch.from_numpy(pred[None]), torch.from_numpy(src[None]))[0].numpy()
    assert np.allclose(out, ref, rtol=2e-6, atol=0)
    with np.errstate(all='ignore'):
        assert np.isnan(R.illuminance_correct(pred, np.ones_like(src))).all()
