"""Pins tests/_h1_ref.py, the float64 restatement the fp16x1 GPU tests compare against (no GPU): the scale exponent is csrc/h2.h's, the rounding
is ONE correctly rounded fp16 conversion of the scaled value (bit for bit numpy's float64 -> float16 on float32 inputs), with the error it
should have."""
import numpy as np
import torch

from _h1_ref import conv64, h1_conv, h1_round, h1_scale_exp, h1_unet_forward


def test_scale_exp_restates_the_header():
    assert h1_scale_exp(0.0) == 0 and h1_scale_exp(1e-45) == 0 and h1_scale_exp(1e-39) == 0              # zero, subnormals
    assert h1_scale_exp(float('inf')) == 0 and h1_scale_exp(float('nan')) == 0
    assert h1_scale_exp(1.0) == 14 and h1_scale_exp(1.999) == 14 and h1_scale_exp(2.0) == 13 and h1_scale_exp(0.75) == 15
    assert h1_scale_exp(2.0 ** 14) == 0 and h1_scale_exp(2.0 ** 15) == -1 and h1_scale_exp(3e38) == 14 - 127
    assert h1_scale_exp(2.0 ** -113) == 127 and h1_scale_exp(2.0 ** -120) == 127                          # capped: the scale stays a normal float32
    for a in (1e-3, 0.3, 7.0, 123.5, 6e4, 1e9):
        assert 2.0 ** 14 <= a * 2.0 ** h1_scale_exp(a) < 2.0 ** 15


def test_round_is_one_fp16_rounding_of_the_scaled_value():
    g = torch.Generator().manual_seed(0)
    t = torch.randn(4096, generator=g) * torch.logspace(-9, 1, 4096)
    amax = float(t.abs().max())
    se = h1_scale_exp(amax)
    want = (t.numpy().astype(np.float64) * 2.0 ** se).astype(np.float16).astype(np.float64) * 2.0 ** -se
    got = h1_round(t, amax).numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(h1_round(t).numpy(), want)                                                     # amax None: the tensor's own
    err, mag = np.abs(got - t.numpy().astype(np.float64)), np.abs(t.numpy().astype(np.float64))
    normal = mag * 2.0 ** se >= 2.0 ** -14
    assert normal.any() and (~normal).any()
    assert (err[normal] <= 2.0 ** -11 * mag[normal]).all()
    assert (err[~normal] <= 2.0 ** -25 * 2.0 ** -se).all()                                                # half an fp16 subnormal step
    assert 2.0 ** 14 <= np.abs(got).max() * 2.0 ** se < 2.0 ** 15 + 1


def test_round_is_the_identity_on_fp16_values():
    g = torch.Generator().manual_seed(1)
    h = (torch.randn(1000, generator=g) * 100).half()
    h[0] = 2.0 ** -24; h[1] = -32752.0; h[2] = 0.0                                                        # (the maximum in [2^14, 2^15): the scale is 2^-k)
    for k in (0, -7, 11):                                                                                 # any power-of-two multiple of an fp16 tensor
        t = h.double() * 2.0 ** k
        assert torch.equal(h1_round(t.float(), float(t.abs().max())), t)


def test_zero_and_diverged_tensors_take_scale_one():
    z = torch.zeros(5)
    assert torch.equal(h1_round(z), z.double())
    t = torch.tensor([1.0, 2.5, 1e-3])
    assert torch.equal(h1_round(t, float('inf')), t.half().double())
    assert torch.equal(h1_round(t, 0.0), t.half().double())
    bad = torch.tensor([1.0, float('inf'), float('nan')])
    r = h1_round(bad)
    assert r[0] == 1.0 and torch.isinf(r[1]) and torch.isnan(r[2])


def test_conv_restatements_against_torch():
    g = torch.Generator().manual_seed(2)
    x1, x2 = torch.randn(2, 8, 6, 10, generator=g), torch.randn(2, 8, 6, 10, generator=g) * 100.0
    w, b = torch.randn(16, 16, 3, 3, generator=g) * 0.1, torch.randn(16, generator=g)
    F = torch.nn.functional
    x = torch.cat([x1, x2], 1)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert torch.allclose(conv64(x, w, b), ref, rtol=1e-12, atol=1e-12)
    assert torch.allclose(conv64(x, w, b, stride=2), F.conv2d(x.double(), w.double(), b.double(), padding=1, stride=2), rtol=1e-12, atol=1e-12)
    # two segments: ONE scale, from the larger slot -- x1 is rounded on x2's grid
    amax = float(x2.abs().max())
    want = F.leaky_relu(F.conv2d(torch.cat([h1_round(x1, amax), h1_round(x2, amax)], 1), h1_round(w), b.double(), padding=1), 0.2)
    assert torch.allclose(h1_conv(x1, x2, w, b, 1), want, rtol=1e-12, atol=1e-12)
    assert not torch.allclose(h1_conv(x1, x2, w, b, 1), F.leaky_relu(ref, 0.2), rtol=1e-6, atol=1e-6)    # ... and it IS rounded
    e = float((h1_conv(x1, x2, w, b, 0) - ref).norm() / ref.norm())
    assert 1e-5 < e < 2e-3


def test_unet_emulation_is_exact_without_h1_layers_and_rounded_with():
    from oracle import net_torch as O
    sd = {k: v * 6.0 for k, v in O.init_state(O.unet_param_shapes(nf=8), seed=1).items()}
    x = torch.rand(1, 4, 32, 32, generator=torch.Generator().manual_seed(3))
    ref = O.unet_forward({k: v.double() for k, v in sd.items()}, x.double())
    exact = h1_unet_forward(sd, x)
    assert torch.allclose(exact, ref, rtol=1e-11, atol=1e-13)
    layers = [f'conv{i}_{j}' for i in range(1, 10) for j in (1, 2)]
    e = float((h1_unet_forward(sd, x, layers) - ref).norm() / ref.norm())
    assert 1e-5 < e < 1e-2
