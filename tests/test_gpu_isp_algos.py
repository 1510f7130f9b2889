"""csrc/isp_algos.hip on the device, against the real functions' recorded outputs (tests/golden/isp_algos*.npz, made by
tests/golden/make_golden_isp_algos.py) and the restatement (tests/_isp_algos_ref.py, pinned on the host by tests/test_host_isp_algos.py).

Bars.  The filters (GuidedFilter, FastGuidedFilter, stdfilt), per golden case: max |out - ref64| <= max(4 e_ref, 2^-23 max |ref64|), where
ref64 is the real function on float64 inputs and e_ref = max |ref32 - ref64| is read from the fixture (the reference's own float32
error; 4x is the project's usual margin); and at most 0.1 % of a case's elements may differ in bits from the real function's float32
output.  VST / inverse_VST, bayer2gray, repair_bad_pixels and vst_denoise: bit-equal.  The box kernel's tile is 16 x 64 outputs up to
d = 15 and 32 x 64 beyond: case B's 37 x 150 planes span two tiles and a remainder each way at d = 7, and the 70 x 150 frame below does
at d = 25."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _isp_algos_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, 'golden', 'isp_algos.json')))
FILTERS = {c['tag']: c for c in META['filters']}


@pytest.fixture(scope='module')
def gold():
    g = dict(np.load(os.path.join(HERE, 'golden', 'isp_algos.npz')))
    g.update(np.load(os.path.join(HERE, 'golden', 'isp_algos_b.npz')))
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def run_filter(c, gold, layout=None):
    from pnnp_amd import isp_algos as A
    layout = layout or ('chw' if len(c['shape']) > 2 else 'hwc')
    if c['fn'] == 'stdfilt':
        x = dev(gold[c['x']])
        return A.stdfilt(x, k=c['d'], layout=layout), (x,)
    p, I = dev(gold[c['p']]), dev(gold[c['I']])
    if c['p'] == c['I']:
        I = p.clone()                                              # two tensors: the general kernel (``p is I`` is tested below)
    return getattr(A, c['fn'])(p, I, d=c['d'], eps=c['eps'], layout=layout), (p, I)


# ------------------------------------------------------------------ 1. the filters against the goldens: cases A - E
@pytest.mark.parametrize('tag', sorted(FILTERS))
def test_filter_accuracy(gold, tag):
    c = FILTERS[tag]
    ref32 = gold[tag + '_ref32']
    ref64 = ref32.astype(np.float64) + gold[tag + '_d64']
    e_ref = c['e_ref']
    assert e_ref == float(np.abs(ref32.astype(np.float64) - ref64).max()) > 0
    out, ins = run_filter(c, gold)
    assert out.is_cuda and out.dtype == torch.float32 and list(out.shape) == c['shape']
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    bar = max(4 * e_ref, 2.0 ** -23 * float(np.abs(ref64).max()))
    differ = int((got.view(np.int32) != ref32.view(np.int32)).sum())
    print(f'{tag}: max|out - ref64| = {err:.4g}, e_ref = {e_ref:.4g}, ratio = {err / e_ref:.3f}, bar = {bar:.4g}; '
          f'{differ} of {got.size} elements differ in bits from ref32 ({100.0 * differ / got.size:.3f} %)')
    assert err <= bar
    assert differ <= 1e-3 * got.size
    # bitwise repeatable, and the inputs are untouched
    again, _ = run_filter(c, gold)
    assert same_bits(out, again)
    keys = (c['x'],) if c['fn'] == 'stdfilt' else (c['p'], c['I'])
    for t, k in zip(ins, keys):
        assert np.array_equal(t.cpu().numpy().view(np.int32), gold[k].view(np.int32))


def test_guided_same_tensor_is_bitwise_the_general_path(gold):
    from pnnp_amd import isp_algos as A
    v = dev(gold['B_g_I'])[0]                                      # [4,37,150]
    for fn, x in ((A.GuidedFilter, v), (A.FastGuidedFilter, v[:, :36])):
        x = x.contiguous()
        assert same_bits(fn(x, x, d=7, eps=0.01, layout='chw'), fn(x, x.clone(), d=7, eps=0.01, layout='chw'))


def test_window_25_spans_the_tall_tiles():
    """d = 25 runs on 32 x 64 tiles: 70 x 150 is two of them and a remainder each way; against the restatement"""
    from pnnp_amd import isp_algos as A
    rng = np.random.RandomState(7)
    I = rng.rand(70, 150).astype(np.float32)
    p = (I + 0.1 * rng.randn(70, 150)).astype(np.float32)
    for fn, ref, args in ((A.GuidedFilter, R.GuidedFilter, (p, I)), (A.FastGuidedFilter, R.FastGuidedFilter, (p, I))):
        got = fn(dev(args[0]), dev(args[1]), d=25, eps=1e-2).cpu().numpy()
        want = ref(args[0], args[1], 25, 1e-2, separable=True)
        assert (got.view(np.int32) != want.view(np.int32)).sum() <= 1e-3 * got.size
        assert np.abs(got - want).max() <= 2.0 ** -22
    got = A.stdfilt(dev(I), k=25).cpu().numpy()
    want = R.stdfilt(I, 25, separable=True)
    assert (got.view(np.int32) != want.view(np.int32)).sum() <= 1e-3 * got.size and np.abs(got - want).max() <= 2.0 ** -22


GROWING_WINDOWS = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from pnnp_amd import isp_algos as A
from tests import _isp_algos_ref as R
rng = np.random.RandomState(3)
I = rng.rand(52, 60).astype(np.float32)
p = (I + 0.1 * rng.randn(52, 60)).astype(np.float32)
dI, dp = torch.from_numpy(I).cuda(), torch.from_numpy(p).cuda()
# each mode's first launch asks for more than 64 KB of LDS, its later ones for more than that
for d in (25, 41, 51):
    for name, got, want in (('GuidedFilter', A.GuidedFilter(dp, dI, d=d, eps=1e-2), R.GuidedFilter(p, I, d, 1e-2, separable=True)),
                            ('GuidedFilter self', A.GuidedFilter(dI, dI, d=d, eps=1e-2), R.GuidedFilter(I, I, d, 1e-2, separable=True)),
                            ('FastGuidedFilter', A.FastGuidedFilter(dp, dI, d=d, eps=1e-2), R.FastGuidedFilter(p, I, d, 1e-2, separable=True)),
                            ('stdfilt', A.stdfilt(dI, k=d), R.stdfilt(I, d, separable=True))):
        got = got.cpu().numpy()
        differ = int((got.view(np.int32) != want.view(np.int32)).sum())
        assert differ <= 1e-3 * got.size and np.abs(got - want).max() <= 2.0 ** -22, (name, d, differ, float(np.abs(got - want).max()))
print('growing windows ok')
'''


def test_growing_windows_in_a_fresh_process():
    """A kernel's dynamic-LDS limit is raised once per process and device, so it has to be raised to the instantiation's largest request.
    A process whose first window is 25 asks for 68 096 B in the two-source modes, at 41 for 66 816 B in the one-source modes, and must
    still run 51 afterwards (116 768 B and 79 376 B).  The other tests of this file cannot see that: they share one process, in which
    a d = 51 case runs first."""
    import subprocess
    import sys
    res = subprocess.run([sys.executable, '-c', GROWING_WINDOWS, os.path.dirname(HERE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'growing windows ok' in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ------------------------------------------------------------------ 2. case F: layouts and batches
def test_channel_last_and_batches_are_their_planes(gold):
    from pnnp_amd import isp_algos as A
    p, I = dev(gold['B_g_p']), dev(gold['B_g_I'])                  # [2,4,37,150]
    full = A.GuidedFilter(p, I, d=7, eps=1, layout='chw')
    std = A.stdfilt(I, k=7, layout='chw')
    for b in range(2):                                             # a batch is its single launches
        assert same_bits(full[b], A.GuidedFilter(p[b], I[b], d=7, eps=1, layout='chw'))
        assert same_bits(full[b, 1], A.GuidedFilter(p[b, 1], I[b, 1], d=7, eps=1))
        assert same_bits(std[b, 2], A.stdfilt(I[b, 2], k=7))
    # [H,W,3] channel-last is the three planes run as 'chw'
    p3, I3 = p[0, :3].permute(1, 2, 0).contiguous(), I[0, :3].permute(1, 2, 0).contiguous()
    got = A.GuidedFilter(p3, I3, d=7, eps=1)
    assert got.shape == (37, 150, 3) and got.is_contiguous()
    assert same_bits(got.permute(2, 0, 1).contiguous(), full[0, :3])
    assert same_bits(A.stdfilt(I3, k=7).permute(2, 0, 1).contiguous(), std[0, :3])
    pe, Ie = p[0, :3, :36], I[0, :3, :36]                          # even sides for the fast filter
    fast = A.FastGuidedFilter(pe.contiguous(), Ie.contiguous(), d=7, eps=1, layout='chw')
    got = A.FastGuidedFilter(pe.permute(1, 2, 0).contiguous(), Ie.permute(1, 2, 0).contiguous(), d=7, eps=1)
    assert same_bits(got.permute(2, 0, 1).contiguous(), fast)
    assert same_bits(fast[1], A.FastGuidedFilter(pe[1].contiguous(), Ie[1].contiguous(), d=7, eps=1))
    # a non-contiguous view is taken by value
    assert same_bits(A.GuidedFilter(p[0, 0, :, ::2], I[0, 0, :, ::2], d=7), A.GuidedFilter(p[0, 0, :, ::2].contiguous(), I[0, 0, :, ::2].contiguous(), d=7))


# ------------------------------------------------------------------ 3. case G: locality
@pytest.mark.parametrize('fn', ['GuidedFilter', 'FastGuidedFilter', 'stdfilt'])
def test_a_nan_stays_inside_its_window(gold, fn):
    from pnnp_amd import isp_algos as A
    H, W, d = (36, 150, 7) if fn == 'FastGuidedFilter' else (37, 150, 7)
    r = d // 2
    p, I = gold['B_g_p'][0, 0, :H].copy(), gold['B_g_I'][0, 0, :H].copy()
    y0, x0 = 17, 66                                                # beside a tile corner (rows 16 | 17 ... , columns 63 | 64)

    def run(v):
        q, J = p.copy(), I.copy()
        q[y0, x0] = v
        J[y0, x0] = v
        if fn == 'stdfilt':
            return A.stdfilt(dev(J), k=d).cpu().numpy()
        return getattr(A, fn)(dev(q), dev(J), d=d, eps=1).cpu().numpy()

    bad, clean = run(np.nan), run(0.0)
    reach = r if fn == 'stdfilt' else 2 * r                        # (2r + 1)^2, or (4r + 1)^2 through the second box
    inside = np.zeros((H, W), bool)
    if fn == 'FastGuidedFilter':
        # at half resolution the pixel is (y0 // 2, x0 // 2); two boxes reach 2r there, the 2x upsampling one more low-resolution pixel
        ly, lx = y0 // 2, x0 // 2
        inside[max(0, 2 * (ly - 2 * r - 1)):2 * (ly + 2 * r + 1) + 2, max(0, 2 * (lx - 2 * r - 1)):2 * (lx + 2 * r + 1) + 2] = True
    else:
        inside[max(0, y0 - reach):y0 + reach + 1, max(0, x0 - reach):x0 + reach + 1] = True
    assert not np.isnan(bad[~inside]).any()
    assert np.array_equal(bad[~inside].view(np.int32), clean[~inside].view(np.int32))
    if fn != 'FastGuidedFilter':
        assert np.isnan(bad[inside]).all()                         # ... and it does reach all of its window
    else:
        assert np.isnan(bad[y0, x0]) and np.isnan(bad).sum() > (4 * r + 1) ** 2


# ------------------------------------------------------------------ 4. refusals leave sentinels in place
def test_refusals_leave_the_outputs_untouched():
    import ctypes as C
    from pnnp_amd import _lib
    lib = _lib.lib()
    x = torch.rand(1, 8, 12, device='cuda')
    a, b, ws, out = (torch.full((1, 8, 12), -7.0, device='cuda') for _ in range(4))
    s = (C.c_int64 * 3)(96, 12, 1)
    st = _lib.stream()
    f1 = C.c_float(1.0)
    codes = [lib.pnnp_guided_ab_f32(_lib.ptr(x), _lib.ptr(x), 1, 8, 12, s, 4, f1, 0, _lib.ptr(a), _lib.ptr(b), st),
             lib.pnnp_guided_ab_f32(_lib.ptr(x), _lib.ptr(x), 1, 8, 12, s, 53, f1, 0, _lib.ptr(a), _lib.ptr(b), st),
             lib.pnnp_guided_ab_f32(_lib.ptr(x), _lib.ptr(x), 1, 8, 12, s, 17, f1, 1, _lib.ptr(a), _lib.ptr(b), st),        # REFLECT_101: 8 >= 8
             lib.pnnp_guided_ab_f32(_lib.ptr(x), _lib.ptr(x), 1, 7, 12, s, 3, f1, 2, _lib.ptr(a), _lib.ptr(b), st),         # half: odd H
             lib.pnnp_guided_apply_f32(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 1, 8, 12, s, 6, 0, _lib.ptr(ws), _lib.ptr(out), s, st),
             lib.pnnp_guided_apply_f32(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 1, 8, 12, s, 9, 2, _lib.ptr(ws), _lib.ptr(out), s, st),   # half: 4 >= 4
             lib.pnnp_stdfilt_f32(_lib.ptr(x), 1, 8, 12, s, 17, _lib.ptr(out), s, st),
             lib.pnnp_stdfilt_f32(_lib.ptr(x), 1, 8, 12, s, 2, _lib.ptr(out), s, st),
             lib.pnnp_vst_f32(_lib.ptr(x), C.c_int64(96), 0, C.c_double(1.0), C.c_double(0.0), C.c_double(0.0), C.c_double(1.0), None, C.c_int64(1), _lib.ptr(out), st),
             lib.pnnp_bayer2gray_f32(_lib.ptr(x), 0, 8, 12, _lib.ptr(out), st)]
    assert codes == [-1] * len(codes)
    torch.cuda.synchronize()
    for t in (a, b, ws, out):
        assert (t == -7.0).all()
    raw = torch.full((8, 12), 9.0, device='cuda')
    pts = torch.tensor([[1, 1]], dtype=torch.int32, device='cuda')
    tmp = torch.full((1,), -7.0, device='cuda')
    assert lib.pnnp_repair_bad_pixels(_lib.ptr(raw), 4, 7, 12, _lib.ptr(pts), 1, _lib.ptr(tmp), st) == -1
    assert lib.pnnp_repair_bad_pixels(_lib.ptr(raw), 3, 8, 12, _lib.ptr(pts), 1, _lib.ptr(tmp), st) == -1
    torch.cuda.synchronize()
    assert (raw == 9.0).all() and (tmp == -7.0).all()
    # a point outside the frame that reaches the kernels anyway is skipped, never written
    far = torch.tensor([[8, 0], [0, 12], [-1, 0], [2, 3]], dtype=torch.int32, device='cuda')
    tmp4 = torch.full((4,), -7.0, device='cuda')
    assert lib.pnnp_repair_bad_pixels(_lib.ptr(raw), 4, 8, 12, _lib.ptr(far), 4, _lib.ptr(tmp4), st) == 0
    torch.cuda.synchronize()
    assert (raw == 9.0).all() and tmp4.tolist() == [-7.0, -7.0, -7.0, 9.0]


# ------------------------------------------------------------------ 5. exact matches
def test_vst_bit_equal_to_the_real_functions(gold):
    from pnnp_amd import isp_algos as A
    x, y = dev(gold['vst_x']), dev(gold['ivst_x'])
    assert x.numel() % 4 != 0
    for c in META['vst']:
        f = A.VST(x, c['sigma'], mu=c['mu'], gain=c['gain'], wp=c['wp'])
        b = A.inverse_VST(y, c['sigma'], gain=c['gain'], wp=c['wp'])
        assert f.dtype == torch.float32 and np.array_equal(bits(f), gold['vst_' + c['tag']].view(np.int32)), c
        assert np.array_equal(bits(b), gold['ivst_' + c['tag']].view(np.int32)), c
    assert np.array_equal(bits(A.VST(x, 1.5)), gold['vst_default'].view(np.int32))
    # an offset view (4-byte aligned only) and a 2-D shape take the element path: the same values
    c = META['vst'][-1]
    f = A.VST(x[1:], c['sigma'], mu=c['mu'], gain=c['gain'], wp=c['wp'])
    assert np.array_equal(bits(f), gold['vst_' + c['tag']].view(np.int32)[1:])
    f2 = A.VST(x[:1000].reshape(10, 100), c['sigma'], mu=c['mu'], gain=c['gain'], wp=c['wp'])
    assert f2.shape == (10, 100) and np.array_equal(bits(f2).reshape(-1), gold['vst_' + c['tag']].view(np.int32)[:1000])
    assert np.array_equal(x.cpu().numpy().view(np.int32), gold['vst_x'].view(np.int32))
    # float64 in: float64 torch ops (not on the path), the reference's float64 arithmetic to a few ulp
    f64 = A.VST(x.double(), 2.5, mu=1.0, gain=3.7, wp=16383)
    assert f64.dtype == torch.float64
    assert np.allclose(f64.cpu().numpy(), R.VST(gold['vst_x'].astype(np.float64), 2.5, 1.0, 3.7, 16383), rtol=1e-14, atol=0)


def test_bayer2gray_bit_equal(gold):
    from pnnp_amd import isp_ops
    for hw in ('6x10', '34x70'):
        m = gold[f'gray_{hw}_x']
        got = isp_ops.bayer2gray(dev(m))
        assert got.is_cuda and np.array_equal(bits(got), gold[f'gray_{hw}_out'].view(np.int32))
        assert np.array_equal(isp_ops.bayer2gray(m).view(np.int32), gold[f'gray_{hw}_out'].view(np.int32))       # numpy in, numpy out
    both = isp_ops.bayer2gray(dev(np.stack([gold['gray_6x10_x'], gold['gray_6x10_x'][::-1].copy()])))
    assert np.array_equal(bits(both[0]), gold['gray_6x10_out'].view(np.int32))
    assert np.array_equal(both[1].cpu().numpy(), R.bayer2gray(gold['gray_6x10_x'][::-1].copy()))


@pytest.mark.parametrize('tag', [c['tag'] for c in META['repair']])
def test_repair_bad_pixels_bit_equal(gold, tag):
    from pnnp_amd import isp_ops
    raw, pts, want = gold[f'repair_{tag}_in'], gold[f'repair_{tag}_pts'], gold[f'repair_{tag}_out']
    t = dev(raw.view(np.int16)).view(torch.uint16) if raw.dtype == np.uint16 else dev(raw)
    got = isp_ops.repair_bad_pixels(t, [tuple(int(v) for v in p) for p in pts])
    assert got is t                                                # in place, and returned
    back = got.cpu().view(torch.int16).numpy().view(np.uint16) if raw.dtype == np.uint16 else got.cpu().numpy()
    assert np.array_equal(back, want)
    listed = np.zeros(raw.shape, bool)
    for y, x in pts:
        listed[y, x] = True
    assert np.array_equal(back[~listed], raw[~listed])             # pixels not listed are untouched
    if len(pts):                                                   # the points as a device tensor
        t2 = dev(raw.view(np.int16)).view(torch.uint16) if raw.dtype == np.uint16 else dev(raw)
        isp_ops.repair_bad_pixels(t2, dev(pts))
        assert torch.equal(t2.view(torch.int16) if raw.dtype == np.uint16 else t2, got.view(torch.int16) if raw.dtype == np.uint16 else got)


# ------------------------------------------------------------------ 6. vst_denoise and evaluate(baseline=)
def _by_hand(x, gain, sigma, d, eps, scale_t):
    from pnnp_amd import isp_algos as A
    v = A.VST(x * scale_t, sigma, 0, gain)
    return A.inverse_VST(A.GuidedFilter(v, v, d, eps, layout='chw'), sigma, gain) / scale_t


def test_vst_denoise_is_the_composition():
    from pnnp_amd import isp_algos as A
    g = torch.Generator().manual_seed(11)
    x = torch.rand(3, 4, 22, 70, generator=g).cuda() * 0.2
    for scale in (1.0, 15871.0 / 100):
        st = torch.full((1,), scale, dtype=torch.float32, device='cuda')
        assert same_bits(A.vst_denoise(x, 2.1, 3.5, d=7, eps=1.0, scale=scale), _by_hand(x, 2.1, 3.5, 7, 1.0, st))
    sb = torch.tensor([15871.0 / 100, 15871.0 / 250, 15871.0], device='cuda')
    assert same_bits(A.vst_denoise(x, 2.1, 3.5, d=5, eps=0.5, scale=sb), _by_hand(x, 2.1, 3.5, 5, 0.5, sb.reshape(3, 1, 1, 1)))
    odd = x[0, 0, :21, :67].contiguous()                           # 1407 elements: the element path of the VST launches
    assert same_bits(A.vst_denoise(odd, 2.1, 3.5, scale=158.71), _by_hand(odd, 2.1, 3.5, 7, 1.0, torch.full((1,), 158.71, device='cuda')))


def test_vst_denoise_improves_a_poisson_gaussian_frame():
    from pnnp_amd import isp_algos as A, process as P
    from pnnp_amd.metrics import quality_assess
    yy, xx = torch.meshgrid(torch.arange(64.0), torch.arange(96.0), indexing='ij')
    clean = (0.05 + 0.02 * torch.sin(xx / 30) * torch.cos(yy / 25))[None].repeat(4, 1, 1).cuda().contiguous()    # dark, smooth: [4,64,96]
    wp, bl, K, sig = 16383, 512, 2.0, 4.0
    param = dict(K=K, sigGs=sig, sigTL=sig, lam=0.0, sigR=0.0, q=1 / 2 ** 14, ratio=1.0, wp=wp, bl=bl, bias=0)
    P.manual_seed(7)
    noisy = P.generate_noisy_torch(clean, noise_code='p', param=param).contiguous()
    den = A.vst_denoise(noisy, K, 0.0, d=7, eps=1.0, scale=float(wp - bl))
    before = float(quality_assess(noisy.clamp(0, 1)[None], clean[None])[0])
    after = float(quality_assess(den.clamp(0, 1)[None], clean[None])[0])
    print(f'PSNR noisy {before:.2f} dB -> VST + guided filter {after:.2f} dB')
    assert after > before


def _tiny_net():
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    torch.manual_seed(5)
    net = UNetSeeInDark(dict(nframes=1, nf=8, in_nc=4, out_nc=4, res=False))
    initialize_weights(net)
    return net.cuda().eval()


def test_evaluate_baseline():
    from pnnp_amd import evaluate as E
    from pnnp_amd.metrics import quality_assess
    g = torch.Generator().manual_seed(3)
    hr = (torch.rand(1, 4, 32, 48, generator=g) ** 2.2).cuda()
    lr = hr + 0.05 * torch.randn(1, 4, 32, 48, generator=g).cuda()
    net = _tiny_net()
    for ori, ratio in ((False, 100.0), (True, 100.0), (False, 3.0), (True, 7.0)):          # 15871 / 3: the float32 and the float64 quotient round apart
        src = lr / ratio if ori else lr
        plain = E.evaluate(net, src, hr, ratio=ratio, ori=ori)
        none = E.evaluate(net, src, hr, ratio=ratio, ori=ori, baseline=None)
        with E._precision(net, None):                             # the body the entry wrapped before it took ``baseline``
            body = E._evaluate(net, src, hr, ratio, ori, True, -1, None, True, None, None)
        assert set(plain) == set(none) == set(body) == {'dn', 'lr', 'metrics'}
        for k in plain:
            assert torch.equal(plain[k], none[k]) and torch.equal(plain[k], body[k])
        cfg = dict(gain=2.1, sigma=3.5, wp_bl=15871.0, d=5, eps=1.0)
        out = E.evaluate(net, src, hr, ratio=ratio, ori=ori, baseline=cfg)
        assert set(out) == {'dn', 'lr', 'metrics', 'base', 'psnr_base', 'ssim_base'}
        for k in plain:
            assert torch.equal(plain[k], out[k])
        # the rule: scale = float32(wp_bl) / float32(ratio), one float32 division, however the ratio is passed
        scale = float(np.float32(15871.0) if ori else np.float32(15871.0) / np.float32(ratio))
        hand = _by_hand(src.contiguous().float(), 2.1, 3.5, 5, 1.0, torch.full((1,), scale, dtype=torch.float32, device='cuda'))
        hand = ((hand * ratio) if ori else hand).clamp(0, 1)
        assert same_bits(out['base'], hand)
        m = quality_assess(hand, hr)
        assert torch.equal(out['psnr_base'], m[0]) and torch.equal(out['ssim_base'], m[1])
        for r_as in (torch.tensor([ratio]), torch.tensor([ratio], device='cuda'), torch.tensor(ratio, dtype=torch.float64, device='cuda')):
            alt = E.evaluate(net, src, hr, ratio=r_as, ori=ori, baseline=cfg)
            assert same_bits(alt['base'], hand) and torch.equal(alt['psnr_base'], m[0]) and torch.equal(alt['ssim_base'], m[1])
    loop = E.EvalLoop(net)
    loop.step('a', lr, hr, ratio=ratio)
    _, text = loop.finish(epoch=3)
    assert 'baseline' not in text and text.count('\n') == 2        # the log line is what it was
    loop = E.EvalLoop(net, baseline=cfg)
    res = loop.step('a', lr, hr, ratio=ratio)
    metrics, text = loop.finish(epoch=3)
    assert f"psnrs_base={float(res['psnr_base']):.2f}" in text and list(metrics) == ['a']
    with pytest.raises(E.PnnpError):
        E.evaluate(net, lr, hr, baseline=cfg)                      # no ratio
    with pytest.raises(E.PnnpError):
        E.evaluate(net, lr, hr, ratio=ratio, baseline=dict(gain=1.0))
