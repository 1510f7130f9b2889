"""csrc/demosaic.hip on the device: the integer stencil exactly against the restatement (tests/_fastisp_ref.py, pinned on the host by
tests/test_host_fastisp.py), the one-launch FastISP against the real function's recorded outputs (tests/golden/fastisp.npz), and the
surfaces built on it: ``isp_ops.FastISP``, ``process.fastisp_render``, ``evaluate(render=dict(full=True))``, ``evaluate.predict_rgb``.

Bars.  The stencil and the uint8 levels: exact (the generator asserts that no recorded 255 v lies within 1e-9 of an integer, and the
device evaluates a value within 1e-6 of one to 1e-14 of numpy's).  The float32 planes: 2^-24 absolute against the float64 golden, one float32 ulp at the
top of [0.5, 1]: correct rounding gives half of it, the other half admits a float32 result one ulp from the correctly rounded one.
The kernel's tile is 16 x 64 output pixels (8 x 32 packed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _fastisp_ref as R
from tests._isp_ref import SONY_CCM, SONY_WB

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ['a', 'b', 'c', 'd', 'e', 'q']
TILE_H, TILE_W = 16, 64


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(HERE, 'golden', 'fastisp.npz')))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u16(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def case_rows(gold, tag, n=1):
    """-> (rows, default_ccm) of a golden case: the defaults case runs with gains 2 and the kernel's own float64 matrix"""
    from pnnp_amd import process as P
    if tag + '_wb' in gold:
        return P.isp_rows(gold[tag + '_wb'], gold[tag + '_ccm'], n), False
    return P.isp_rows([2.0, 1.0, 2.0, 1.0], np.eye(3, dtype=np.float32), n), True


# ------------------------------------------------------------------ 1. the stencil alone
SIZES = [(4, 4), (4, 12), (12, 4), (6, 10), (16, 24),
         (TILE_H - 2, TILE_W - 2), (TILE_H, TILE_W), (TILE_H + 2, TILE_W + 2), (TILE_H + 2, TILE_W - 2), (TILE_H - 2, TILE_W + 2),
         (2 * TILE_H + 2, 2 * TILE_W + 2)]


@pytest.mark.parametrize('H,W', SIZES)
def test_demosaic_sizes(H, W):
    from pnnp_amd import isp_ops
    m = np.random.default_rng(H * 1000 + W).integers(0, 65536, size=(H, W), dtype=np.uint16)
    md = dev(m)
    got = isp_ops.demosaic_ea(md)
    assert got.is_cuda and got.dtype == torch.uint16 and got.shape == (H, W, 3)
    assert np.array_equal(u16(got), R.demosaic_ea(m))
    assert np.array_equal(u16(md), m)                                               # the input is untouched
    back = isp_ops.demosaic_ea(m)                                                   # numpy in -> numpy out
    assert isinstance(back, np.ndarray) and back.dtype == np.uint16 and np.array_equal(back, R.demosaic_ea(m))


def test_demosaic_misaligned_views_take_the_scalar_path():
    """W % 8 == 0 from an aligned allocation stores vectors; the same frame read from and written to views two bytes off cannot"""
    from pnnp_amd import isp_ops
    H, W = 16, 24
    m = np.random.default_rng(5).integers(0, 65536, size=(H, W), dtype=np.uint16)
    want = R.demosaic_ea(m)
    buf = torch.zeros(H * W + 1, dtype=torch.uint16, device='cuda')
    src = buf[1:].view(H, W)
    src.copy_(dev(m))
    obuf = torch.zeros(H * W * 3 + 2, dtype=torch.uint16, device='cuda')
    out = obuf[1:-1].view(H, W, 3)
    assert src.data_ptr() % 4 == 2 and out.data_ptr() % 4 == 2 and out.is_contiguous()
    isp_ops.demosaic_ea(src, out=out)
    assert np.array_equal(u16(out), want)
    assert int(u16(obuf)[0]) == 0 and int(u16(obuf)[-1]) == 0                       # nothing written past either end
    assert np.array_equal(u16(isp_ops.demosaic_ea(dev(m))), want)


@pytest.mark.parametrize('kind', ['random', 'ties', 'full'])
def test_demosaic_data_and_batch(kind):
    from pnnp_amd import isp_ops
    rng = np.random.default_rng(11)
    B, H, W = 2, TILE_H + 2, TILE_W + 2
    if kind == 'random':
        m = rng.integers(0, 65536, size=(B, H, W), dtype=np.uint16)
    elif kind == 'ties':
        m = rng.integers(0, 3, size=(B, H, W)).astype(np.uint16)                    # equal gradients are common
    else:
        m = np.full((B, H, W), 65535, np.uint16)
    got = u16(isp_ops.demosaic_ea(dev(m)))
    assert got.shape == (B, H, W, 3) and np.array_equal(got, R.demosaic_ea(m))
    for b in range(B):
        assert np.array_equal(u16(isp_ops.demosaic_ea(dev(m[b]))), got[b])


# ------------------------------------------------------------------ 2. FastISP against the real function's outputs
@pytest.mark.parametrize('tag', CASES)
def test_fastisp_golden(gold, tag):
    from pnnp_amd import isp_ops, process as P
    x, want64, want8 = gold[tag + '_x'], gold[tag + '_out'], gold[tag + '_u8']
    wb, ccm = gold.get(tag + '_wb'), gold.get(tag + '_ccm')
    H, W = 2 * x.shape[1], 2 * x.shape[2]
    xd = dev(x)[None]
    keep = xd.clone()
    rows, default = case_rows(gold, tag)
    f, u = P.fastisp_render(xd, rows, f32=True, u8=True, default_ccm=default)
    assert f.shape == (1, 3, H, W) and f.dtype == torch.float32 and u.shape == (1, H, W, 3) and u.dtype == torch.uint8
    assert torch.equal(xd, keep)                                                    # the input is untouched
    err = np.abs(f[0].permute(1, 2, 0).cpu().numpy().astype(np.float64) - want64).max()
    n8 = int((u[0].cpu().numpy() != want8).sum())
    print(f'fastisp {tag}: float planes max |error| = {err:.3e} (bar {2.0 ** -24:.3e}), {n8} of {want8.size} levels differ')
    assert n8 == 0
    assert err <= 2.0 ** -24
    _, u_only = P.fastisp_render(xd, rows, f32=False, u8=True, default_ccm=default)
    assert torch.equal(u_only, u)                                                   # the bytes do not depend on whether the planes are asked for
    f_only, none = P.fastisp_render(xd, rows, default_ccm=default)
    assert none is None and torch.equal(f_only.view(torch.int32), f.view(torch.int32))
    _, ub = P.fastisp_render(xd, rows, f32=False, u8=True, bgr=True, default_ccm=default)
    assert torch.equal(ub, u.flip(-1))
    f2, u2 = P.fastisp_render(xd, rows, f32=True, u8=True, default_ccm=default)     # bitwise repeatable
    assert torch.equal(f2.view(torch.int32), f.view(torch.int32)) and torch.equal(u2, u)
    # the reference's name and argument order: numpy in -> numpy [H,W,3] float32
    out = isp_ops.FastISP(x, wb, ccm)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (H, W, 3)
    assert np.array_equal(out.view(np.uint32), f[0].permute(1, 2, 0).cpu().numpy().view(np.uint32))
    d = isp_ops.FastISP(xd[0], wb, ccm, 2.2, device_out=True, u8=True)
    assert d.is_cuda and torch.equal(d, u[0])
    assert np.array_equal(isp_ops.FastISP(x, wb, ccm, u8=True, bgr=True), want8[..., ::-1])


def test_fastisp_batch_is_its_single_launches(gold):
    from pnnp_amd import process as P
    x = dev(np.stack([gold['a_x'], gold['q_x'], gold['a_x']]))
    rows = torch.cat([P.isp_rows(SONY_WB, SONY_CCM, 2), P.isp_rows(np.ones(4, np.float32), np.eye(3, dtype=np.float32), 1)])
    f, u = P.fastisp_render(x, rows, f32=True, u8=True)
    for i in range(3):
        fi, ui = P.fastisp_render(x[i:i + 1], rows[i:i + 1].contiguous(), f32=True, u8=True)
        assert torch.equal(fi[0].view(torch.int32), f[i].view(torch.int32)) and torch.equal(ui[0], u[i])
    assert np.array_equal(u[0].cpu().numpy(), gold['a_u8']) and np.array_equal(u[1].cpu().numpy(), gold['q_u8'])
    assert not torch.equal(u[2], u[0])                                              # the third image has its own row


@pytest.mark.parametrize('h,w', [(2, 2), (3, 5), (TILE_H // 2 - 1, TILE_W // 2 - 1), (TILE_H // 2, TILE_W // 2), (TILE_H // 2 + 1, TILE_W // 2 + 1),
                                 (TILE_H + 1, TILE_W + 2)])
def test_fastisp_sizes_against_the_restatement(h, w):
    """odd packed sizes (W % 4 != 0: element stores), the tile's edges, more than one workgroup"""
    from pnnp_amd import process as P
    x = (np.random.default_rng(h * 100 + w).random((4, h, w)) * 1.4 - 0.1).astype(np.float32)
    want = R.fastisp(x, SONY_WB, SONY_CCM)
    rows = P.isp_rows(SONY_WB, SONY_CCM, 1)
    f, u = P.fastisp_render(dev(x)[None], rows, f32=True, u8=True)
    s = 255 * want
    safe = ~((np.abs(s - np.rint(s)) < 1e-9) & (s != 0) & (s != 255))               # (random data: a value next to a threshold is not compared)
    assert safe.mean() > 0.999
    assert np.array_equal(u[0].cpu().numpy()[safe], R.levels(want)[safe])
    assert np.abs(f[0].permute(1, 2, 0).cpu().numpy().astype(np.float64) - want).max() <= 2.0 ** -24
    assert torch.equal(P.fastisp_render(dev(x)[None], rows, f32=False, u8=True)[1], u)


@pytest.mark.parametrize('plane', [0, 1])
def test_fastisp_nan_renders_as_zero(gold, plane):
    from pnnp_amd import process as P
    x = gold['a_x'].copy()
    rows = P.isp_rows(SONY_WB, SONY_CCM, 1)
    zero = x.copy()
    zero[plane, 5, 7] = 0.0
    x[plane, 5, 7] = np.nan
    f, u = P.fastisp_render(dev(x)[None], rows, f32=True, u8=True)
    fz, uz = P.fastisp_render(dev(zero)[None], rows, f32=True, u8=True)
    assert torch.equal(f.view(torch.int32), fz.view(torch.int32)) and torch.equal(u, uz)      # everywhere: inside and outside its neighbourhood
    clean = P.fastisp_render(dev(gold['a_x'])[None], rows, f32=True, u8=True)[1]
    y, xx = 10, 14 + plane
    far = torch.ones(u.shape[1:3], dtype=torch.bool)
    far[y - 1:y + 2, xx - 1:xx + 2] = False
    assert torch.equal(u[0].cpu()[far], clean[0].cpu()[far]) and not torch.equal(u, clean)
    assert torch.equal(P.fastisp_render(dev(x)[None], rows, f32=False, u8=True)[1], u)


def test_fastisp_refusals(gold):
    from pnnp_amd import _lib, isp_ops, process as P
    x = dev(gold['a_x'])[None]
    rows = P.isp_rows(SONY_WB, SONY_CCM, 1)
    with pytest.raises(_lib.PnnpError):
        P.fastisp_render(x[:, :, :1], rows)                                         # h = 1
    with pytest.raises(_lib.PnnpError):
        P.fastisp_render(x, rows, f32=False, u8=False)
    for bad in (rows[:, :15].contiguous(), rows.double(), torch.cat([rows, rows]), None, rows.cpu()):
        with pytest.raises(_lib.PnnpError):
            P.fastisp_render(x, bad)
    with pytest.raises(_lib.PnnpError, match='unsupported'):
        isp_ops.FastISP(gold['a_x'], SONY_WB, SONY_CCM, 2.4)
    with pytest.raises(_lib.PnnpError):
        isp_ops.demosaic_ea(torch.zeros(5, 8, dtype=torch.uint16, device='cuda'))
    # the C entries themselves: a refusal returns PNNP_E_INVALID and leaves the outputs untouched
    lib = _lib.lib()
    h, w = x.shape[2:]
    outf = torch.full((1, 3, 2 * h, 2 * w), -7.0, device='cuda')
    out8 = torch.full((1, 2 * h, 2 * w, 3), 99, dtype=torch.uint8, device='cuda')
    call = lambda *a: lib.pnnp_fastisp_f32(*a, _lib.stream())
    null = C.c_void_p(0)
    assert call(_lib.ptr(x), 1, 1, w, _lib.ptr(rows), C.c_uint(0), _lib.ptr(outf), _lib.ptr(out8)) == -1
    assert call(_lib.ptr(x), 1, h, 1, _lib.ptr(rows), C.c_uint(0), _lib.ptr(outf), _lib.ptr(out8)) == -1
    assert call(_lib.ptr(x), 0, h, w, _lib.ptr(rows), C.c_uint(0), _lib.ptr(outf), _lib.ptr(out8)) == -1
    assert call(_lib.ptr(x), 1, h, w, _lib.ptr(rows), C.c_uint(0), null, null) == -1
    assert call(_lib.ptr(x), 1, h, w, null, C.c_uint(0), _lib.ptr(outf), _lib.ptr(out8)) == -1
    assert call(null, 1, h, w, _lib.ptr(rows), C.c_uint(0), _lib.ptr(outf), _lib.ptr(out8)) == -1
    assert call(_lib.ptr(x), 1, 20000, 20000, _lib.ptr(rows), C.c_uint(0), _lib.ptr(outf), _lib.ptr(out8)) == -1      # 3 H W past 2^31
    src = torch.zeros(8, 8, dtype=torch.uint16, device='cuda')
    out16 = torch.full((8, 8, 3), 77, dtype=torch.uint16, device='cuda')
    assert lib.pnnp_demosaic_ea_u16(_lib.ptr(src), 1, 7, 8, _lib.ptr(out16), _lib.stream()) == -1
    assert lib.pnnp_demosaic_ea_u16(_lib.ptr(src), 1, 2, 8, _lib.ptr(out16), _lib.stream()) == -1
    assert lib.pnnp_demosaic_ea_u16(_lib.ptr(src), 1, 8, 8, null, _lib.stream()) == -1
    torch.cuda.synchronize()
    assert (outf == -7.0).all() and (out8 == 99).all() and (u16(out16) == 77).all()


def test_simple_isp_golden(gold):
    """float64 torch ops: everything before the power is bit-equal to numpy, the power within two float64 ulps each way"""
    from pnnp_amd import isp_ops
    got = isp_ops.SimpleISP(gold['simple_raw'], 512, 16383, list(gold['simple_wb']), 2.2)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == gold['simple_out'].shape
    assert np.allclose(got, gold['simple_out'], rtol=2.0 ** -50, atol=0)
    assert np.allclose(isp_ops.SimpleISP(dev(gold['simple_raw']), device_out=True).cpu().numpy(), gold['simple_default_out'], rtol=2.0 ** -50, atol=0)


# ------------------------------------------------------------------ 3. evaluate(render=dict(full=True)) and predict_rgb
def _tiny_net():
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    torch.manual_seed(5)
    net = UNetSeeInDark(dict(nframes=1, nf=8, in_nc=4, out_nc=4, res=False))
    initialize_weights(net)
    return net.cuda().eval()


def test_evaluate_full_resolution_render():
    from oracle import metrics_np as M
    from pnnp_amd import process as P
    from pnnp_amd.evaluate import EvalLoop, evaluate
    from pnnp_amd.metrics import quality_assess
    g = torch.Generator().manual_seed(3)
    hr = (torch.rand(1, 4, 32, 48, generator=g) ** 2.2).cuda()
    lr = hr + 0.05 * torch.randn(1, 4, 32, 48, generator=g).cuda()
    net = _tiny_net()
    render = dict(wb=SONY_WB, ccm=SONY_CCM)
    half = evaluate(net, lr, hr, render=render)
    out = evaluate(net, lr, hr, render=dict(render, full=True))
    assert set(out) == {'dn', 'lr', 'metrics', 'rgb', 'metrics_rgb'}
    for k in ('dn', 'lr', 'metrics'):
        assert torch.equal(out[k].view(torch.int32), half[k].view(torch.int32))
    rows = P.isp_rows(SONY_WB, SONY_CCM, 1)
    srcs = dict(lr=out['lr'], dn=out['dn'], hr=hr)
    ref = {}
    for k, src in srcs.items():
        f, u = P.fastisp_render(src, rows, f32=True, u8=True)
        assert out['rgb'][k].shape == (64, 96, 3) and out['rgb'][k].dtype == torch.uint8 and torch.equal(out['rgb'][k], u[0])
        ref[k] = R.fastisp(src[0].cpu().numpy(), SONY_WB, SONY_CCM).astype(np.float32).transpose(2, 0, 1)[None]
    tgt = M.tensor2im(ref['hr'])
    want = [M.psnr(tgt, M.tensor2im(ref['dn'])), M.ssim(tgt, M.tensor2im(ref['dn'])), M.psnr(tgt, M.tensor2im(ref['lr'])), M.ssim(tgt, M.tensor2im(ref['lr']))]
    got = out['metrics_rgb'].tolist()
    print('metrics_rgb at full resolution', got, 'oracle', want)
    assert abs(got[0] - want[0]) < 1e-3 and abs(got[2] - want[2]) < 1e-3
    assert abs(got[1] - want[1]) < 2e-5 and abs(got[3] - want[3]) < 2e-5
    assert torch.equal(evaluate(net, lr, hr, render=dict(render, full=True, bgr=True))['rgb']['dn'], out['rgb']['dn'].flip(-1))
    # without the key: the binned render, as before
    for k, src in srcs.items():
        assert torch.equal(half['rgb'][k], P.raw2rgb_v2(src[0], SONY_WB, SONY_CCM, device_out=True, u8=True))
    fl = {k: P.process(src, dev(SONY_WB[None]), dev(SONY_CCM[None])) for k, src in srcs.items()}
    same = torch.cat([quality_assess(fl['dn'], fl['hr']), quality_assess(fl['lr'], fl['hr'])])
    assert torch.equal(half['metrics_rgb'].view(torch.int32), same.view(torch.int32))
    assert torch.equal(evaluate(net, lr, hr, render=dict(render, full=False))['metrics_rgb'].view(torch.int32), same.view(torch.int32))
    loop = EvalLoop(net)
    loop.step('a', lr, hr, render=dict(render, full=True))
    _, text = loop.finish(epoch=3)
    assert text.endswith(f"rgb: psnrs_lr={got[2]:.2f}, psnrs_dn={got[0]:.2f}, ssims_lr={got[3]:.4f}, ssims_dn={got[1]:.4f}")


def test_predict_rgb():
    from pnnp_amd import process as P
    from pnnp_amd.evaluate import predict, predict_rgb
    net = _tiny_net()
    raw = torch.from_numpy(np.random.default_rng(3).integers(400, 16383, size=(128, 160), dtype=np.uint16))
    got = predict_rgb(net, raw, 16383, 512, 48, SONY_WB, SONY_CCM, base=16)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (128, 160, 3)
    dn = predict(net, raw, 16383, 512, 48, base=16)
    want = P.fastisp_render(dn.clamp(0, 1)[None], P.isp_rows(SONY_WB, SONY_CCM, 1), f32=False, u8=True)[1][0]
    assert torch.equal(got, want)
    assert torch.equal(predict_rgb(net, raw, 16383, 512, 48, SONY_WB, SONY_CCM, base=16, bgr=True), want.flip(-1))
