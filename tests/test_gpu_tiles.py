"""Tiled full-frame inference on the device (pnnp_amd/tiles.py, evaluate.forward_tiled / predict / evaluate(tiles=), csrc/tiles.hip):
the two gather kernels against index maps recorded from the real reference (tests/golden/make_golden_tiles.py), the fused engine
path against its own composition bit for bit, and the whole thing against the CPU oracle run tile by tile."""
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RUN = [m for m in json.load(open(os.path.join(GOLDEN, 'tiles.json')))['cases'] if not m['raises']]
H, W, P, BASE = 80, 150, 48, 16                    # the frame of the network tests: 3 x 5 tiles, body, both strips and the corner
ARGS = dict(nframes=1, nf=8, in_nc=4, out_nc=4)


@pytest.fixture(scope='module')
def maps():
    return np.load(os.path.join(GOLDEN, 'tiles.npz'))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bit-equal, NaNs included"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ 1. crop and merge parity
@pytest.mark.parametrize('m', RUN, ids=[m['tag'] for m in RUN])
def test_crop_and_merge_equal_the_reference_gathers(m, maps):
    from pnnp_amd import ops, tiles
    h, w, p, base, c = m['h'], m['w'], m['P'], m['base'], m['c']
    grid = tiles.TileGrid(h, w, p, base)
    T = grid.T
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, c, h, w, generator=g)
    y = torch.randn(T, c, p, p, generator=g)
    xd, yd = x.cuda(), y.cuda()
    x0, y0 = xd.clone(), yd.clone()
    crop = tiles.eval_crop(xd, p, base)
    want_crop = x.reshape(-1)[torch.from_numpy(maps[m['tag'] + '_crop'].astype(np.int64))]
    assert _same(crop.cpu(), want_crop)
    merge = tiles.eval_merge(yd, h, w, base)
    want_merge = y.reshape(-1)[torch.from_numpy(maps[m['tag'] + '_merge'].astype(np.int64))]
    assert _same(merge.cpu(), want_merge)
    assert _same(tiles.eval_merge(crop, h, w, base), xd)                                  # lossless
    assert _same(tiles.eval_crop(xd, p, base), crop) and _same(tiles.eval_merge(yd, h, w, base), merge)     # repeatable
    assert _same(xd, x0) and _same(yd, y0)                                                # inputs untouched
    # the engines' layout [nt][P][pitch][Cp]: equal to nchw_to_nhwc of the NCHW tiles, zero channels included; the amax slot
    for cp, pitch in ((8, p), (12, p + 3)):
        nhwc = torch.full((T, p, pitch, cp), float('nan'), device='cuda')
        both = torch.full((T, c, p, p), float('nan'), device='cuda')
        slot = torch.zeros(1, dtype=torch.int32, device='cuda')
        ops.tile_crop(xd, grid, 0, T, nchw=both, nhwc=nhwc, amax=slot)
        ref = ops.nchw_to_nhwc(crop, torch.full((T, p, p, cp), float('nan'), device='cuda'), cp)
        assert _same(both, crop) and _same(nhwc[:, :, :p], ref)
        assert torch.isnan(nhwc[:, :, p:]).all()                                          # nothing written past a row's P pixels
        assert _same(slot.view(torch.float32), crop.abs().max().reshape(1))
    # chunks: tiles t0 .. t0 + nt of both kernels; any partition of the tiles fills the frame exactly once
    for nt in (1, 4, T):
        frame = torch.full((1, c, h, w), float('nan'), device='cuda')
        for t0, n in grid.chunks(nt):
            part = torch.full((n, c, p, p), float('nan'), device='cuda')
            nh8 = torch.full((n, p, p, 8), float('nan'), device='cuda')
            ops.tile_crop(xd, grid, t0, n, nchw=part, nhwc=nh8)
            assert _same(part, crop[t0:t0 + n]) and _same(nh8[..., :c], crop[t0:t0 + n].permute(0, 2, 3, 1))
            before = torch.isnan(frame)
            ops.tile_merge(yd[t0:t0 + n].contiguous(), frame, grid, t0, n)
            wrote = before & ~torch.isnan(frame)
            assert int(wrote.sum()) == c * int(grid.owned(t0, n).sum()) and _same(frame[~before], merge[~before])
        assert _same(frame, merge)


def test_kernels_refuse_bad_arguments():
    from pnnp_amd import ops, tiles
    from pnnp_amd._lib import PnnpError
    grid = tiles.TileGrid(H, W, P, BASE)
    x = torch.zeros(1, 4, H, W, device='cuda')
    y = torch.zeros(grid.T, 4, P, P, device='cuda')
    for t0, nt in ((grid.T, 1), (grid.T - 1, 2), (-1, 1)):                                # a tile range outside the grid
        with pytest.raises(PnnpError):
            ops.tile_crop(x, grid, t0, nt, nchw=torch.zeros(nt, 4, P, P, device='cuda'))
        with pytest.raises(PnnpError):
            ops.tile_merge(y[:nt].contiguous(), x.clone(), grid, t0, nt)
    with pytest.raises(PnnpError):
        ops.tile_crop(x, grid, 0, 1)                                                      # no output
    with pytest.raises(PnnpError):
        ops.tile_crop(x, grid, 0, 1, nhwc=torch.zeros(1, P, P, 6, device='cuda'))         # Cp % 4
    with pytest.raises(PnnpError):
        ops.tile_crop(x, grid, 0, 1, nhwc=torch.zeros(1, P, P - 1, 8, device='cuda'))     # pitch < P
    with pytest.raises(PnnpError):
        tiles.eval_merge(y[:-1].contiguous(), H, W, BASE)                                 # not the grid's tile count
    with pytest.raises(PnnpError):
        tiles.eval_crop(torch.zeros(1, 4, 31, 40, device='cuda'), 48, 16)                 # the case the reference raises on


# ------------------------------------------------------------------ 2. the merge's fused tail
@pytest.mark.parametrize('clamp', [False, True])
def test_merge_tail_equals_the_tensor_ops_bit_for_bit(clamp):
    from pnnp_amd import tiles
    grid = tiles.TileGrid(H, W, P, BASE)
    g = torch.Generator(device='cuda').manual_seed(2)
    y = torch.randn(grid.T, 4, P, P, device='cuda', generator=g) * 0.3 + 0.2               # both clamps act
    own = torch.from_numpy(grid.merge_index()).cuda()
    flat = y.view(grid.T, 4, -1)
    t, rc = own // (P * P), own % (P * P)
    for ch, pix in ((1, (0, 0)), (3, (H - 1, W - 1)), (0, (40, 70))):                       # NaNs in owned elements: the corners and the body
        flat[t[pix], ch, rc[pix]] = float('nan')
    plain = tiles.eval_merge(y, H, W, BASE)
    assert int(torch.isnan(plain).sum()) == 3
    for ratio in (3.7, torch.tensor([3.7], device='cuda')):
        got = tiles.eval_merge(y, H, W, BASE, ratio=ratio, clamp=clamp)
        ref = plain * 3.7
        ref = ref.clamp(0, 1) if clamp else ref
        assert _same(got, ref)
        assert int(torch.isnan(got).sum()) == 3 and torch.isnan(got[0, 1, 0, 0]) and torch.isnan(got[0, 3, H - 1, W - 1])
    assert _same(tiles.eval_merge(y, H, W, BASE, clamp=clamp), plain.clamp(0, 1) if clamp else plain)


# ------------------------------------------------------------------ 3. / 4. the networks
def _make(arch, res):
    from pnnp_amd.archs import ResUnet, UNetSeeInDark, initialize_weights
    torch.manual_seed(5)
    net = (UNetSeeInDark if arch == 'unet' else ResUnet)(dict(ARGS, res=res))
    initialize_weights(net)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return net.cuda().eval(), sd


@pytest.fixture(scope='module')
def frame():
    g = torch.Generator().manual_seed(9)
    hr = torch.rand(1, 4, H, W, generator=g) ** 2.2
    ratio = 6.0
    lr = hr / ratio + torch.randn(1, 4, H, W, generator=g) * 0.004
    return lr, hr, ratio


@pytest.fixture(scope='module')
def oracle(frame, maps):
    """arch -> (net, the CPU composition's frame): golden-pinned numpy gathers, the oracle's forward per tile, numpy merge.  Once per module."""
    from oracle import net_torch as O
    lr = frame[0]
    tag = f'h{H}w{W}p{P}b{BASE}c4'
    ci, mi = maps[tag + '_crop'].astype(np.int64), maps[tag + '_merge'].astype(np.int64)
    out = {}
    nthr = torch.get_num_threads(); torch.set_num_threads(min(nthr, 8))
    for arch, res in (('unet', False), ('resunet', True)):
        net, sd = _make(arch, res)
        fwd = O.unet_forward if arch == 'unet' else O.resunet_forward
        tiles_in = torch.from_numpy(lr.numpy().reshape(-1)[ci])
        with torch.no_grad():
            y = torch.cat([fwd(sd, t[None], res=res) for t in tiles_in])
        out[arch] = (net, torch.from_numpy(y.numpy().reshape(-1)[mi]))
    torch.set_num_threads(nthr)
    return out


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
def test_forward_tiled_bit_equals_its_composition(arch, oracle, frame):
    """the same kernels on the same batch with the same amax: only the first layout pass differs, and it writes the same bytes"""
    from pnnp_amd import tiles
    from pnnp_amd.evaluate import forward_tiled
    net, _ = oracle[arch]
    x = frame[0].cuda()
    with torch.no_grad():
        comp = tiles.eval_merge(net(tiles.eval_crop(x, P, BASE)), H, W, BASE)
    got = forward_tiled(net, x, P, BASE)
    assert got.shape == (1, 4, H, W) and _same(got, comp)
    assert _same(forward_tiled(net, x, P, BASE), got)                                      # repeatable
    # a net without an engine takes the crop -> net -> merge fall-back, chunked alike
    plain = lambda t: t * 0.5 + 0.25
    want = tiles.eval_merge(plain(tiles.eval_crop(x, P, BASE)), H, W, BASE)
    for tb in (None, 4):
        assert _same(forward_tiled(plain, x, P, BASE, tile_batch=tb), want)


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
@pytest.mark.parametrize('tile_batch', [None, 4, 1])
def test_forward_tiled_vs_cpu_oracle(arch, tile_batch, oracle, frame):
    from pnnp_amd.evaluate import forward_tiled
    net, ref = oracle[arch]
    got = forward_tiled(net, frame[0].cuda(), P, BASE, tile_batch=tile_batch).cpu()
    print(f'{arch} tile_batch {tile_batch}: max abs diff {float((got - ref).abs().max()):.3e}')
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-6)             # the bar of an eval forward (test_gpu_unet.py)


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
def test_evaluate_tiles_vs_cpu_oracle(arch, oracle, frame):
    """evaluate(tiles=...) on a dst.ori pair against the same steps on the oracle: x ratio, clamp, IlluminanceCorrect, PSNR / SSIM"""
    from oracle import metrics_np as M, net_torch as O
    from pnnp_amd.evaluate import evaluate
    net, ref = oracle[arch]
    lr, hr, ratio = frame
    out = evaluate(net, lr.cuda(), hr.cuda(), ratio=ratio, ori=True, tiles=dict(patch_size=P, base=BASE, tile_batch=4))
    got = out['metrics'].cpu().numpy()
    assert out['dn'].shape == hr.shape and _same(out['lr'].cpu(), (lr * ratio).clamp(0, 1))
    dn = O.illuminance_correct((ref * ratio).clamp(0, 1), hr)
    lr_c = (lr * ratio).clamp(0, 1)
    tgt = M.tensor2im(hr.numpy())
    want = [M.psnr(tgt, M.tensor2im(dn.numpy())), M.ssim(tgt, M.tensor2im(dn.numpy())),
            M.psnr(tgt, M.tensor2im(lr_c.numpy())), M.ssim(tgt, M.tensor2im(lr_c.numpy()))]
    print(f'{arch}: metrics {got.tolist()} oracle {want}')
    assert abs(got[0] - want[0]) < 1e-3 and abs(got[2] - want[2]) < 1e-3, (got, want)     # dB
    assert abs(got[1] - want[1]) < 2e-5 and abs(got[3] - want[3]) < 2e-5, (got, want)
    # the device ratio (no synchronisation) gives the same frames
    out2 = evaluate(net, lr.cuda(), hr.cuda(), ratio=torch.tensor([ratio], device='cuda'), ori=True, tiles=dict(patch_size=P, base=BASE, tile_batch=4))
    assert _same(out2['dn'], out['dn']) and _same(out2['lr'], out['lr'])


def test_engine_tile_input_refusals(oracle, frame):
    from pnnp_amd import tiles
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.evaluate import forward_tiled
    net, _ = oracle['resunet']
    x = frame[0].cuda()
    grid = tiles.TileGrid(H, W, P, BASE)
    with pytest.raises(PnnpError):
        net.engine.forward(None, True, tile_src=(x, grid, 0, 2))                          # train
    with pytest.raises(PnnpError):
        net.engine.forward(None, False, reflect_pad=4, add_residual=False, tile_src=(x, grid, 0, 2))
    with pytest.raises(PnnpError):
        net.engine.forward(None, False, tile_src=(x, grid, grid.T - 1, 2))                # past the grid
    with pytest.raises(PnnpError):
        forward_tiled(net, x, 40, BASE)                                                    # patch_size % 16
    with pytest.raises(PnnpError):
        forward_tiled(net, torch.zeros(1, 8, H, W, device='cuda'), P, BASE)                # not the net's channel count
    with pytest.raises(PnnpError):
        forward_tiled(net, torch.zeros(1, 4, 31, 40, device='cuda'), P, BASE)              # h < patch_size - base


# ------------------------------------------------------------------ 5. predict
def test_predict_packs_and_tiles(oracle):
    from pnnp_amd import isp_ops
    from pnnp_amd.evaluate import forward_tiled, predict
    net, _ = oracle['unet']
    raw = torch.from_numpy(np.random.default_rng(3).integers(400, 16383, size=(2 * H, 2 * W), dtype=np.uint16))
    wp, bl = 16383, 512                                                                    # SonyA7S2
    got = predict(net, raw, wp, bl, P, base=BASE)
    assert got.is_cuda and got.shape == (4, H, W)
    want = forward_tiled(net, isp_ops.raw2bayer(raw.cuda(), wp=wp, bl=bl)[None], P, BASE)[0]
    assert _same(got, want)
    assert _same(predict(net, raw.numpy(), wp, bl, P, base=BASE, tile_batch=4), forward_tiled(net, isp_ops.raw2bayer(raw.cuda(), wp=wp, bl=bl)[None], P, BASE, tile_batch=4)[0])


# ------------------------------------------------------------------ 6. the frame the engine refuses
def test_frame_past_the_image_limit_runs_in_tiles():
    import torch.nn.functional as F
    from pnnp_amd import ops, tiles
    from pnnp_amd._lib import PnnpError
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    from pnnp_amd.evaluate import evaluate
    torch.manual_seed(4)
    net = UNetSeeInDark(dict(nframes=1, res=True, nf=32, in_nc=4, out_nc=4)); initialize_weights(net); net = net.cuda().eval()
    n, p, base = 4100, 512, 64
    assert ops.x3_image_fits(4080, 4080, 32) and not ops.x3_image_fits(n, n, 32)          # just past the limit ((H + 4) W 32 4 < 2^31 up to 4094 x 4094)
    g = torch.Generator(device='cuda').manual_seed(6)
    hr = torch.rand(1, 4, n, n, device='cuda', generator=g) * 0.8 + 0.1
    lr = hr + torch.randn(1, 4, n, n, device='cuda', generator=g) * 0.01
    with pytest.raises(PnnpError, match='too large'):
        evaluate(net, lr, hr, brightness_correct=False)
    out = evaluate(net, lr, hr, brightness_correct=False, with_lr=False, tiles=dict(patch_size=p, base=base, tile_batch=16))
    dn = out['dn']
    assert dn.shape == (1, 4, n, n) and bool(torch.isfinite(dn).all())
    # two tiles cut by torch slicing from the reflect-padded frame (independent of the crop kernel), each through net() on its own
    grid = tiles.TileGrid(n, n, p, base)
    d, l = grid.d, grid.l
    pad = F.pad(lr, (d, d, d, d), mode='reflect')
    i, j = 1, 2
    cases = [(pad[..., i * l:i * l + p, j * l:j * l + p], dn[..., i * l:(i + 1) * l, j * l:(j + 1) * l]),          # a body tile
             (pad[..., -p:, -p:], dn[..., -l:, -l:])]                                                                  # the corner tile
    for tile, region in cases:
        with torch.no_grad():
            ref = net(tile.contiguous())[..., d:-d, d:-d].clamp(0, 1)
        assert float(((ref > 0) & (ref < 1)).float().mean()) > 0.5                        # the clamp leaves most of the comparison alone
        print(f'tile vs merged region: max abs diff {float((region - ref).abs().max()):.3e}')
        np.testing.assert_allclose(region.cpu().numpy(), ref.cpu().numpy(), rtol=1e-4, atol=2e-6)


# ------------------------------------------------------------------ 7. EvalLoop
def test_eval_loop_with_tiles_keeps_the_report_layout(oracle, frame):
    from pnnp_amd.evaluate import EvalLoop
    net, _ = oracle['unet']
    lr, hr, ratio = frame
    lr, hr = lr[..., :80, :144].contiguous().cuda(), hr[..., :80, :144].contiguous().cuda()          # a multiple of 16: the whole-frame loop takes it too
    reports = []
    for t in (None, dict(patch_size=P, base=BASE)):
        loop = EvalLoop(net, ori=True, brightness_correct=True, tiles=t)
        loop.step('frame_a', lr, hr, ratio=ratio)
        loop.step('frame_b', lr, hr, ratio=ratio)
        reports.append(loop.finish(epoch=-1))
    (m0, t0), (m1, t1) = reports
    assert list(m0) == list(m1) == ['frame_a', 'frame_b']
    assert all(len(v) == 2 and all(isinstance(f, float) for f in v) for v in m1.values())
    shape = lambda s: re.sub(r'\d', '0', s)
    assert len(t1.splitlines()) == len(t0.splitlines()) == 3
    assert re.fullmatch(r'Epoch -1: PSNR=\d+\.\d\d', t1.splitlines()[0])
    assert re.fullmatch(r'psnrs_lr=\d+\.\d\d, psnrs_dn=\d+\.\d\d', t1.splitlines()[1])
    assert re.fullmatch(r'ssims_lr=\d\.\d{4}, ssims_dn=\d\.\d{4}', t1.splitlines()[2])
    assert [re.sub(r'\d+', 'N', ln) for ln in t1.splitlines()] == [re.sub(r'\d+', 'N', ln) for ln in t0.splitlines()], shape(t1)
    # the noisy frame's figures do not depend on how the network ran
    assert m1['frame_a'] == m1['frame_b'] and t0.splitlines()[1].split(',')[0] == t1.splitlines()[1].split(',')[0]
