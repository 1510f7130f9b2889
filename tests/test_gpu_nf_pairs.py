"""The NoiseFlow pair kernels (csrc/nf.hip, csrc/nf_train.hip) one launch at a time, straight through the C ABI, every pixel, every
per-tile sum and every statistic against the float64 reference of ONE pair (tests/_nf_pair_ref.py, pinned on the CPU by
tests/test_host_nf_pair_ref.py).  The chain tests (tests/test_gpu_noiseflow.py) need bars that a wrong ring of pixels, a wrong seam
line or a wrong tail round passes; one pair has no chain to amplify rounding, so a tight bar holds everywhere.

Shapes (B, H, W), the smallest that reach each piece of index arithmetic: (1,1,1) every ring tap out of the image | (3,5,3) below one
tile, batch stride | (1,32,64) exact tiles and a seam | (2,33,65) seams both ways, one-pixel partial tiles beside full tiles with
their 2+2+1 rounds | (1,31,34).  Parameters: ``_nf_pair_ref.draw`` with the seeds ``_nf_pair_ref.SEEDS`` (101 .. 105; 204 for the
large-mean case), never the golden state dict: BatchNorm weights and ``scale`` of both signs, large border-ones weights, out_mul 0.6.
Buffers that a kernel must fill are handed over full of NaN.

Bar (nothing in it comes from the device): per compared tensor E32 = max|helper in float32 - helper in float64| on the same inputs,
run on one CPU thread and floored at 2^-22 max|ref64|; every element must satisfy |device - ref64| <= 4 E32.  The sampling step, whose
tanh / exp are the hardware's (about 1e-7 relative), additionally gets 4e-7 |post| sum_c |winv[o][c]| |v[c]| per element (post: the
factor out_mul sqrt(a clean + b) behind the matrix, below 1 here).  bn[24] is compared slot by slot (mean, rstd, var of each layer):
a variance is not measured on the scale of a reciprocal deviation.  The 319 backward sums are one tensor.  From the dx comparison,
and from it alone, the pixels of ``_nf_pair_ref.dx_excluded`` are left out (ReLU masks within rounding of zero; at most 2 %, asserted).

Every test prints its worst error / bar per tensor; 1 is the bar.  Measured on an MI355X (the whole table: profiles/r7/nf_pairs.txt),
worst over the cases:  nf_step eval 0.15;  nf_step_mix with bn_stats 0.90 at (1,1,1) (one pixel, rstd = 316: the offset
beta - (mean + bias) scale cancels against scale (h + bias) in the kernel as in the float32 helper, E32 1.8e-5; 0.24 elsewhere);
nf_train_stats 0.23;  nf_bn_update 0.12;  nf_fwd_step y 0.25, partial 0.09;  nf_train_fwd_pair z 0.27, h1 0.20, h2 0.26, out3 0.26,
bn 0.28, ldpart 0.16 / 0.28;  nf_train_bwd_pair dx 0.43 (25 of 4290 pixels left out at (2,33,65) without clean, none elsewhere),
sums 0.38.  This suite is what replaced E[x^2] - mean^2 in csrc/nf_train.hip: before, a one-pixel image gave var = 6e-8 x^2 where
the reference has 0 (rstd 380 .. 1040x the bar in nf_train_fwd_pair) and the mean-30 case missed var1 / var2 by 1.25 / 1.35."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pnnp_amd import _lib
from tests import _nf_pair_ref as P

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NUL = C.c_void_p(0)
CASES = [(s, False) for s in P.SHAPES]
BN_SLOTS = ('mean1', 'rstd1', 'var1', 'mean2', 'rstd2', 'var2')


@functools.lru_cache(maxsize=None)
def _case(shape, mean30=False):
    return P.draw(shape, P.MEAN30[1] if mean30 else P.SEEDS[shape], mean30)


def _d(t):
    return t.to(F32).contiguous().cuda()


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=F32, device='cuda')


def _host(vec):
    assert vec.numel() == 317 and vec.dtype == F32
    return (C.c_float * 317)(*vec.tolist())


def _both(fn):
    """(helper in float64, helper in float32) on one CPU thread; tuples stay tuples"""
    with P.one_thread():
        return fn(F64), fn(F32)


def _check(name, got, ref64, ref32, extra=None, keep=None):
    """prints and returns the worst |got - ref64| / (4 E32 [+ extra]) over the elements (``keep``: a mask of those compared)"""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.double(), ref32.double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    if keep is not None:
        got, ref64, ref32, extra = got[keep], ref64[keep], ref32[keep], (None if extra is None else extra[keep])
    e32 = P.e32_of(ref32, ref64)
    r = P.worst_ratio(got, ref64, e32, extra)
    print(f'{name}: E32 {e32:.3e} (max|ref| {float(ref64.abs().max()):.3e})  worst error / bar {r:.3f}')
    return r


def _scratch(B, H, W):
    L = _lib.lib()
    tiles, pb = L.pnnp_nf_train_tiles(B, H, W), L.pnnp_nf_train_pblocks(B, H, W)
    gy, gx = P.tiles(H, W)
    assert tiles == B * gy * gx and pb == (B * H * W + 1023) // 1024
    return tiles, _nan(max(tiles * 197, pb * 28))


def _step(c, shape, step, clean, bn=None):
    """one launch of pnnp_nf_step_f32 (or, with device statistics, pnnp_nf_step_mix_f32 without its mix epilogue) -> y"""
    B, H, W = shape
    L = _lib.lib()
    x, y = _d(c['x']), _nan(B, 4, H, W)
    cl = _d(clean) if clean is not None else None
    a, b, m = C.c_float(P.SDN_A), C.c_float(P.SDN_B), C.c_float(P.OUT_MUL)
    if bn is None:
        _lib.check(L.pnnp_nf_step_f32(_lib.ptr(x), _lib.ptr(y), B, H, W, _host(step), _lib.ptr(cl), a, b, m, _lib.stream()), 'nf_step')
    else:
        _lib.check(L.pnnp_nf_step_mix_f32(_lib.ptr(x), _lib.ptr(y), B, H, W, _host(step), _lib.ptr(cl), a, b, m, NUL, C.c_float(1.0), NUL, NUL,
                                          C.c_float(1.0), C.c_float(0.0), C.c_float(0.0), NUL, _lib.ptr(bn), _lib.stream()), 'nf_step_mix')
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), c['x'])
    return y.cpu()


# ------------------------------------------------------------------------------------------------------------ 1. sampling, eval mode
@pytest.mark.parametrize('with_clean', (False, True))
@pytest.mark.parametrize('shape', P.SHAPES)
def test_step_eval_every_pixel(shape, with_clean):
    c = _case(shape)
    clean = c['clean'] if with_clean else None
    y = _step(c, shape, c['step_eval'], clean)
    (r64, reach), (r32, _r) = _both(lambda dt: P.sample_pair(c['step_eval'], c['x'], clean, P.SDN_A, P.SDN_B, P.OUT_MUL, dtype=dt, with_reach=True))
    assert _check(f'nf_step eval {shape} clean={with_clean} y', y, r64, r32, 4e-7 * reach) <= 1


# ------------------------------------------------------------------------------------------------------------ 2. sampling, batch statistics
@pytest.mark.parametrize('shape,mean30', CASES + [(P.MEAN30[0], True)])
def test_train_stats_then_step_then_buffer_update(shape, mean30):
    B, H, W = shape
    c = _case(shape, mean30)
    L = _lib.lib()
    tag = f'{shape}{" mean30" if mean30 else ""}'
    # the statistics
    tiles, part = _scratch(B, H, W)
    u, prm, ident, bn = _d(c['x']), _d(c['prm']), _d(torch.eye(4).reshape(-1)), _nan(24)
    h1, h2 = _nan(B, 4, H, W), _nan(B, 4, H, W)
    _lib.check(L.pnnp_nf_train_stats_f32(_lib.ptr(u), _lib.ptr(ident), _lib.ptr(prm), _lib.ptr(bn), _lib.ptr(h1), _lib.ptr(h2), _lib.ptr(part),
                                         B, H, W, _lib.stream()), 'nf_train_stats')
    torch.cuda.synchronize()
    s64, s32 = _both(lambda dt: P.stats(c['prm'], c['x'], dtype=dt))
    got = bn.cpu()
    worst = {n: _check(f'nf_train_stats {tag} {n}', got[4 * i:4 * i + 4], s64[4 * i:4 * i + 4], s32[4 * i:4 * i + 4]) for i, n in enumerate(BN_SLOTS)}
    # the step, fed the device's own statistics
    y = _step(c, shape, c['step_train'], c['clean'], bn)
    (r64, reach), (r32, _r) = _both(lambda dt: P.sample_pair(c['step_train'], c['x'], c['clean'], P.SDN_A, P.SDN_B, P.OUT_MUL, bn_stats=got,
                                                             dtype=dt, with_reach=True))
    worst['y'] = _check(f'nf_step_mix bn_stats {tag} y', y, r64, r32, 4e-7 * reach)
    # the running buffers
    bufs = [_d(c[k]) for k in ('rm1', 'rv1', 'rm2', 'rv2')]
    nb = [torch.tensor([7], dtype=torch.int64, device='cuda'), torch.tensor([11], dtype=torch.int64, device='cuda')]
    b1, b2 = _d(c['b1']), _d(c['b2'])
    _lib.check(L.pnnp_nf_bn_update_f32(_lib.ptr(bn), _lib.ptr(b1), _lib.ptr(b2), *[_lib.ptr(t) for t in bufs],
                                       _lib.ptr(nb[0]), _lib.ptr(nb[1]), C.c_double(float(B * H * W)), _lib.stream()), 'nf_bn_update')
    torch.cuda.synchronize()
    u64, u32 = _both(lambda dt: P.bn_update(got, c['b1'], c['b2'], c['rm1'], c['rv1'], c['rm2'], c['rv2'], B * H * W, dtype=dt))
    for i, n in enumerate(('running_mean1', 'running_var1', 'running_mean2', 'running_var2')):
        worst[n] = _check(f'nf_bn_update {tag} {n}', bufs[i], u64[i], u32[i])
    assert int(nb[0]) == 8 and int(nb[1]) == 12
    assert torch.equal(bn.cpu(), got)
    assert max(worst.values()) <= 1, {k: v for k, v in worst.items() if not v <= 1}


# ------------------------------------------------------------------------------------------------------------ 3. density direction
@pytest.mark.parametrize('with_clean', (False, True))
@pytest.mark.parametrize('shape', P.SHAPES)
def test_fwd_step_every_pixel_and_tile(shape, with_clean):
    B, H, W = shape
    c = _case(shape)
    L = _lib.lib()
    clean = c['clean'] if with_clean else None
    gy, gx = P.tiles(H, W)
    x, y, partial = _d(c['x']), _nan(B, 4, H, W), _nan(B, gy * gx)
    cl = _d(clean) if with_clean else None
    _lib.check(L.pnnp_nf_fwd_step_f32(_lib.ptr(x), _lib.ptr(y), _lib.ptr(partial), B, H, W, _host(c['step_eval']),
                                      _lib.ptr(cl), C.c_float(P.SDN_A), C.c_float(P.SDN_B), _lib.stream()), 'nf_fwd_step')
    torch.cuda.synchronize()
    (y64, l64), (y32, l32) = _both(lambda dt: P.density_pair(c['step_eval'], c['x'], clean, P.SDN_A, P.SDN_B, dtype=dt))
    tag = f'nf_fwd_step {shape} clean={with_clean}'
    worst = {'y': _check(tag + ' y', y, y64, y32), 'partial': _check(tag + ' partial', partial, P.tile_sums(l64), P.tile_sums(l32))}
    assert max(worst.values()) <= 1, worst


# ------------------------------------------------------------------------------------------------------------ 4. training mode
def _train_fwd(c, shape, clean):
    B, H, W = shape
    L = _lib.lib()
    tiles, part = _scratch(B, H, W)
    dev = dict(x=_d(c['x']), clean=_d(clean) if clean is not None else None, ab=_d(c['ab']) if clean is not None else None,
               wm=_d(c['m'].reshape(-1)), prm=_d(c['prm']), bn=_nan(24), h1=_nan(B, 4, H, W), h2=_nan(B, 4, H, W), out3=_nan(B, 4, H, W),
               z=_nan(B, 4, H, W), ldpart=_nan(tiles, 2), part=part)
    _lib.check(L.pnnp_nf_train_fwd_pair_f32(*[_lib.ptr(dev[k]) for k in ('x', 'clean', 'ab', 'wm', 'prm', 'bn', 'h1', 'h2', 'out3', 'z', 'ldpart', 'part')],
                                            B, H, W, _lib.stream()), 'nf_train_fwd_pair')
    torch.cuda.synchronize()
    return dev


@pytest.mark.parametrize('with_clean', (False, True))
@pytest.mark.parametrize('shape', P.SHAPES)
def test_train_fwd_pair_every_pixel_statistic_and_tile(shape, with_clean):
    c = _case(shape)
    clean = c['clean'] if with_clean else None
    dev = _train_fwd(c, shape, clean)
    r64, r32 = _both(lambda dt: P.train_pair(c['prm'], c['m'].reshape(-1), c['ab'], c['x'], clean, dtype=dt))
    tag = f'nf_train_fwd_pair {shape} clean={with_clean} '
    worst = {n: _check(tag + n, dev[n], r64[i], r32[i]) for i, n in enumerate(('z', 'h1', 'h2', 'out3'))}
    for i, n in enumerate(BN_SLOTS):
        worst[n] = _check(tag + n, dev['bn'][4 * i:4 * i + 4], r64[4][4 * i:4 * i + 4], r32[4][4 * i:4 * i + 4])
    for j, n in enumerate(('ldpart log-det', 'ldpart sum z^2')):
        worst[n] = _check(tag + n, dev['ldpart'][:, j], r64[5][:, j], r32[5][:, j])
    assert max(worst.values()) <= 1, {k: v for k, v in worst.items() if not v <= 1}


@pytest.mark.parametrize('with_clean', (False, True))
@pytest.mark.parametrize('shape', P.SHAPES)
def test_train_bwd_pair_every_pixel_and_sum(shape, with_clean):
    B, H, W = shape
    c = _case(shape)
    L = _lib.lib()
    clean = c['clean'] if with_clean else None
    dev = _train_fwd(c, shape, clean)
    dz, dx, sums = _d(c['dz']), _nan(B, 4, H, W), _nan(319)
    dy2, dy1, dv23 = _nan(B, 4, H, W), _nan(B, 4, H, W), _nan(B, 2, H, W)
    _lib.check(L.pnnp_nf_train_bwd_pair_f32(*[_lib.ptr(dev[k]) for k in ('x', 'clean', 'ab', 'wm', 'prm', 'bn', 'h1', 'h2', 'out3')], _lib.ptr(dz),
                                            C.c_float(P.DZMUL), C.c_float(P.COBJ), _lib.ptr(dx), _lib.ptr(sums), _lib.ptr(dy2), _lib.ptr(dy1),
                                            _lib.ptr(dv23), _lib.ptr(dev['part']), B, H, W, _lib.stream()), 'nf_train_bwd_pair')
    torch.cuda.synchronize()
    (dx64, s64), (dx32, s32) = _both(lambda dt: P.train_pair_bwd(c['prm'], c['m'].reshape(-1), c['ab'], c['x'], clean, c['dz'], P.DZMUL, P.COBJ, dtype=dt))
    out = P.dx_excluded(c['prm'], c['m'].reshape(-1), c['ab'], c['x'], clean)
    share = float(out.double().mean())
    print(f'nf_train_bwd_pair {shape} clean={with_clean}: {int(out.sum())} of {out.numel()} pixels left out of dx')
    assert share <= 0.02, share
    assert bool(torch.isfinite(dx).all())
    keep = ~out.unsqueeze(1).expand(B, 4, H, W)
    tag = f'nf_train_bwd_pair {shape} clean={with_clean} '
    worst = {'dx': _check(tag + 'dx', dx, dx64, dx32, keep=keep), 'sums': _check(tag + 'sums', sums, s64, s32)}
    if not with_clean:                                                     # da, db: no signal-dependent scale, no gradient
        assert float(sums[317:].abs().max()) == 0
    assert max(worst.values()) <= 1, worst


# ------------------------------------------------------------------------------------------------------------ 5. the module's packer
def test_the_module_packs_the_blocks_the_helper_builds(golden_dir):
    """ties the random-parameter tests above to NoiseFlow: for the golden state dict its own step vectors (eval and train), matrices and
    301-float blocks are, bit for bit, what the helper builds from the same dict per the header"""
    import os
    from pnnp_amd.archs import NoiseFlow
    from pnnp_amd.archs.noise_flow import _coupling_params
    g = np.load(os.path.join(golden_dir, 'noiseflow.npz'))
    sd = {k: torch.from_numpy(g['sd:' + k]) for k in [str(x) for x in g['keys']]}
    net = NoiseFlow({'x_shape': (4, 32, 32), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'})
    net.load_state_dict({k: sd[k].clone() for k in net.state_dict().keys()})
    plan = net._plan()
    assert len(plan) == 8
    for train in (False, True):
        net.train(train)
        tables = net._tables(train)
        for k, (vec, winv, _g, _s, host), (ac, _cv, _g2, _s2) in zip(P.COUPLING_IDX[::-1], tables, plan):
            assert vec.dtype == np.float32 and vec.shape == (317,)
            assert np.array_equal(vec[:301], P.step_vector(sd, k, train).numpy()), (k, train)
            w, wi = P.conv_matrices(sd, k - 1)
            assert np.array_equal(winv, wi.numpy()) and np.array_equal(host['w'], w.numpy()), k
            assert torch.equal(torch.cat([t.detach().reshape(-1) for t in _coupling_params(ac)]), P.prm_block(sd, k)), k
