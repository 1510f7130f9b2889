"""csrc/unet_loss.hip on the MI355X: Unet_Loss (plain / Charbonnier, flat / 4-level pyramid) and the Sobel edge term with their gradients, against
ops.l1_clamp_loss (options off: the same bits), the reference's recorded float32 outputs (tests/golden/unet_loss.npz) and the float64 restatement
(tests/_unet_loss_ref.py); then losses.Unet_Loss as an autograd module and HipTrainStep(loss=).

Bars.  Scalars (loss, level terms, edge term) and Charbonnier gradients: the kernel's error against float64 is at most max(4 x the reference's own
float32 error against float64 in that case, one float32 ulp of the value) -- the bar of DESIGN section 7b rows f6 to f11.  L1-family gradients are
an integer (8 s0 + 4 s1 + 2 s2 + s3 under the pyramid, the sign otherwise, the Sobel integer in [-8, 8]) times a float32 coefficient, so they are
compared EXACTLY with the restatement's integers through the documented coefficient chain (R.l1_family_expected), except where the restatement
marks an element fragile (some |d_l|, | |u| - |v| | or |u| below 1e-6: a float32 pooling order may flip the sign); at most 0.5 % of a case may be
fragile, and the planted elements are compared exactly whatever their flag.

Observed on the MI355X (every figure is printed before it is asserted): the largest error / bar over all scalars 0.69 (the plain L1 loss of the
8 x 8 case, whose float partials are l1_clamp_kernel's), 0.63 for a level term, 0.39 for a Charbonnier gradient; no L1-family gradient element
differed from the restatement's integers in any case and none was fragile outside the planted case; the Charbonnier-pyramid step's loss lay
1.4e-8 from oracle + restatement."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import _unet_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24
NAN = float('nan')
MODES = [(c, p) for c in (0, 1) for p in (0, 1)]
FRAGILE_CAP = 0.005


@pytest.fixture(scope='module')
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'unet_loss.npz'))
    meta = json.load(open(os.path.join(golden_dir, 'unet_loss.json')))
    return {k: g[k] for k in g.files}, {c['tag']: c for c in meta['cases']}


_REFS = {}


def ref_of(golden, tag, **kw):
    """the float64 restatement of a golden case, computed once per (case, settings)"""
    key = (tag, tuple(sorted((k, v if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in kw.items())))
    if key not in _REFS:
        _REFS[key] = R.closed_form(golden[0][f'{tag}_pred'], golden[0][f'{tag}_hr'], **kw)
    return _REFS[key]


def bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def run(pred, hr, Cp=None, nchw=False, scale=None, terms=True, **kw):
    """ops.unet_loss on host arrays; every output starts as NaN -> dict of host arrays"""
    from pnnp_amd import ops
    pred, hr = torch.as_tensor(pred).to(DEV), torch.as_tensor(hr).to(DEV)
    B, Cc, H, W = pred.shape
    g = torch.full((B, H, W, Cp), NAN, device=DEV) if Cp else None
    gn = torch.full((B, Cc, H, W), NAN, device=DEV) if nchw else None
    lo = torch.full((1 + B,), NAN, device=DEV)
    tm = torch.full((5,), NAN, device=DEV) if terms else None
    ws = torch.full((ops.unet_loss_workspace_floats(B),), NAN, device=DEV)
    sc = torch.as_tensor(scale).to(DEV) if scale is not None else None
    p0, h0 = pred.clone(), hr.clone()
    ops.unet_loss(pred, hr, g, lo, ws, scale=sc, terms=tm, grad_nchw=gn, **kw)
    torch.cuda.synchronize()
    assert same_bits(pred, p0) and same_bits(hr, h0)                       # the inputs are never modified
    return dict(lo=lo.cpu(), terms=tm.cpu() if terms else None, nhwc=g.cpu() if Cp else None, nchw=gn.cpu() if nchw else None)


def recombine(tm):
    """Pyramid_Loss(rate=0.5, norm=True) of four float32 level terms, in float32 and in the reference's order"""
    f = np.float32
    return (((f(tm[0]) + f(tm[1]) * f(0.5)) + f(tm[2]) * f(0.25)) + f(tm[3]) * f(0.125)) / f(1.875)


def nhwc_to_nchw(g, Cc):
    return g[..., :Cc].permute(0, 3, 1, 2).contiguous()


def within(name, dev, f32, f64):
    """max(4 x the reference's own float32 error, one float32 ulp of the value); prints the observed ratio"""
    dev, f32, f64 = np.asarray(dev, np.float64), np.asarray(f32, np.float64), np.asarray(f64, np.float64)
    top = np.abs(f64).max()
    e_ref, e_dev = np.abs(f32 - f64).max(), np.abs(dev - f64).max()
    bar = max(4 * e_ref, float(np.spacing(np.float32(top))))
    print(f'{name}: E_dev {e_dev:.3e} E_ref {e_ref:.3e} ulp {float(np.spacing(np.float32(top))):.3e} -> E_dev / bar {e_dev / bar:.3f}')
    assert e_dev <= bar, (name, e_dev, e_ref, bar)


# ------------------------------------------------------------------------------------------------ options off
OFF_SHAPES = [(1, 3, 8, 8, 4), (3, 4, 16, 24, 4), (3, 4, 16, 24, 8), (1, 8, 8, 8, 8), (2, 4, 32, 40, 8), (2, 4, 5, 7, 4), (1, 1, 1, 1, 4), (1, 4, 130, 131, 8)]


@pytest.mark.parametrize('B,Cc,H,W,Cp', OFF_SHAPES)
def test_options_off_is_l1_clamp_loss_bit_for_bit(B, Cc, H, W, Cp):
    """charbonnier = pyramid = 0, grad = 0, clamp_pred = 1: loss, SSE and gradient are ops.l1_clamp_loss's bits, with the ratio, the target clamp and
    grad_weight on and off; 130 x 131 gives a thread more than one pixel (64 blocks x 256 threads per crop)."""
    from pnnp_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + Cc * 100 + H + W)
    pred = torch.rand(B, Cc, H, W, generator=gen) * 1.4 - 0.2
    hr = torch.rand(B, Cc, H, W, generator=gen) * 1.3 - 0.1
    pred.view(-1)[0] = 0.0
    hr.view(-1)[0] = 0.0
    for scaled, clamp_target, gw in ((False, False, 1.0), (True, False, 1.0), (False, True, 0.6), (True, True, 0.6)):
        scale = (torch.rand(B, generator=gen) + 0.5) if scaled else None
        g = torch.full((B, H, W, Cp), NAN, device=DEV); lo = torch.full((1 + B,), NAN, device=DEV); ws = torch.full((128 * B,), NAN, device=DEV)
        ops.l1_clamp_loss(pred.to(DEV), hr.to(DEV), g, lo, ws, scale=scale.to(DEV) if scaled else None, clamp_target=clamp_target, grad_weight=gw)
        got = run(pred, hr, Cp=Cp, nchw=True, scale=scale, clamp_target=clamp_target, grad_weight=gw)
        what = (scaled, clamp_target, gw)
        assert same_bits(got['lo'], lo.cpu()), (what, got['lo'], lo.cpu())
        assert same_bits(got['nhwc'], g.cpu()), what
        assert same_bits(got['nchw'], nhwc_to_nchw(g.cpu(), Cc)), what
        assert same_bits(got['terms'], torch.tensor([float(lo[0]), 0, 0, 0, 0])), what


# ------------------------------------------------------------------------------------------------ values against the goldens
# 5 x 7 ('f') is the edge term's case: only the flat modes exist there (the pyramid's refusal of such a size is tested below)
CASE_MODES = [(tag, c, p) for tag in ('a', 'b', 'c', 'd', 'e', 'f', 'planted') for c, p in MODES if not (p and tag == 'f')]


@pytest.mark.parametrize('tag,c,p', CASE_MODES)
def test_values_against_the_recorded_reference(golden, tag, c, p):
    """Every golden case in every mode it allows, through both gradient layouts and both paddings (C = 4: Cp 4 and 8; C = 3: Cp 4; C = 8: Cp 8)."""
    g, meta = golden
    assert meta[tag]['pyramid'] or not p
    pred, hr = g[f'{tag}_pred'], g[f'{tag}_hr']
    Cc = pred.shape[1]
    ref = ref_of(golden, tag, charbonnier=bool(c), pyramid=bool(p))
    outs = [run(pred, hr, Cp=Cp, nchw=True, charbonnier=bool(c), pyramid=bool(p)) for Cp in ((4, 8) if Cc <= 4 else (8,))]
    for o in outs:
        name = f'{tag} c{c}p{p}'
        within(name + ' loss', o['lo'][0], g[f'{tag}_loss_c{c}p{p}'], ref['loss'])
        if p:
            for l in range(4):
                within(f'{name} term {l}', o['terms'][l], g[f'{tag}_terms_c{c}'][l], ref['terms'][l])
        else:
            assert same_bits(o['terms'], torch.tensor([float(o['lo'][0]), 0, 0, 0, 0]))
        # SSE: float partials as in l1_clamp_kernel; the longest chain: 8 elements, <= 8 channels, one trip, the LDS tree 8, the finish 1 + 6
        assert np.all(np.abs(o['lo'][1:].double().numpy() - ref['sse']) <= 32 * U * ref['sse']), name
        Cp = o['nhwc'].shape[3]
        assert same_bits(nhwc_to_nchw(o['nhwc'], Cc), o['nchw']), name                                        # both layouts: the same numbers
        assert same_bits(o['nhwc'][..., Cc:], torch.zeros(o['nhwc'][..., Cc:].shape)), (name, Cp)             # padding channels: +0
        got = o['nchw'].numpy()
        if c:
            within(name + ' gradient', got, g[f'{tag}_grad_c{c}p{p}'], ref['grad'])
        else:
            want = R.l1_family_expected(ref, pyramid=bool(p))
            differ = got.view(np.int32) != want.view(np.int32)
            print(f'{name}: {int(differ.sum())} of {differ.size} gradient elements differ, {int(ref["fragile"].sum())} fragile')
            assert not (differ & ~ref['fragile']).any(), (name, int((differ & ~ref['fragile']).sum()))
            assert tag == 'planted' or ref['fragile'].mean() <= FRAGILE_CAP
    assert all(same_bits(outs[0][k], o[k]) for o in outs[1:] for k in ('lo', 'terms', 'nchw'))


@pytest.mark.parametrize('tag', ['e', 'f', 'b', 'planted'])
def test_edge_term_against_the_recorded_reference(golden, tag):
    """grad_loss alone (recon = 0) on 32 x 40 (tiles across a row of tiles, a partial tile), 5 x 7 and 8 x 8 (one partial tile), and added to the L1
    and Charbonnier losses with a weight: the total and the summed gradient."""
    g, _ = golden
    pred, hr = g[f'{tag}_pred'], g[f'{tag}_hr']
    Cc = pred.shape[1]
    ref = ref_of(golden, tag, grad=1.0, recon=False)
    o = run(pred, hr, Cp=4 if Cc <= 4 else 8, nchw=True, grad=1.0, recon=False)
    within(f'{tag} edge loss', o['lo'][0], g[f'{tag}_edge_loss'], ref['loss'])
    assert same_bits(o['terms'], torch.tensor([0, 0, 0, 0, float(o['lo'][0])])) and not o['lo'][1:].any()
    want = R.l1_family_expected(ref, grad=1.0)
    differ = o['nchw'].numpy().view(np.int32) != want.view(np.int32)
    print(f'{tag} edge: {int(differ.sum())} of {differ.size} gradient elements differ, {int(ref["fragile"].sum())} fragile')
    assert not (differ & ~ref['fragile']).any() and ref['fragile'].mean() <= FRAGILE_CAP
    assert same_bits(nhwc_to_nchw(o['nhwc'], Cc), o['nchw']) and not o['nhwc'][..., Cc:].any()
    # recon + 0.25 * edge, L1: exact integers again; the total is the float32 sum of the two parts
    ref2 = ref_of(golden, tag, grad=0.25)
    o2 = run(pred, hr, Cp=8, nchw=True, grad=0.25)
    want2 = R.l1_family_expected(ref2, grad=0.25)
    differ = o2['nchw'].numpy().view(np.int32) != want2.view(np.int32)
    assert not (differ & ~ref2['fragile']).any(), int((differ & ~ref2['fragile']).sum())
    assert same_bits(o2['terms'][4], o['terms'][4])
    assert float(o2['lo'][0]) == float(np.float32(o2['terms'][0]) + np.float32(0.25) * np.float32(o2['terms'][4]))
    assert abs(float(o2['lo'][0]) - ref2['loss']) <= 4 * U * ref2['loss']
    assert same_bits(nhwc_to_nchw(o2['nhwc'], Cc), o2['nchw'])


def test_edge_term_on_one_pixel():
    """1 x 1: every Sobel tap but the (zero) centre falls on the padding, so the term and its gradient are exactly zero."""
    o = run(np.full((2, 3, 1, 1), 0.25, np.float32), np.full((2, 3, 1, 1), 0.75, np.float32), Cp=4, nchw=True, grad=1.0, recon=False)
    assert same_bits(o['lo'], torch.zeros(3)) and same_bits(o['nchw'], torch.zeros(2, 3, 1, 1)) and same_bits(o['nhwc'], torch.zeros(2, 1, 1, 4))


# ------------------------------------------------------------------------------------------------ planted elements
@pytest.mark.parametrize('c,p', MODES)
def test_planted_elements_exactly(golden, c, p):
    """The planted case's three blocks, compared exactly whatever the fragile flag: pred exactly 0, 1 and -0.0 pass the clamp, their float32
    neighbours outside do not, d == 0 at level 0 gives sign 0; a block with pred == hr has every level exactly zero (Charbonnier value
    sqrt(1e-6), gradient 0); a block of +-0.25 halves has a level-3 mean that cancels exactly while levels 0 to 2 do not."""
    g, _ = golden
    pred, hr = g['planted_pred'], g['planted_hr']
    ref = ref_of(golden, 'planted', charbonnier=bool(c), pyramid=bool(p))
    got = run(pred, hr, nchw=True, charbonnier=bool(c), pyramid=bool(p))['nchw'].numpy()
    blocks = [(0, slice(0, 8), slice(0, 8)), (1, slice(0, 8), slice(8, 16)), (2, slice(8, 16), slice(0, 8))]
    if not c:
        want = R.l1_family_expected(ref, pyramid=bool(p))
        for ch, ys, xs in blocks:
            assert np.array_equal(got[0, ch, ys, xs].view(np.int32), want[0, ch, ys, xs].view(np.int32)), (ch, got[0, ch, ys, xs], want[0, ch, ys, xs])
    row = got[0, 0, 0, :6]
    assert row[0] < 0 and row[1] > 0 and row[2] < 0 and row[3] == 0 and row[4] == 0            # 0, 1, -0.0 pass; the neighbours outside do not
    if not p:
        assert row[5] == 0                                                                      # d == 0: sign 0, and 0 / sqrt(1e-6)
    assert not got[0, 1, 0:8, 8:16].any()                                                       # pred == hr: zero at every level
    # the two constructed blocks alone, as 1 x 1 x 8 x 8 problems
    same = run(hr[:, 1:2, 0:8, 8:16].copy(), hr[:, 1:2, 0:8, 8:16].copy(), nchw=True, charbonnier=bool(c), pyramid=bool(p))
    root = float(np.sqrt(np.float32(1e-6)))
    want_terms = [root if c else 0.0] * (4 if p else 1) + [0.0] * (0 if p else 3) + [0.0]
    assert same['terms'].tolist() == want_terms and not same['nchw'].any()
    assert float(same['lo'][0]) == float(recombine(same['terms'].numpy()) if p else same['terms'][0]) and float(same['lo'][1]) == 0.0
    halves = run(pred[:, 2:3, 8:16, 0:8].copy(), hr[:, 2:3, 8:16, 0:8].copy(), nchw=True, charbonnier=bool(c), pyramid=bool(p))
    if p:
        assert float(halves['terms'][3]) == (root if c else 0.0)
        if not c:
            assert halves['terms'].tolist() == [0.25, 0.25, 0.25, 0.0, 0.0]
            k = np.where(np.arange(8) < 4, 14, -14).astype(np.float32) * (np.float32(1.0 / 64) * np.float32(1.0 / 15))
            assert np.array_equal(halves['nchw'].numpy()[0, 0], np.broadcast_to(k, (8, 8)))


# ------------------------------------------------------------------------------------------------ other properties
@pytest.mark.parametrize('kw', [dict(), dict(charbonnier=True, pyramid=True), dict(pyramid=True), dict(grad=0.5)], ids=str)
def test_nan_crop_determinism_and_layouts(golden, kw):
    g, _ = golden
    pred, hr = g['c_pred'].copy(), g['c_hr']                          # B = 3
    sc = np.array([0.5, 1.0, 1.5], np.float32)
    a = run(pred, hr, Cp=8, nchw=True, scale=sc, clamp_target=True, grad_weight=0.6, **kw)
    b = run(pred, hr, Cp=8, nchw=True, scale=sc, clamp_target=True, grad_weight=0.6, **kw)
    assert all(same_bits(a[k], b[k]) for k in a)                      # two runs: identical bits
    assert not any(bool(torch.isnan(a[k]).any()) for k in a)
    assert same_bits(nhwc_to_nchw(a['nhwc'], 4), a['nchw']) and same_bits(a['nhwc'][..., 4:], torch.zeros(3, 16, 24, 4))
    no_terms = run(pred, hr, Cp=4, scale=sc, clamp_target=True, grad_weight=0.6, terms=False, **kw)
    assert same_bits(no_terms['lo'], a['lo']) and same_bits(no_terms['nhwc'], a['nhwc'][..., :4].contiguous())
    # the ratio, the target clamp and grad_weight against the restatement; the plain L1 sums in float like l1_clamp_kernel, whose longest
    # chain here is 4 channels + the LDS tree 8 + the finish 1 + 6 + 3 crops = 22 additions (tests/test_gpu_misc.py)
    ref = R.closed_form(pred, hr, scale=sc, clamp_target=True, grad_weight=0.6, **kw)
    assert abs(float(a['lo'][0]) - ref['loss']) <= 24 * U * ref['loss']
    assert np.all(np.abs(a['lo'][1:].double().numpy() - ref['sse']) <= 32 * U * ref['sse'])
    if not kw.get('charbonnier'):
        want = R.l1_family_expected(ref, grad_weight=0.6, scale=sc, grad=kw.get('grad', 0.0), pyramid=kw.get('pyramid', False))
        differ = a['nchw'].numpy().view(np.int32) != want.view(np.int32)
        assert not (differ & ~ref['fragile']).any() and ref['fragile'].mean() <= FRAGILE_CAP
    else:
        assert np.abs(a['nchw'].double().numpy() - ref['grad']).max() <= (16 + 8 * 1000) * U * ref['coef'].max()
    pred[1, 2, 7, 9] = NAN                                            # a NaN prediction: a NaN loss; the other crops' SSE untouched
    n = run(pred, hr, Cp=8, scale=sc, clamp_target=True, grad_weight=0.6, **kw)
    assert math.isnan(float(n['lo'][0])) and math.isnan(float(n['lo'][2]))
    assert same_bits(n['lo'][[1, 3]], a['lo'][[1, 3]])


def test_refusals_leave_every_output_untouched():
    """PNNP_E_INVALID (-1) / PNNP_E_WORKSPACE (-4) straight from the C entry, before any launch: every output still holds its sentinel."""
    from pnnp_amd import ops
    fn = ops._tile_fn('pnnp_unet_loss_f32')
    B, Cc, H, W = 2, 4, 16, 24
    pred = torch.rand(B, Cc, H, W, device=DEV); hr = torch.rand(B, Cc, H, W, device=DEV)
    n_ws = ops.unet_loss_workspace_floats(B)
    assert n_ws == 768 * B
    outs = dict(g=torch.full((B, H, W, 8), 7.0, device=DEV), gn=torch.full((B, Cc, H, W), 7.0, device=DEV), lo=torch.full((1 + B,), 7.0, device=DEV),
                tm=torch.full((5,), 7.0, device=DEV), ws=torch.full((n_ws + 1,), 7.0, device=DEV))

    def call(pred=pred, hr=hr, Cc=Cc, H=H, W=W, Cp=8, ws=outs['ws'], n=n_ws, ct=0, cpd=1, gw=1.0, ch=0, py=0, gl=0.0, recon=1, lo=outs['lo']):
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        return fn(p(pred), p(hr), p(None), p(outs['g']), p(outs['gn']), p(lo), p(outs['tm']), B, Cc, H, W, Cp, p(ws), C.c_int64(n), ct, cpd,
                  C.c_float(gw), ch, py, C.c_float(gl), recon, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    refused = dict(null_pred=call(pred=None), null_loss=call(lo=None), null_ws=call(ws=None), c9=call(Cc=9), c0=call(Cc=0), cp12=call(Cp=12), cp_lt_c=call(Cc=8, Cp=4),
                   h0=call(H=0), flag2=call(ch=2), flag_neg=call(py=-1), recon2=call(recon=2), gl_neg=call(gl=-0.5), gl_nan=call(gl=NAN), gl_inf=call(gl=float('inf')),
                   pyramid_with_edge=call(py=1, gl=0.5), pyramid_h12=call(py=1, H=12), pyramid_w20=call(py=1, W=20), nothing=call(recon=0),
                   pyramid_pred_off_16=call(py=1, pred=pred.view(-1)[1:]), ws_off_8=call(ws=outs['ws'][1:]))
    assert all(v == -1 for v in refused.values()), refused
    assert call(n=n_ws - 1) == -4
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 7.0).all()), k
    assert call(py=1, ch=1) == 0                                      # and the same arguments without a fault go through
    torch.cuda.synchronize()
    assert not bool((outs['g'] == 7.0).any()) and not bool((outs['lo'] == 7.0).any())


# ------------------------------------------------------------------------------------------------ losses.Unet_Loss
@pytest.mark.parametrize('c,p', MODES)
def test_module_forward_backward(golden, c, p):
    """losses.Unet_Loss(charbonnier)(low, high, pyramid) and .backward() on CUDA, no clamp inside, against the restatement.  Bars from the formats:
    a term is a mean (carried in double) of float32 elements whose d carries <= 8 x 2^-24 absolute error (values <= 1.4, three poolings, the
    subtraction) through a 1-Lipschitz f; the Charbonnier derivative has slope <= 1000; the L1 family is exact off the fragile elements."""
    from pnnp_amd import _lib, losses
    g, _ = golden
    pred, hr = g['c_pred'], g['c_hr']
    ref = ref_of(golden, 'c', charbonnier=bool(c), pyramid=bool(p), clamp_pred=False)
    low = torch.from_numpy(pred).to(DEV).requires_grad_(True)
    crit = losses.Unet_Loss(charbonnier=bool(c))
    loss = crit(low, torch.from_numpy(hr).to(DEV), pyramid=bool(p))
    assert loss.shape == () and abs(float(loss) - ref['loss']) <= 8 * U * 1.4
    assert np.all(np.abs(crit.terms.cpu().double().numpy() - ref['terms']) <= 8 * U * 1.4)
    (loss * 2.0).backward()
    got = low.grad.cpu().numpy()
    if c:
        assert np.abs(got.astype(np.float64) - 2 * ref['grad']).max() <= 2 * (16 + 8 * 1000) * U * ref['coef'].max()
    else:
        want = R.l1_family_expected(ref, pyramid=bool(p)) * np.float32(2.0)
        differ = got.view(np.int32) != want.view(np.int32)
        assert not (differ & ~ref['fragile']).any() and ref['fragile'].mean() <= FRAGILE_CAP
    if c and not p:
        l2 = losses.L1_Charbonnier_loss()(low.detach(), torch.from_numpy(hr).to(DEV))
        assert same_bits(l2.cpu(), loss.detach().cpu())
    with pytest.raises(_lib.PnnpError):
        crit(torch.from_numpy(pred), torch.from_numpy(hr))


def test_module_grad_loss(golden):
    from pnnp_amd import losses
    g, _ = golden
    for tag in ('f', 'c'):
        pred, hr = g[f'{tag}_pred'], g[f'{tag}_hr']
        ref = ref_of(golden, tag, grad=1.0, recon=False, clamp_pred=False)
        low = torch.from_numpy(pred).to(DEV).requires_grad_(True)
        loss = losses.Unet_Loss().grad_loss(low, torch.from_numpy(hr).to(DEV))
        assert abs(float(loss) - ref['loss']) <= 4 * U * ref['loss']
        loss.backward()
        differ = low.grad.cpu().numpy().view(np.int32) != R.l1_family_expected(ref, grad=1.0).view(np.int32)
        assert not (differ & ~ref['fragile']).any() and ref['fragile'].mean() <= FRAGILE_CAP


# ------------------------------------------------------------------------------------------------ HipTrainStep(loss=)
def _unet(sd):
    from pnnp_amd.archs import UNetSeeInDark
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=8, in_nc=4, out_nc=4))
    net.load_state_dict({k: v.clone() for k, v in sd.items()})
    return net.cuda()


def _step_by_hand(net, x, t, lr, loss_kw):
    """engine.forward, the loss op, engine.backward, ops.adam_step: what HipTrainStep.step composes -> (loss tensor, terms)"""
    from pnnp_amd import ops
    e = net.engine
    dev = x.device
    B, _, H, W = t.shape
    e.params.ensure(dev)
    m, v = torch.zeros_like(e.params.flat), torch.zeros_like(e.params.flat)
    pred = e.forward(x, True)
    gch = e.grad_out_channels(B, H, W)
    g8 = torch.full((B, H, W, gch), NAN, device=dev)
    lo = torch.full((1 + B,), NAN, device=dev)
    terms = None
    if loss_kw is None:
        ops.l1_clamp_loss(pred, t, g8, lo, torch.empty(128 * B, device=dev), scale=None, clamp_target=False, grad_weight=1.0)
    else:
        terms = torch.full((5,), NAN, device=dev)
        ops.unet_loss(pred, t, g8, lo, torch.empty(ops.unet_loss_workspace_floats(B), device=dev), clamp_pred=True, terms=terms, **loss_kw)
    e.backward(g8)
    ops.adam_step(e.params.flat, e.params.grad, m, v, lr, 1, grad_scale=1.0)
    e.mark_dirty()
    return lo, terms


@pytest.mark.parametrize('loss_kw', [None, dict(pyramid=True, charbonnier=True)], ids=['default', 'charbonnier-pyramid'])
def test_train_step_is_the_composition_by_hand(loss_kw):
    """UNet nf = 8 on 1 x 4 x 32 x 32.  loss=None runs the parent's step (composed here with ops.l1_clamp_loss), a mapping routes to ops.unet_loss:
    loss tensor and updated weights bit for bit; the Charbonnier-pyramid loss against oracle.net_torch.unet_forward + the restatement within 5e-6,
    the bar tests/test_gpu_unet.py applies to the nf = 8 L1 step's loss; loss_terms recombine to the loss with the level weights."""
    from oracle import net_torch as O
    from pnnp_amd.trainer import HipTrainStep
    sd = O.init_state(O.unet_param_shapes(nf=8), seed=42)
    gen = torch.Generator().manual_seed(5)
    x, t = torch.rand(1, 4, 32, 32, generator=gen), torch.rand(1, 4, 32, 32, generator=gen)
    a, b = _unet(sd), _unet(sd)
    ts = HipTrainStep(a, lr=1e-3, clip=0, loss=loss_kw)
    lo = ts.step(t.cuda(), noisy=x.cuda())
    lo_hand, terms_hand = _step_by_hand(b, x.cuda(), t.cuda(), 1e-3, loss_kw)
    torch.cuda.synchronize()
    assert same_bits(lo.cpu(), lo_hand.cpu()), (lo, lo_hand)
    assert same_bits(a.engine.params.flat.cpu(), b.engine.params.flat.cpu())
    fresh = _unet(sd)
    fresh.engine.params.ensure(torch.device('cuda', torch.cuda.current_device()))
    assert not same_bits(a.engine.params.flat.cpu(), fresh.engine.params.flat.cpu())          # and the step did move the weights
    with torch.no_grad():
        pred = O.unet_forward(sd, x)
    if loss_kw is None:
        assert ts.loss_terms is None
        assert abs(float(lo[0]) - float(O.l1_clamp_loss(pred, t))) < 5e-6
        return
    ref = R.closed_form(pred.numpy(), t.numpy(), **loss_kw)
    print(f'charbonnier-pyramid step: loss {float(lo[0]):.8f}, oracle + restatement {ref["loss"]:.8f}, diff {abs(float(lo[0]) - ref["loss"]):.3e}')
    assert abs(float(lo[0]) - ref['loss']) < 5e-6
    assert same_bits(ts.loss_terms.cpu(), terms_hand.cpu())
    tm = ts.loss_terms.cpu().numpy()
    assert tm.dtype == np.float32 and tm[4] == 0
    assert float(recombine(tm)) == float(lo[0])
    assert np.all(np.abs(tm[:4] - ref['terms'][:4]) < 5e-6)
    ps = HipTrainStep.psnr_from(lo, t[0].numel())                    # the SSE slots keep serving the PSNR
    assert abs(ps - float(-10 * torch.log10(((pred.clamp(0, 1) - t) ** 2).mean()))) < 2e-3


def test_train_step_refuses_an_odd_crop_under_the_pyramid():
    from oracle import net_torch as O
    from pnnp_amd import _lib
    from pnnp_amd.trainer import HipTrainStep
    net = _unet(O.init_state(O.unet_param_shapes(nf=8), seed=42))
    with pytest.raises(_lib.PnnpError):
        HipTrainStep(net, loss=dict(pyramid=True, grad=1.0))
    ts = HipTrainStep(net, lr=1e-3, clip=0, loss=dict(grad=0.5))      # the edge term has no size rule: 16 x 16 trains
    lo = ts.step(torch.rand(1, 4, 16, 16, device=DEV), noisy=torch.rand(1, 4, 16, 16, device=DEV))
    assert math.isfinite(float(lo[0])) and float(ts.loss_terms[4]) > 0
