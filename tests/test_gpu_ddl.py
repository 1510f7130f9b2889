"""The distribution losses on the device (csrc/ddl.hip; losses.CDFPPF / CDFLoss / KLD, NoiseFlowFitStep.ddl) against the sort-based
restatement (tests/_ddl_ref.py, pinned to the reference by tests/test_host_ddl.py) run on the CPU.

Pass conditions:
  cdf         bitwise equal to the float32 restatement: every operation is one IEEE add, subtract, divide or int -> float conversion.
  CDFLoss     within 2^-23 relative of the float64 mean of the (bit-equal) float32 terms -- the device sums in float64 and rounds once --
              and within K 2^-24 relative of the restatement's float32 value (the bound of a float32 sum of K non-negative terms).
  gradients, KLD value
              E_ref = max|f32 - f64| / max|f64| of the restatement's own CPU autograd, float32 against float64, on the same inputs; the
              device's same measure against float64 must be <= 4 E_ref + 2^-23 (another summation order and the device's log; one
              float32 rounding of the result).  With ties the gradients are compared summed per distinct value, and the lowest index
              of a value must hold them.
"""
import numpy as np
import pytest
import torch

from pnnp_amd import _lib, losses
from tests import _ddl_ref as R

pytestmark = pytest.mark.gpu

NS = [2, 63, 64, 65, 4097, 16387, 2 ** 20 + 5]
KS = [1, 2, 64, 1000, 4096]
DATA = ['distinct', 'ties', 'const', 'zeros']
POINTS = ['below', 'above', 'straddle', 'data', 'ends', 'repeat']
EPS = 2.0 ** -23


def make_data(kind, n, seed):
    rng = np.random.default_rng([seed, n])
    if kind == 'distinct':                                     # a scaled permutation: exact in float32, every value once
        return ((rng.permutation(n) - n // 2) / 64.0).astype(np.float32)
    if kind == 'ties':
        return np.rint(rng.normal(0, 3.0, n)).astype(np.float32)
    if kind == 'const':
        return np.full(n, 1.25, np.float32)
    if kind == 'zeros':                                        # -0.0 and +0.0 are one value; with and without other values around them
        return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0] if seed % 2 else [-0.0, 0.0], np.float32), n).astype(np.float32)
    raise KeyError(kind)


def make_points(kind, d, k, seed):
    rng = np.random.default_rng([seed, k, d.size])
    lo, hi = float(d.min()), float(d.max())
    if kind == 'below':
        x = np.linspace(lo - 3.0, lo - 1.0, k)
    elif kind == 'above':
        x = np.linspace(hi + 1.0, hi + 3.0, k)
    elif kind == 'straddle':
        x = np.linspace(lo - 1.0, hi + 1.0, k) if k > 1 else np.array([(lo + hi) / 2 + 0.01])
    elif kind == 'data':                                       # points equal to data values (repeated where K > N)
        x = rng.choice(d, k, replace=k > d.size)
    elif kind == 'ends':                                       # the minimum and the maximum themselves
        x = np.where(np.arange(k) < (k + 1) // 2, lo, hi)
    elif kind == 'repeat':
        x = rng.choice(np.array([lo - 0.5, (lo + hi) / 2, (lo + 3 * hi) / 4 + 0.003, hi]), k)
    else:
        raise KeyError(kind)
    return np.sort(x.astype(np.float32))


def on_device(a, offset=0):
    """a copy on the GPU that starts ``offset`` elements after a 16-byte boundary"""
    buf = torch.empty(a.size + 4, dtype=torch.float32, device='cuda')
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * offset
    return view


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cpu_cdf(d, x):
    return R.ecdf(torch.from_numpy(d), torch.from_numpy(x)).numpy()


def brackets_by_sort(d, x):
    """arg hi / arg lo of distinct data"""
    order = np.argsort(d, kind='stable')
    s = d[order]
    idx = np.searchsorted(s, np.clip(x, s[0], s[-1]), side='left')
    return order[idx], np.where(idx > 0, order[np.maximum(idx - 1, 0)], -1)


def first_index_of_value(d):
    """for every element: the lowest index that holds its value (-0.0 and +0.0 are one value)"""
    _, first, inv = np.unique(d + np.float32(0), return_index=True, return_inverse=True)
    return first[inv]


def check_cdf(d, x, offset):
    want = cpu_cdf(d, x)
    dd, xx = on_device(d, offset), torch.from_numpy(x).cuda()
    keep = dd.clone()
    got, br = losses.ecdf_with_brackets(dd, xx)
    got2 = losses.CDFPPF(dd).get_cdf(xx)
    got, got2, br = got.cpu().numpy(), got2.cpu().numpy(), br.cpu().numpy()
    assert torch.equal(dd, keep)
    where = (d.size, x.size, offset)
    assert np.array_equal(bits(got), bits(want)), (where, np.abs(got - want).max())
    assert np.array_equal(bits(got2), bits(want)), where
    k = x.size
    arg_hi, arg_lo, amin, amax = br[:k], br[k:2 * k], br[2 * k], br[2 * k + 1]
    first = first_index_of_value(d)
    xc = np.clip(x, d.min(), d.max())
    # the brackets hold the right values, and the lowest index of those values
    assert d[amin] == d.min() and d[amax] == d.max() and first[amin] == amin and first[amax] == amax, where
    assert np.all(d[arg_hi] >= xc) and np.array_equal(first[arg_hi], arg_hi), where
    has = arg_lo >= 0
    assert np.all(d[arg_lo[has]] < xc[has]) and np.array_equal(first[arg_lo[has]], arg_lo[has]), where
    assert np.array_equal(has, xc > d.min()), where
    if np.unique(d).size == d.size:
        want_hi, want_lo = brackets_by_sort(d, x)
        assert np.array_equal(arg_hi, want_hi) and np.array_equal(arg_lo, want_lo), where


@pytest.mark.parametrize('n', NS[:-1])
def test_cdf_is_bitwise_the_restatement(n):
    """Every data kind x K x kind of points, from an aligned start and from one element past it."""
    for di, data in enumerate(DATA):
        for seed in ((0, 1) if data == 'zeros' else (0,)):
            d = make_data(data, n, seed)
            for k in KS:
                for pi, pts in enumerate(POINTS):
                    check_cdf(d, make_points(pts, d, k, seed), (di + pi + k) % 2)


@pytest.mark.parametrize('data', DATA)
def test_cdf_is_bitwise_where_many_workgroups_share_a_bin(data):
    """N = 2^20 + 5: every workgroup merges into the same few bins at K = 1 and 2, into all of them at K = 4096."""
    n = NS[-1]
    d = make_data(data, n, 1)
    for k, pts, off in ((1, 'straddle', 1), (2, 'data', 0), (64, 'repeat', 1), (1000, 'straddle', 0), (4096, 'straddle', 1), (4096, 'data', 0)):
        check_cdf(d, make_points(pts, d, k, 1), off)


# (n_output, n_gt, data, K, points): different lengths; more than one block; odd sizes; ties; the largest K; the smallest N and K
LOSS_CASES = [(4097, 16387, 'distinct', 64, 'straddle'), (65, 63, 'distinct', 64, 'data'), (16387, 4097, 'ties', 64, 'straddle'),
              (2 ** 20 + 5, 4097, 'distinct', 1000, 'straddle'), (64, 2, 'distinct', 2, 'data'), (4097, 4099, 'distinct', 4096, 'straddle'),
              (4097, 65, 'zeros', 64, 'straddle'), (63, 4097, 'const', 64, 'straddle'), (16387, 16385, 'ties', 1000, 'repeat'),
              (4097, 4097, 'distinct', 64, 'ends'), (4097, 2 ** 20 + 5, 'distinct', 64, 'below')]
_loss_cache = {}


def loss_case(case):
    """inputs and the restatement's CPU results (computed once, shared, left unchanged)"""
    if case not in _loss_cache:
        n_o, n_g, data, k, pts = case
        o = make_data(data, n_o, 1)
        g = make_data('distinct' if data == 'const' else data, n_g, 3) * np.float32(0.5) + np.float32(0.25 if data != 'zeros' else 0.0)
        both = np.concatenate([o, g])
        x = make_points(pts, o if pts in ('data', 'ends') else both, k, 5)
        ref = {}
        for kind in ('cdf', 'kld'):
            if kind == 'kld' and k < 2:
                continue
            ref[kind] = (R.loss_and_grads(kind, o, g, x, torch.float32), R.loss_and_grads(kind, o, g, x, torch.float64))
        _loss_cache[case] = (o, g, x, ref)
    return _loss_cache[case]


def per_value(d, grad):
    _, inv = np.unique(d + np.float32(0), return_inverse=True)
    return np.bincount(inv, np.asarray(grad, np.float64))


def device_loss(kind, o, g, x, offset=1):
    do, dg = on_device(o, offset).requires_grad_(True), on_device(g, 1 - offset).requires_grad_(True)
    loss = (losses.CDFLoss if kind == 'cdf' else losses.KLD)(do, dg, torch.from_numpy(x).cuda())
    loss.backward()
    return loss.detach().cpu().numpy(), do.grad.cpu().numpy(), dg.grad.cpu().numpy()


@pytest.mark.parametrize('case', LOSS_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_cdf_loss_value(case):
    o, g, x, ref = loss_case(case)
    got, _, _ = device_loss('cdf', o, g, x)
    terms = np.abs(cpu_cdf(o, x) - cpu_cdf(g, x))              # float32 terms, bit-equal on the device (tested above)
    exact = terms.astype(np.float64).mean()
    f32 = ref['cdf'][0][0]
    print(case, 'device', float(got), 'f64 mean of f32 terms', exact, 'restatement f32', f32)
    assert got.dtype == np.float32 and got.shape == ()
    assert abs(float(got) - exact) <= EPS * exact
    assert abs(float(got) - f32) <= x.size * 2.0 ** -24 * abs(f32)


@pytest.mark.parametrize('kind', ['cdf', 'kld'])
@pytest.mark.parametrize('case', LOSS_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_gradients_and_kld_value(case, kind):
    o, g, x, ref = loss_case(case)
    if kind not in ref:
        with pytest.raises(_lib.PnnpError):                    # the KLD of one point has no difference
            device_loss(kind, o, g, x)
        return
    (l32, go32, gg32), (l64, go64, gg64) = ref[kind]
    l_dev, go_dev, gg_dev = device_loss(kind, o, g, x)
    for name, d, dev, f32, f64 in (('output', o, go_dev, go32, go64), ('gt', g, gg_dev, gg32, gg64)):
        assert np.all(np.isfinite(dev)), name
        nz = np.nonzero(dev)[0]
        assert np.array_equal(first_index_of_value(d)[nz], nz), name            # among equal samples the lowest index holds the gradient
        dev, f32, f64 = per_value(d, dev), per_value(d, f32), per_value(d, f64)
        top = np.abs(f64).max()
        if top == 0:
            assert not dev.any() and not f32.any(), name
            continue
        e_ref, e_dev = np.abs(f32 - f64).max() / top, np.abs(dev - f64).max() / top
        print(case, kind, name, 'E_ref', e_ref, 'E_dev', e_dev, 'max|grad|', top)
        assert e_dev <= 4 * e_ref + EPS, (name, e_dev, e_ref)
    if kind == 'kld' and l64 == 0:
        assert float(l_dev) == 0 and l32 == 0
    elif kind == 'kld':
        e_ref, e_dev = abs(l32 - l64) / abs(l64), abs(float(l_dev) - l64) / abs(l64)
        print(case, 'KLD', float(l_dev), 'f32', l32, 'f64', l64, 'E_ref', e_ref, 'E_dev', e_dev)
        assert e_dev <= 4 * e_ref + EPS, (e_dev, e_ref)


@pytest.mark.parametrize('kind', ['cdf', 'kld'])
def test_two_calls_give_identical_bits_and_leave_the_inputs_alone(kind):
    o, g, x, _ = loss_case(LOSS_CASES[3])
    do, dg, dx = on_device(o, 1), on_device(g, 0), torch.from_numpy(x).cuda()
    keep = (do.clone(), dg.clone(), dx.clone())
    runs = []
    for _ in range(2):
        a, b = do.detach().requires_grad_(True), dg.detach().requires_grad_(True)
        loss = (losses.CDFLoss if kind == 'cdf' else losses.KLD)(a, b, dx)
        (loss * 3.0).backward()
        runs.append((loss.detach().clone(), a.grad.clone(), b.grad.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    assert runs[0][1].abs().max() > 0 and runs[0][2].abs().max() > 0
    for u, v in zip((do, dg, dx), keep):
        assert torch.equal(u, v)


def test_only_the_operand_that_requires_grad_gets_one():
    o, g, x, _ = loss_case(LOSS_CASES[0])
    do, dg = on_device(o).requires_grad_(True), on_device(g)
    losses.CDFLoss(do, dg, torch.from_numpy(x).cuda()).backward()
    assert do.grad is not None and dg.grad is None
    do, dg = on_device(o), on_device(g).requires_grad_(True)
    losses.KLD(do, dg, torch.from_numpy(x).cuda()).backward()
    assert do.grad is None and dg.grad is not None


def test_shapes_strides_and_unsorted_points():
    """Inputs are flattened like .view(-1); non-contiguous inputs are accepted; points that are not ascending are sorted and un-permuted."""
    o, g, x, ref = loss_case(LOSS_CASES[0])
    o, g = o[:4096], g[:16384]
    wide = torch.zeros(64, 128, device='cuda')
    wide[:, ::2] = torch.from_numpy(o).cuda().view(64, 64)
    do = wide[:, ::2]                                          # [64, 64], stride 2
    assert not do.is_contiguous()
    dg = torch.from_numpy(g).cuda().view(4, 64, 64)
    perm = np.random.default_rng(9).permutation(x.size)
    xp = torch.from_numpy(x[perm]).cuda()
    want = cpu_cdf(o, x)
    got = losses.CDFPPF(do).get_cdf(xp.view(8, 8))
    assert got.shape == (8, 8) and np.array_equal(bits(got.cpu().numpy().reshape(-1)), bits(want[perm]))
    do = do.detach().requires_grad_(True)
    for kind, fn in (('cdf', losses.CDFLoss), ('kld', losses.KLD)):
        l32, go32, _ = R.loss_and_grads(kind, o, g, x[perm], torch.float32)
        do.grad = None
        loss = fn(do, dg, xp)
        loss.backward()
        assert do.grad.shape == (64, 64)
        loss = float(loss.detach())
        assert abs(loss - l32) <= 1e-5 * abs(l32), (kind, loss, l32)
        assert np.abs(do.grad.cpu().numpy().reshape(-1) - go32).max() <= 1e-5 * np.abs(go32).max(), kind
    pdf = losses.cdf2pdf(torch.from_numpy(want).cuda()).cpu().numpy()
    assert np.array_equal(pdf, np.abs(want[:-1] - want[1:]))


def test_refusals():
    d = torch.zeros(4097, device='cuda')
    with pytest.raises(_lib.PnnpError, match='4097 points'):
        losses.CDFPPF(d).get_cdf(torch.linspace(0, 1, 4097, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='4097 points'):
        losses.CDFLoss(d, d, torch.linspace(0, 1, 4097, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='1 points'):
        losses.KLD(d, d, torch.zeros(1, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='float32'):
        losses.CDFLoss(d.double(), d, torch.linspace(0, 1, 8, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='float32'):
        losses.CDFLoss(d, d, torch.linspace(0, 1, 8, device='cuda').double())
    with pytest.raises(_lib.PnnpError, match='1 samples'):
        losses.CDFLoss(d[:1], d, torch.linspace(0, 1, 8, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.CDFLoss(d, d, torch.linspace(0, 1, 8))


def test_adam_on_the_cdf_loss_fits_a_scale_and_a_shift():
    """scale * z + shift with fixed z, from (1, 0), 200 Adam steps on CDFLoss against a N(0.3, 1.5^2) sample: the loss must fall below a tenth
    of its start and both parameters must end closer to (1.5, 0.3).  The same run through the restatement on the device must reach the
    same loss within the gradient tolerance 4 E_ref + 2^-23 (E_ref: the restatement's CPU float32 against float64 gradient at the start)
    accumulated over the steps -- steps x tolerance, relative to the starting loss."""
    steps, n, k = 200, 65536, 256
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(n, generator=gen)
    target = 0.3 + 1.5 * torch.randn(n, generator=gen)
    x = torch.linspace(float(target.min()), float(target.max()), k)
    _, g32, _ = R.loss_and_grads('cdf', z, target, x, torch.float32)
    _, g64, _ = R.loss_and_grads('cdf', z, target, x, torch.float64)
    e_ref = np.abs(g32 - g64).max() / np.abs(g64).max()
    z, target, x = z.cuda(), target.cuda(), x.cuda()

    def fit(loss_fn):
        p = torch.tensor([1.0, 0.0], device='cuda', requires_grad=True)
        opt = torch.optim.Adam([p], lr=0.01)
        trace = []
        for _ in range(steps):
            opt.zero_grad()
            loss = loss_fn(p[0] * z + p[1], target, x)
            loss.backward()
            opt.step()
            trace.append(loss.detach())
        with torch.no_grad():
            trace.append(loss_fn(p[0] * z + p[1], target, x))
        return torch.stack(trace).cpu().numpy(), p.detach().cpu().numpy()

    ours, p = fit(lambda a, b, c: losses.CDFLoss(a, b, c, assume_sorted=True))
    theirs, q = fit(R.cdf_loss)
    tol = steps * (4 * e_ref + EPS) * ours[0]
    print('start', ours[0], 'end', ours[-1], 'parameters', p, '| restatement end', theirs[-1], q, '| E_ref', e_ref, 'tolerance', tol,
          'difference', abs(ours[-1] - theirs[-1]))
    assert ours[-1] < ours[0] / 10
    assert abs(p[0] - 1.5) < 0.5 and abs(p[1] - 0.3) < 0.3
    assert abs(ours[-1] - theirs[-1]) <= tol


def test_noiseflow_fit_step_ddl():
    """NoiseFlowFitStep.ddl compares the pair that score draws at the same counters (host RNG, net.offset): it equals the losses called
    on the returned tensors of score."""
    from pnnp_amd.archs import NoiseFlow
    from pnnp_amd.trainer import NoiseFlowFitStep
    np.random.seed(3); torch.manual_seed(3)
    net = NoiseFlow({'x_shape': (4, 64, 64), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'}).cuda()
    fs = NoiseFlowFitStep(net, camera_type='SonyA7S2', noise_code='pgrq', clip=2)
    hr = (torch.rand(2, 4, 64, 64, generator=torch.Generator().manual_seed(16)) * 0.3).cuda()
    with pytest.raises(_lib.PnnpError, match='kind'):
        fs.ddl(hr, kind='quantile')
    for kind in ('cdf', 'kld'):
        np.random.seed(4); torch.manual_seed(4)
        offset = net.offset                      # NoiseFlow.sample draws from a counter-based generator and advances this counter
        got = fs.ddl(hr, iso=1600, kind=kind)
        assert net.training and fs.step_count == 0 and net.offset == offset + 1
        np.random.seed(4); torch.manual_seed(4)
        net.offset = offset                      # the same prior draw for score
        _, (hr_used, real, sampled) = fs.score(hr, iso=1600, return_tensors=True)
        noise = real - hr_used
        x = noise.min() + losses.get_x(size=1000, mode='uniform').cuda() * (noise.max() - noise.min())
        want = (losses.CDFLoss if kind == 'cdf' else losses.KLD)(sampled, noise, x)
        assert got.shape == () and got.is_cuda and torch.isfinite(got)
        assert torch.equal(got, want), (kind, float(got), float(want))
