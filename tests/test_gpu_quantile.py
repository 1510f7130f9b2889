"""QuantileLoss on the device (csrc/quantile.hip; losses.quantile / QuantileLoss, NoiseFlowFitStep.qloss / qloss_step) against the
reference's outputs (tests/golden/quantile.npz), CPU torch.quantile and the sort-based restatement (tests/_quantile_ref.py, pinned to
the reference by tests/test_host_quantile.py).

Pass conditions:
  order statistics s[lo], s[hi], the weights w and the elements that hold them
              exact (compared with ==: -0.0 equals +0.0); the element is the lowest index of its value.
  values      within BAND = 4 * 2^-24 * max(|s_lo|, |s_hi|) of the reference's value and of the float64 evaluation with the same float32 w:
              each side is at most three float32 roundings of that magnitude.  (A float32 rounding is never finer than 2^-150, half the
              spacing of the subnormals, so the band is 4 * max(2^-24 max(|s_lo|, |s_hi|), 2^-150): the floor matters for the subnormal case
              only, where the reference itself is 0.495 * 2^-149 away from float64.)  Where an order statistic is infinite the value must be the
              reference's (NaN where it is NaN).
  loss        within 2^-24 relative (one float32 rounding: the device sums in float64) of the float64 mean of the device's own quantile
              differences, and within the mean band of both operands plus K R 2^-24 relative (a float32 sum) of the reference's loss.
  gradients   E_ref = max|f32 - f64| / max|f64| of the restatement's CPU autograd; the device's same measure against float64 must be
              <= 4 E_ref + 2^-23, and the non-zero entries must be float64 autograd's.  With ties the gradients are compared summed per
              distinct value, and the lowest index of a value must hold them.
"""
import os

import numpy as np
import pytest
import torch

from pnnp_amd import _lib, losses
from tests import _quantile_ref as R

pytestmark = pytest.mark.gpu

CASES = ['normal', 'edges', 'ties', 'rows', 'tiny1', 'tiny2', 'tiny3']
EPS = 2.0 ** -23
MAX_K = losses.QUANTILE_MAX_K


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'quantile.npz'))


def on_device(a, offset=0):
    """a copy on the GPU whose first element lies ``offset`` elements after a 16-byte boundary"""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device='cuda')
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    assert view.data_ptr() % 16 == 4 * offset
    return view.view(a.shape)


def rows_of(a):
    return a.reshape(-1, a.shape[-1])


def band_of(a, b):
    with np.errstate(invalid='ignore'):
        return 4 * np.maximum(2.0 ** -24 * np.maximum(np.abs(a), np.abs(b)).astype(np.float64), 2.0 ** -150)


def check_values(got, want, a, b, w, where):
    """one row: device values against the reference's values ``want`` and the float64 evaluation; -> the band"""
    band = band_of(a, b)
    fin = np.isfinite(a) & np.isfinite(b)
    exact = R.value_from(a, b, w, np.float64)
    g64 = got.astype(np.float64)
    assert np.all(np.abs(g64[fin] - want[fin]) <= band[fin]), (where, np.abs(g64[fin] - want[fin]).max())
    assert np.all(np.abs(g64[fin] - exact[fin]) <= band[fin]), where
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), where
    print(where, 'bit-equal to the reference:', int((got[fin] == want[fin]).sum()), 'of', int(fin.sum()))
    return band


def check_select(d, q, want=None, offset=0):
    """quantile_with_state of ``d`` [N] or [R, N] (numpy) at ``q``: order statistics, weights and elements exact, the values against
    ``want`` (default: CPU torch.quantile).  -> (device values [K, R], the band [K, R])"""
    d, q = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(q, np.float32)
    if want is None:
        want = torch.quantile(torch.from_numpy(d), torch.from_numpy(q), dim=-1, interpolation='linear').numpy()
    dd, dq = on_device(d, offset), torch.from_numpy(q).cuda()
    keep = dd.clone()
    values, arg, w = losses.quantile_with_state(dd, dq)
    values, arg, w = values.cpu().numpy(), arg.cpu().numpy(), w.cpu().numpy()
    assert torch.equal(dd, keep)
    rows = rows_of(d)
    assert values.shape == (q.size, rows.shape[0]) and arg.shape == (2, rows.shape[0], q.size)
    want = want.reshape(q.size, rows.shape[0])
    bands = np.zeros(values.shape)
    for r, row in enumerate(rows):
        a, b, alo, ahi, wref = R.order_stats(row, q)
        where = (d.shape, q.size, offset, r)
        assert arg[:, r].min() >= 0 and arg[:, r].max() < row.size, where
        assert np.all(row[arg[0, r]] == a) and np.all(row[arg[1, r]] == b), where
        assert np.array_equal(arg[0, r], alo) and np.array_equal(arg[1, r], ahi), where
        assert np.array_equal(w.view(np.uint32), wref.view(np.uint32)), where
        bands[:, r] = np.nan_to_num(check_values(values[:, r], want[:, r], a, b, wref, where), nan=0.0, posinf=0.0)
    return values, bands


# ------------------------------------------------------------------------------------------------------------ 1. golden cases
@pytest.mark.parametrize('case', CASES)
def test_golden_cases(golden, case):
    g = golden
    o, t, q = g[case + '_out'], g[case + '_gt'], g[case + '_q']
    vo, bo = check_select(o, q, g[case + '_q_out'], offset=1)
    vt, bt = check_select(t, q, g[case + '_q_gt'], offset=0)
    loss = losses.QuantileLoss(on_device(o, 0), on_device(t, 1), torch.from_numpy(q).cuda())
    assert loss.shape == () and loss.is_cuda and loss.dtype == torch.float32
    loss = float(loss)
    exact = np.abs(vo.astype(np.float64) - vt.astype(np.float64)).mean()
    ref = float(g[case + '_loss'])
    print(case, 'device', loss, 'f64 mean of the device quantiles', exact, 'reference', ref)
    assert abs(loss - exact) <= 2.0 ** -24 * exact
    assert abs(loss - ref) <= (bo + bt).mean() + vo.size * 2.0 ** -24 * abs(ref) + 2.0 ** -24 * exact


# ------------------------------------------------------------------------------------------------------------ 2. digit and tile boundaries
def boundary_data(kind):
    rng = np.random.default_rng([11, len(kind)])
    u32 = lambda v: np.float32(v).view(np.uint32)
    if kind == 'low10':                                        # keys that differ only in their lowest 10 bits
        return (u32(1.5) + rng.integers(0, 1024, 5000).astype(np.uint32)).view(np.float32)
    if kind == 'mid':                                          # ... only in bits 10..19
        return (u32(1.0) + (rng.integers(0, 1024, 5000).astype(np.uint32) << 10)).view(np.float32)
    if kind == 'sign':                                         # across the sign change, with both zeros
        d = rng.normal(0, 1e-3, 5003).astype(np.float32)
        d[rng.choice(5003, 40, replace=False)] = np.tile(np.array([-0.0, 0.0], np.float32), 20)
        return d
    if kind == 'subnormal':
        bits = rng.integers(0, 1 << 23, 5001).astype(np.uint32) | (rng.integers(0, 2, 5001).astype(np.uint32) << 31)
        return bits.view(np.float32)
    if kind == 'inf':
        d = rng.normal(0, 1, 5000).astype(np.float32)
        d[[7, 4000, 4999]] = np.inf
        d[[0, 2500]] = -np.inf
        return d
    if kind == 'const':
        return np.full(5000, 1.25, np.float32)
    if kind == 'const_long':                                   # one bin longer than the LDS sort takes: the radix select, one key
        return np.full(20001, -2.5, np.float32)
    if kind == 'ties_long':                                    # several such bins, several entries in each
        return np.rint(rng.normal(0, 1.0, 70001)).astype(np.float32)
    if kind == 'outlier':                                      # one far value puts every other sample into the first bin: the radix select, distinct keys
        d = rng.normal(0, 1, 20003).astype(np.float32)
        d[12345] = 1e30
        return d
    raise KeyError(kind)


Q64 = np.concatenate([[0.0, 1.0, 0.5, 0.5], np.random.default_rng(5).uniform(0, 1, 60)]).astype(np.float32)


@pytest.mark.parametrize('kind', ['low10', 'mid', 'sign', 'subnormal', 'inf', 'const', 'const_long', 'ties_long', 'outlier'])
def test_boundaries_against_cpu_torch_quantile(kind):
    check_select(boundary_data(kind), Q64, offset=len(kind) % 4)


def test_unaligned_view_of_more_than_one_block():
    d = np.random.default_rng(12).normal(0, 1, 16384 * 2 + 4).astype(np.float32)
    dd = torch.from_numpy(d).cuda()[1:]
    assert dd.data_ptr() % 16 == 4
    q = torch.from_numpy(Q64).cuda()
    got = losses.quantile(dd, q).cpu().numpy()
    want = torch.quantile(torch.from_numpy(d[1:]), torch.from_numpy(Q64), dim=-1, interpolation='linear').numpy()
    a, b, _, _, w = R.order_stats(d[1:], Q64)
    check_values(got, want, a, b, w, 'view')
    check_select(d[1:], Q64, offset=3)


@pytest.mark.parametrize('n,k', [(5000, 1), (5000, MAX_K), (100, 300)])
def test_k_one_k_max_and_k_above_n(n, k):
    d = np.random.default_rng([13, n]).normal(0, 2, n).astype(np.float32)
    q = np.random.default_rng([14, k]).uniform(0, 1, k).astype(np.float32) if k > 1 else np.array([0.37], np.float32)
    check_select(d, q, offset=1)


# ------------------------------------------------------------------------------------------------------------ 3. the rank rule above 2^24
def test_rank_rule_above_2_to_24():
    """float32(N - 1) is not N - 1 here and q = 1 gives a position that must be clamped.  CPU torch.quantile refuses more than 2^24
    elements ("input tensor is too large"), so the reference is what it is made of, run by hand on the CPU: torch.sort, the ranks from
    torch's own float32 product q * (N - 1), and torch.lerp."""
    n = 2 ** 24 + 5
    d = np.random.default_rng(15).normal(0, 1, n).astype(np.float32)
    q = np.array([0.0, 1.0, 0.5, 0.99999994, 0.123456, 0.75, 1e-7, 0.9], np.float32)
    s = torch.sort(torch.from_numpy(d)).values
    pos = torch.from_numpy(q) * (n - 1)
    tlo, thi = pos.floor().long().clamp(0, n - 1), pos.ceil().long().clamp(0, n - 1)
    want = torch.lerp(s[tlo], s[thi], pos - pos.floor()).numpy()
    values, arg, w = losses.quantile_with_state(torch.from_numpy(d).cuda(), torch.from_numpy(q).cuda())
    values, arg, w = values.cpu().numpy()[:, 0], arg.cpu().numpy()[:, 0], w.cpu().numpy()
    lo, hi, wref = R.ranks(q, n)
    assert np.array_equal(lo, tlo.numpy()) and np.array_equal(hi, thi.numpy()) and hi.max() == n - 1
    assert np.array_equal(w.view(np.uint32), wref.view(np.uint32)) and np.array_equal(wref, (pos - pos.floor()).numpy())
    assert arg.min() >= 0 and arg.max() < n
    a, b = s.numpy()[lo], s.numpy()[hi]
    assert np.all(d[arg[0]] == a) and np.all(d[arg[1]] == b)
    check_values(values, want, a, b, wref, 'N = 2^24 + 5')


# ------------------------------------------------------------------------------------------------------------ 4. gradients
def per_value(d, grad):
    _, inv = np.unique(d + np.float32(0), return_inverse=True)
    return np.bincount(inv, np.asarray(grad, np.float64))


def check_grads(name, d, dev, f32, f64, ties):
    """one operand, all rows"""
    for r, (row, gd, g32, g64) in enumerate(zip(rows_of(d), rows_of(dev), rows_of(f32), rows_of(f64))):
        assert np.all(np.isfinite(gd)), (name, r)
        nz = np.nonzero(gd)[0]
        assert np.array_equal(R.first_index_of_value(row)[nz], nz), (name, r)          # among equal samples the lowest index holds the gradient
        if ties:
            gd, g32, g64 = per_value(row, gd), per_value(row, g32), per_value(row, g64)
        else:
            assert np.array_equal(nz, np.nonzero(g64)[0]), (name, r)
        top = np.abs(g64).max()
        assert top > 0
        e_ref, e_dev = np.abs(g32 - g64).max() / top, np.abs(gd - g64).max() / top
        print(name, 'row', r, 'E_ref', e_ref, 'E_dev', e_dev, 'max|grad|', top)
        assert e_dev <= 4 * e_ref + EPS, (name, r, e_dev, e_ref)


@pytest.mark.parametrize('case', ['normal', 'edges', 'rows', 'ties'])
def test_loss_gradients_of_both_operands(golden, case):
    """1-D operands of different length, repeated q and lo == hi ('edges'), the 2-D form ('rows'), ties; the upstream scalar 3"""
    o, t, q = golden[case + '_out'], golden[case + '_gt'], golden[case + '_q']
    l32, go32, gt32 = R.loss_and_grads(o, t, q, torch.float32)
    l64, go64, gt64 = R.loss_and_grads(o, t, q, torch.float64)
    do, dt = on_device(o, 1).requires_grad_(True), on_device(t, 0).requires_grad_(True)
    loss = losses.QuantileLoss(do, dt, torch.from_numpy(q).cuda())
    (loss * 3.0).backward()
    assert do.grad.shape == o.shape and dt.grad.shape == t.shape
    check_grads(case + ' output', o, do.grad.cpu().numpy(), 3 * go32, 3 * go64, case == 'ties')
    check_grads(case + ' gt', t, dt.grad.cpu().numpy(), 3 * gt32, 3 * gt64, case == 'ties')
    assert abs(float(loss.detach()) - l64) <= 1e-5 * abs(l64)


@pytest.mark.parametrize('case', ['edges', 'rows', 'ties'])
def test_quantile_gradient(golden, case):
    """sum g quantile(data) with a seeded g [K, *leading]: contributions of both signs meet on elements"""
    d, q, g = golden[case + '_out'], golden[case + '_q'], golden[case + '_g']
    ref = {}
    for dtype in (torch.float32, torch.float64):
        a = torch.from_numpy(d).to(dtype).requires_grad_(True)
        (R.quantile(a, torch.from_numpy(q)) * torch.from_numpy(g).to(dtype)).sum().backward()
        ref[dtype] = a.grad.numpy()
    dd = on_device(d, 1).requires_grad_(True)
    qd = torch.from_numpy(q).cuda()
    out = losses.quantile(dd, qd)
    assert out.shape == g.shape
    (out * torch.from_numpy(g).cuda()).sum().backward()
    assert qd.grad is None
    check_grads(case, d, dd.grad.cpu().numpy(), ref[torch.float32], ref[torch.float64], case == 'ties')


# ------------------------------------------------------------------------------------------------------------ 5. determinism and hygiene
def test_two_calls_give_identical_bits_and_leave_the_inputs_alone(golden):
    o, t, q = golden['ties_out'], np.random.default_rng(16).normal(0, 3, 40000).astype(np.float32), golden['ties_q']
    do, dt, dq = on_device(o, 1), on_device(t, 0), torch.from_numpy(q).cuda()
    keep = (do.clone(), dt.clone(), dq.clone())
    runs = []
    for _ in range(2):
        a, b = do.detach().requires_grad_(True), dt.detach().requires_grad_(True)
        loss = losses.QuantileLoss(a, b, dq)
        (loss * 3.0).backward()
        runs.append((loss.detach().clone(), a.grad.clone(), b.grad.clone()) + tuple(x.clone() for x in losses.quantile_with_state(dt, dq)))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    assert runs[0][1].abs().max() > 0 and runs[0][2].abs().max() > 0
    for u, v in zip((do, dt, dq), keep):
        assert torch.equal(u, v)


def test_only_the_operand_that_requires_grad_gets_one(golden):
    o, t, q = golden['edges_out'], golden['edges_gt'], torch.from_numpy(golden['edges_q']).cuda()
    do, dt = on_device(o).requires_grad_(True), on_device(t)
    losses.QuantileLoss(do, dt, q).backward()
    assert do.grad is not None and dt.grad is None


def test_shapes_and_strides(golden):
    """Leading dimensions are rows; non-contiguous input is copied; a 0-dim q gives [*leading]."""
    o, q = golden['rows_out'][:, :4096], golden['rows_q']
    wide = torch.zeros(3, 8192, device='cuda')
    wide[:, ::2] = torch.from_numpy(o).cuda()
    do = wide[:, ::2].view(3, 1, 4096)
    assert not do.is_contiguous()
    keep = wide.clone()
    want = torch.quantile(torch.from_numpy(o), torch.from_numpy(q), dim=-1, interpolation='linear').numpy()
    do = do.detach().requires_grad_(True)
    got = losses.quantile(do, torch.from_numpy(q).cuda())
    assert got.shape == (q.size, 3, 1)
    got.sum().backward()
    assert do.grad.shape == (3, 1, 4096) and torch.equal(wide, keep)
    got = got.detach().cpu().numpy().reshape(q.size, 3)
    for r in range(3):
        a, b, _, _, w = R.order_stats(o[r], q)
        check_values(got[:, r], want[:, r], a, b, w, ('strided', r))
    one = losses.quantile(do.detach(), torch.tensor(0.5, device='cuda'))
    assert one.shape == (3, 1)
    med = torch.quantile(torch.from_numpy(o), 0.5, dim=-1).numpy()
    assert np.all(np.abs(one.cpu().numpy().reshape(-1) - med) <= 4 * 2.0 ** -24 * np.abs(med) + 1e-7)


def test_refusals():
    d = torch.zeros(4097, device='cuda')
    q = torch.linspace(0, 1, 8, device='cuda')
    with pytest.raises(_lib.PnnpError, match='1025 probabilities'):
        losses.quantile(d, torch.linspace(0, 1, 1025, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='0 probabilities'):
        losses.QuantileLoss(d, d, torch.zeros(0, device='cuda'))
    with pytest.raises(_lib.PnnpError, match='float32'):
        losses.QuantileLoss(d.double(), d, q)
    with pytest.raises(_lib.PnnpError, match='float32'):
        losses.QuantileLoss(d, d, q.double())
    with pytest.raises(_lib.PnnpError, match='0 samples'):
        losses.QuantileLoss(d[:0], d, q)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.QuantileLoss(d, d.cpu(), q)
    with pytest.raises(_lib.PnnpError, match='CPU tensor'):
        losses.QuantileLoss(d, d, q.cpu())
    with pytest.raises(_lib.PnnpError, match='rows'):
        losses.QuantileLoss(d[:4096].view(2, 2048), d[:4095].view(3, 1365), q)
    if torch.cuda.device_count() > 1:
        with pytest.raises(_lib.PnnpError, match='different devices'):
            losses.QuantileLoss(d, d.to('cuda:1'), q)


# ------------------------------------------------------------------------------------------------------------ 6. fitting
def test_adam_on_the_quantile_loss_fits_a_scale_and_a_shift():
    """The scheme of test_gpu_ddl.test_adam_on_the_cdf_loss_fits_a_scale_and_a_shift with QuantileLoss: scale * z + shift with fixed z, from
    (1, 0), 200 Adam steps against a N(0.3, 1.5^2) sample.  The loss must fall below a tenth of its start, both parameters must end closer
    to (1.5, 0.3), and the same run through the restatement on the device must reach the same loss within the gradient tolerance
    4 E_ref + 2^-23 accumulated over the steps -- steps x tolerance, relative to the starting loss."""
    steps, n, k = 200, 65536, 256
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(n, generator=gen)
    target = 0.3 + 1.5 * torch.randn(n, generator=gen)
    q = torch.linspace(0.002, 0.998, k)
    _, g32, _ = R.loss_and_grads(z, target, q, torch.float32)
    _, g64, _ = R.loss_and_grads(z, target, q, torch.float64)
    e_ref = np.abs(g32 - g64).max() / np.abs(g64).max()
    z, target, q = z.cuda(), target.cuda(), q.cuda()

    def fit(loss_fn):
        p = torch.tensor([1.0, 0.0], device='cuda', requires_grad=True)
        opt = torch.optim.Adam([p], lr=0.01)
        trace = []
        for _ in range(steps):
            opt.zero_grad()
            loss = loss_fn(p[0] * z + p[1], target, q)
            loss.backward()
            opt.step()
            trace.append(loss.detach())
        with torch.no_grad():
            trace.append(loss_fn(p[0] * z + p[1], target, q))
        return torch.stack(trace).cpu().numpy(), p.detach().cpu().numpy()

    ours, p = fit(losses.QuantileLoss)
    theirs, pr = fit(R.quantile_loss)
    tol = steps * (4 * e_ref + EPS) * ours[0]
    print('start', ours[0], 'end', ours[-1], 'parameters', p, '| restatement end', theirs[-1], pr, '| E_ref', e_ref, 'tolerance', tol,
          'difference', abs(ours[-1] - theirs[-1]))
    assert ours[-1] < ours[0] / 10
    assert abs(p[0] - 1.5) < 0.5 and abs(p[1] - 0.3) < 0.3
    assert abs(ours[-1] - theirs[-1]) <= tol


# ------------------------------------------------------------------------------------------------------------ 7. NoiseFlowFitStep
def fit_step_net():
    from pnnp_amd.archs import NoiseFlow
    np.random.seed(3); torch.manual_seed(3)
    return NoiseFlow({'x_shape': (4, 64, 64), 'arch': 'sdn|unc|unc|unc|unc|giso|unc|unc|unc|unc'}).cuda()


def test_noiseflow_fit_step_qloss():
    """qloss compares the pair that score draws at the same counters: it equals QuantileLoss on the tensors score returns."""
    from pnnp_amd.trainer import NoiseFlowFitStep
    net = fit_step_net()
    fs = NoiseFlowFitStep(net, camera_type='SonyA7S2', noise_code='pgrq', clip=2)
    hr = (torch.rand(2, 4, 64, 64, generator=torch.Generator().manual_seed(16)) * 0.3).cuda()
    with pytest.raises(_lib.PnnpError, match='CUDA'):
        fs.qloss(hr.cpu())
    q = losses.get_x(size=1000, mode='uniform').cuda()
    for per_crop in (False, True):
        for training in (True, False):
            net.train(training)
            np.random.seed(4); torch.manual_seed(4)
            offset = net.offset
            got = fs.qloss(hr, iso=1600, per_crop=per_crop)
            assert net.training == training and fs.step_count == 0 and net.offset == offset + 1
            np.random.seed(4); torch.manual_seed(4)
            net.offset = offset
            _, (hr_used, real, sampled) = fs.score(hr, iso=1600, return_tensors=True)
            noise = real - hr_used
            shape = (2, -1) if per_crop else (-1,)
            want = losses.QuantileLoss(sampled.reshape(shape), noise.reshape(shape), q)
            assert got.shape == () and got.is_cuda and torch.isfinite(got)
            assert torch.equal(got, want), (per_crop, float(got), float(want))
    net.train()
    np.random.seed(4); torch.manual_seed(4)
    net.offset = offset
    short = fs.qloss(hr, iso=1600, q=q[::10].contiguous())
    assert torch.isfinite(short) and not torch.equal(short, got)


@pytest.mark.parametrize('per_crop', [False, True])
def test_qloss_step_is_the_hand_written_composition(per_crop):
    from pnnp_amd.trainer import NoiseFlowFitStep
    hr = (torch.rand(2, 4, 64, 64, generator=torch.Generator().manual_seed(16)) * 0.3).cuda()
    kw = dict(lr=2e-3, camera_type='SonyA7S2', noise_code='pgrq', clip=2)
    net = fit_step_net().eval()
    fs = NoiseFlowFitStep(net, **kw)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    with pytest.raises(_lib.PnnpError, match='CUDA'):
        fs.qloss_step(hr.cpu())
    np.random.seed(4); torch.manual_seed(4)
    loss = fs.qloss_step(hr, iso=1600, per_crop=per_crop)
    assert loss.shape == () and loss.is_cuda and not loss.requires_grad and bool(torch.isfinite(loss))
    assert fs.step_count == 1 and net.training and net.offset == 1
    assert any(not torch.equal(p, before[k]) for k, p in net.named_parameters() if p.requires_grad)
    for k, p in net.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p, before[k]), k
    # the same step by hand on an identically seeded net
    net2 = fit_step_net().train()
    fs2 = NoiseFlowFitStep(net2, **kw)
    opt = torch.optim.Adam([p for p in net2.parameters() if p.requires_grad], lr=2e-3)
    np.random.seed(4); torch.manual_seed(4)
    real, ratio = fs2.make_pair(hr, 1600)
    hrc = hr.clamp(0, 1)
    sampled = net2.sample(clean=hrc / ratio, iso=1600.0, differentiable=True) * ratio
    noise = real - hrc
    shape = (2, -1) if per_crop else (-1,)
    loss2 = losses.QuantileLoss(sampled.reshape(shape), noise.reshape(shape), losses.get_x(size=1000, mode='uniform').cuda())
    loss2.backward(); opt.step()
    assert torch.equal(loss, loss2.detach())
    for (k, p), (_k2, p2) in zip(net.named_parameters(), net2.named_parameters()):
        assert torch.equal(p, p2), k
    sa, sb = net.state_dict(), net2.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # lr as for ddl_step
    fs.qloss_step(hr, iso=1600, per_crop=per_crop, lr=1e-3)
    assert fs.step_count == 2 and all(g['lr'] == 1e-3 for g in fs.optimizer.param_groups)
