"""The fp16x2 range census on the device (csrc/range_census.hip, ops.RangeCensus, HipTrainStep(range_every=...) / check_range()):
exact histograms against torch on the same tensors and slots, the job set against what the h2 kernels receive, bit-neutrality,
determinism, trips on outliers (warn / raise / fallback), no trip on SID-like data, no added synchronisation, and the
data-parallel fallback on two ranks."""
import inspect
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from pnnp_amd import ops
from pnnp_amd._lib import PnnpRangeError, PnnpRangeWarning

pytestmark = pytest.mark.gpu


def _unet(seed=5, nf=32):
    from pnnp_amd.archs import UNetSeeInDark, initialize_weights
    torch.manual_seed(seed)
    net = UNetSeeInDark(dict(nframes=1, res=False, nf=nf, in_nc=4, out_nc=4))
    initialize_weights(net)
    return net.cuda()


def _resunet(seed=5, nf=32):
    from pnnp_amd.archs import ResUnet, initialize_weights
    torch.manual_seed(seed)
    net = ResUnet(dict(nframes=1, res=False, nf=nf, in_nc=4, out_nc=4))
    initialize_weights(net)
    return net.cuda()


def _ts(net, **kw):
    from pnnp_amd.trainer import HipTrainStep
    return HipTrainStep(net, lr=1e-4, camera_type='SonyA7S2', noise_code='pr', ori=False, clip=2, seed=1997, **kw)


def _sid_like(B, S, gen):
    hr = torch.rand(B, 4, S, S, device='cuda', generator=gen) ** 2.2 * 0.1
    sat = torch.rand(B, 4, S, S, device='cuda', generator=gen) < 1e-3
    return torch.where(sat, torch.ones_like(hr), hr)


def _ref_counts(t, slot_bits):
    """The census of one job in torch: (48 bins, zero, nonfinite, over)."""
    ax = t.detach().reshape(-1).view(torch.int32).long() & 0x7fffffff
    A = int(slot_bits) & 0x7fffffff
    nonfin = int((ax >= 0x7f800000).sum())
    if A >= 0x7f800000:
        return [0] * 48, 0, nonfin, 0
    v = ax[(ax > 0) & (ax < 0x7f800000)]

    def flog2(b):
        E = b >> 23
        return torch.where(E > 0, E - 127, torch.floor(torch.log2(b.clamp(min=1).double())).long() - 149)
    ea = int(flog2(torch.tensor([A]))[0]) if A else 0
    k = (ea - flog2(v)).clamp(0, 47)
    return torch.bincount(k, minlength=48).cpu().tolist(), int((ax == 0).sum()), nonfin, int((v > A).sum())


def _slot_bits(s):
    return int(s.reshape(-1)[0].item()) & 0xffffffff


def _check_exact(net, hr):
    e = net.engine
    ts = _ts(net, range_every=1)
    for _ in range(2):
        ts.step(hr)
    flat = e.params.flat
    ts.census.reset()
    flat0 = e.params.flat.clone()                    # the weights this step's forward packs (Adam moves them after the census)
    ts.step(hr)
    rows = {(r['kind'], r['name']): r for r in ts.census.read()}
    pairs = e.census_pairs()
    kinds = {k for _, k, _, _ in pairs}
    assert kinds == {'act', 'grad', 'weight'}, kinds
    assert len(rows) == len(pairs)
    for name, kind, t, s in pairs:
        if kind == 'weight':
            off = (t.data_ptr() - flat.data_ptr()) // 4
            t = flat0[off:off + t.numel()]
        hist, zero, nonfin, over = _ref_counts(t, _slot_bits(s))
        r = rows[(kind, name)]
        assert r['hist'] == hist, (kind, name)
        assert (r['zero'], r['nonfinite'], r['over']) == (zero, nonfin, over), (kind, name)
        assert over == 0 and nonfin == 0 and r['censuses'] == 1
    # the median bin against h2_range_report's log2(amax / median) (a sampled median: within one bin)
    rep = {(r['kind'], r['name']): r for r in e.h2_range_report(sample=1 << 30)}
    both = [k for k in rep if k in rows and np.isfinite(rep[k]['log2_ratio'])]
    assert len(both) >= 10
    for k in both:
        assert abs(rows[k]['log2_ratio'] - rep[k]['log2_ratio']) <= 1.0 + 1e-6, (k, rows[k]['log2_ratio'], rep[k]['log2_ratio'])


def test_exact_histograms_unet_and_resunet():
    g = torch.Generator(device='cuda').manual_seed(3)
    _check_exact(_unet(), _sid_like(2, 64, g))
    _check_exact(_resunet(), _sid_like(2, 64, g))


_IN_PAIRS = (('x1', 'amax_x1'), ('x2', 'amax_x2'), ('x', 'amax_x'), ('g', 'amax_g'))


def _recording(monkeypatch):
    """Wrap every ops.*_h2* entry point and the PackJobs fp16x2 builders: the (tensor, slot) pairs they receive as split operands."""
    seen = set()

    def key(t, s):
        return (t.data_ptr(), t.numel(), s.data_ptr())
    for name, fn in list(vars(ops).items()):
        if callable(fn) and inspect.isfunction(fn) and '_h2' in name and 'supported' not in name and 'bytes' not in name:
            sig = inspect.signature(fn)

            def wrap(*a, __fn=fn, __sig=sig, **kw):
                b = __sig.bind(*a, **kw).arguments
                for tn, sn in _IN_PAIRS:
                    if b.get(tn) is not None and b.get(sn) is not None:
                        seen.add(key(b[tn], b[sn]))
                return __fn(*a, **kw)
            monkeypatch.setattr(ops, name, wrap)
    for name in ('add_h2', 'add_h2_convt', 'add_h2_1x1', 'add_h2_s2'):
        fn = getattr(ops.PackJobs, name)

        def wrapw(self, w, *a, __fn=fn, **kw):
            s = __fn(self, w, *a, **kw)
            seen.add(key(w, s))
            return s
        monkeypatch.setattr(ops.PackJobs, name, wrapw)
    return seen, key


@pytest.mark.parametrize('arch', ['unet', 'resunet'])
def test_job_set_equals_what_the_h2_kernels_split(monkeypatch, arch):
    seen, key = _recording(monkeypatch)
    net = _unet() if arch == 'unet' else _resunet()
    ts = _ts(net, range_every=0)
    g = torch.Generator(device='cuda').manual_seed(4)
    hr = _sid_like(2, 64, g)
    ts.step(hr)
    jobs = {key(t, s) for _, _, t, s in net.engine.census_pairs()}
    assert len(jobs) == len(net.engine.census_pairs()) >= 20
    assert jobs == seen, (len(jobs), len(seen), len(jobs - seen), len(seen - jobs))


def _run(net_fn, every, steps=10, seed=6):
    net = net_fn()
    ts = _ts(net, range_every=every)
    g = torch.Generator(device='cuda').manual_seed(seed)
    hr = _sid_like(2, 64, g)
    losses = []
    for s in range(steps):
        np.random.seed(100 + s)
        losses.append(ts.step(hr).clone())
    torch.cuda.synchronize()
    return torch.stack(losses).cpu(), net.engine.params.flat.cpu(), ts


def test_census_is_bit_neutral_and_deterministic():
    l1, p1, ts1 = _run(_unet, 1)
    l0, p0, _ = _run(_unet, 0)
    assert torch.equal(l1, l0) and torch.equal(p1, p0)
    _, _, ts2 = _run(_unet, 1)
    assert torch.equal(ts1.census.table.cpu(), ts2.census.table.cpu())
    assert int(ts1.census.table[1]) == 10                # one census per step


def _outlier_input(B, S, gen):
    noisy = torch.rand(B, 4, S, S, device='cuda', generator=gen) * 0.1
    noisy[0, 1, 5, 7] = float(noisy.abs().max()) * 1e8
    return noisy


def test_trips_on_an_input_outlier_warn_raise_fallback():
    g = torch.Generator(device='cuda').manual_seed(7)
    hr = torch.rand(2, 4, 64, 64, device='cuda', generator=g) * 0.1
    noisy = _outlier_input(2, 64, g)
    for action in ('warn', 'raise', 'fallback'):
        net = _unet()
        ts = _ts(net, range_every=1, on_range_trip=action)
        ts.step(hr, noisy=noisy)
        if action == 'raise':
            with pytest.raises(PnnpRangeError, match='act x8'):
                ts.check_range()
            continue
        with pytest.warns(PnnpRangeWarning, match='act x8') as rec:
            rows = ts.check_range()
        assert any(r['name'] == 'x8' and r['worst_share'] > 0.99 and r['worst_step'] == 1 for r in rows)
        assert all(r['over'] == 0 for r in rows)
        if action == 'fallback':
            assert 'bf16x3' in str(rec[0].message)
            assert net.engine.policy.h2 is False
            for _ in range(3):
                lo = ts.step(hr)
                assert torch.isfinite(lo).all()
            assert ts.check_range() == []                # nothing is split any more
        else:
            assert net.engine.policy.h2 is True


def test_trips_on_a_weight_outlier():
    g = torch.Generator(device='cuda').manual_seed(8)
    hr = torch.rand(2, 4, 64, 64, device='cuda', generator=g) * 0.1
    net = _unet()
    w = dict(net.named_parameters())['conv3_1.weight']
    with torch.no_grad():
        w[0, 0, 1, 1] = float(w.abs().max()) * 1e8
    net.engine.mark_dirty()
    ts = _ts(net, range_every=1, on_range_trip='fallback')
    ts.step(hr)
    with pytest.warns(PnnpRangeWarning, match=r'weight conv3_1\.weight'):
        ts.check_range()
    assert net.engine.policy.h2 is False
    for _ in range(2):
        assert torch.isfinite(ts.step(hr)).all()


def test_no_trip_on_sid_like_crops_and_config5_over_is_zero(golden_dir):
    gen = torch.Generator(device='cuda').manual_seed(21)
    pool = [_sid_like(2, 128, gen) for _ in range(4)]
    net = _unet()
    ts = _ts(net, range_every=5)
    for s in range(20):
        np.random.seed(1997 + s)
        ts.step(pool[s % 4])
    with warnings.catch_warnings():
        warnings.simplefilter('error', PnnpRangeWarning)
        rows = ts.check_range()
    assert rows and all(r['censuses'] == 4 and r['over'] == 0 and r['nonfinite'] == 0 for r in rows)
    # config 5: ResUnet + the NoiseFlow proxy (IMX686 ratios), small crops
    from tests.test_gpu_noiseflow import _net as _proxy
    proxy = _proxy(np.load(os.path.join(golden_dir, 'noiseflow.npz')))
    from pnnp_amd.trainer import HipTrainStep
    ts5 = HipTrainStep(_resunet(), lr=2e-3, clip=2, proxy_net=proxy, proxy_ratio_choices=(1, 2, 4, 8, 16), proxy_iso=1600, range_every=1)
    hr = torch.rand(2, 4, 64, 64, device='cuda', generator=gen) * 0.01
    for _ in range(3):
        ts5.step(hr)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', PnnpRangeWarning)      # (only `over` is asserted here: the proxy's noise is not SID-like)
        rows5 = ts5.check_range()
    assert rows5 and all(r['over'] == 0 and r['nonfinite'] == 0 for r in rows5)


def _sync_warnings(ts, hr, n=2):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            for _ in range(n):
                ts.step(hr)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return [f'{os.path.basename(w.filename)}:{w.lineno}' for w in rec if 'called a synchronizing' in str(w.message)]     # (not the mode's own notice)


def test_census_steps_add_no_synchronisation():
    g = torch.Generator(device='cuda').manual_seed(9)
    hr = _sid_like(2, 64, g)
    on, off = _ts(_unet(), range_every=1), _ts(_unet(), range_every=0)
    for ts in (on, off):                                  # warm-up: buffers, packs, the census job table
        ts.step(hr)
    torch.cuda.synchronize()
    got_on, got_off = _sync_warnings(on, hr), _sync_warnings(off, hr)
    assert len(got_on) <= len(got_off), (got_on, got_off)


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        g = torch.Generator(device='cuda').manual_seed(11 + rank)
        hr = torch.rand(2, 4, 64, 64, device='cuda', generator=g) * 0.1
        noisy = _outlier_input(2, 64, g) if rank == 1 else torch.rand(2, 4, 64, 64, device='cuda', generator=g) * 0.1
        ts = _ts(_unet(), range_every=1, on_range_trip='fallback', rank=rank, world=world)
        ts.step(hr, noisy=noisy)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            rows = ts.check_range()
        h2 = ts.engine.policy.h2
        losses = [float(ts.step(hr)[0]) for _ in range(2)]
        out.put((rank, h2, [str(w.message) for w in rec if issubclass(w.category, PnnpRangeWarning)],
                 [(r['name'], r['hist'], r['worst_share']) for r in rows], losses, ts.replica_checksum()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_fallback_on_both_ranks():
    ctx = mp.get_context('spawn')
    q = ctx.SimpleQueue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in procs:
        r, *rest = q.get()
        got[r] = rest
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    (h0, w0, rows0, l0, cs0), (h1, w1, rows1, l1, cs1) = got[0], got[1]
    assert h0 is False and h1 is False                    # both ranks switched, though only rank 1 saw the outlier
    assert w0 and w1 and w0 == w1 and 'x8' in w0[0]
    assert rows0 == rows1
    assert np.isfinite(l0).all() and np.isfinite(l1).all()
    assert cs0 == 0.0 and cs1 == 0.0
