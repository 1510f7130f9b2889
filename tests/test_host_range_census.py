"""The fp16x2 range census on the host (no GPU): the bin-to-bits mapping against the split itself (numpy's float16 rounds to nearest
even like the gfx950 conversion), the report and trip logic on synthetic tables, the cross-rank reduction over gloo (world size 2),
and the C entry's argument checks."""
import ctypes
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pnnp_amd import ops
from pnnp_amd._lib import PnnpError, PnnpRangeError, PnnpRangeWarning
from pnnp_amd.trainer import handle_range_trips, range_trips

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR, ROW = ops.CENSUS_HDR, ops.CENSUS_ROW


def _scale_exp(amax_bits):                       # csrc/h2.h pnnp_h2_scale_exp
    E = (amax_bits >> 23) & 0xff
    return 0 if E in (0, 255) else min(141 - E, 127)


def _split_rel_err(x, A):
    """max |s x - hi - lo| / |s x| of the fp16x2 split of float32 values x scaled by their tensor's amax A"""
    s = np.float32(2.0 ** _scale_exp(int(np.float32(A).view(np.uint32))))
    sx = (x.astype(np.float32) * s).astype(np.float32)
    hi = sx.astype(np.float16)
    lo = (sx - hi.astype(np.float32)).astype(np.float16)
    return float(np.max(np.abs(sx.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)) / np.abs(sx.astype(np.float64))))


@pytest.mark.parametrize('A', [1.7, 3.0e-3, 6.1e4])
def test_bin_bits_mapping_matches_the_split(A):
    rng = np.random.default_rng(0)
    ea = int(np.floor(np.log2(np.float32(A))))
    for k in range(0, 47):
        bits = ops.census_bin_bits(k)
        x = (np.float32(2.0) ** (ea - k)) * (1 + rng.random(4000, dtype=np.float32))          # floor(log2 x) = floor(log2 A) - k
        x = x[np.floor(np.log2(x.astype(np.float64))) == ea - k].astype(np.float32)
        err = _split_rel_err(x, A)
        if bits > 0:
            assert err <= 2.0 ** -bits, (k, bits, err)                                      # keeps at least `bits` bits ...
            assert err > 2.0 ** -(bits + 2), (k, bits, err)                                 # ... and not two more
        else:
            assert err >= 0.25, (k, err)                                                    # nothing left worth a bit
    assert [ops.census_bin_bits(k) for k in (0, 17, 18, 24, 28, 29, 39, 47)] == [22, 22, 21, 15, 11, 10, 0, 0]
    assert ops.census_first_low_bin(16) == 24 and ops.census_first_low_bin(23) == 0 and ops.census_first_low_bin(0) == 48


def _fp16_subnormal_from(k, A=1.0):
    s = 2.0 ** _scale_exp(int(np.float32(A).view(np.uint32)))
    return abs(np.float16(np.float32(A * 2.0 ** -k * 1.5 * s))) < np.float16(2.0 ** -14)


def test_hi_is_subnormal_from_bin_29():
    assert not _fp16_subnormal_from(28) and _fp16_subnormal_from(29)


def _table(rows, kmin=24):
    """A census table (int64 numpy) from per-row dicts of bins / counters / worst / step / amax / censuses."""
    t = np.zeros(HDR + len(rows) * ROW, np.int64)
    t[0] = kmin
    for r, d in enumerate(rows):
        w = t[HDR + r * ROW:HDR + (r + 1) * ROW]
        for k, v in d.get('bins', {}).items():
            w[k] = v
        w[48], w[49], w[50] = d.get('zero', 0), d.get('nonfinite', 0), d.get('over', 0)
        w[51] = int(np.float32(d.get('worst', 0.0)).view(np.uint32))
        w[52] = d.get('step', 0)
        w[53] = int(np.float32(d.get('last', 0.0)).view(np.uint32))
        w[54] = int(np.float32(d.get('amax', 1.0)).view(np.uint32))
        w[55] = d.get('censuses', 1)
    return t


def test_report_share_median_and_small_fraction():
    t = _table([dict(bins={2: 600, 3: 300, 20: 95, 30: 5}, zero=7, worst=0.005, step=512, amax=2.5),
                dict(bins={0: 10}, censuses=0),                                             # took part in no census: not reported
                dict(bins={1: 1000}, amax=0.25, censuses=3)])
    rows = ops.census_rows(t, [('c1', 'act'), ('x', 'act'), ('conv1_1.weight', 'weight')])
    assert [r['name'] for r in rows] == ['c1', 'conv1_1.weight']
    r = rows[0]
    assert r['count'] == 1000 and r['zero'] == 7 and r['amax'] == 2.5 and r['kind'] == 'act'
    assert r['log2_ratio'] == 2.0                       # median bin: 600 of 1000 in bin 2
    assert r['frac_small'] == pytest.approx(0.1)        # bins >= 18
    assert r['low_share'] == pytest.approx(0.005)       # bins >= 24 (16 bits)
    assert r['worst_share'] == pytest.approx(0.005, rel=1e-6) and r['worst_step'] == 512
    assert rows[1]['censuses'] == 3 and rows[1]['low_share'] == 0.0
    # another bits threshold moves the low bins: 10 bits -> bins >= 30
    assert ops.census_rows(t, [('c1', 'act')], min_bits=10)[0]['low_share'] == pytest.approx(0.005)
    assert ops.census_rows(t, [('c1', 'act')], min_bits=20)[0]['low_share'] == pytest.approx(0.1)     # bins >= 20


def test_slot_exponent_255_counts_nonfinite_only_and_trips():
    t = _table([dict(nonfinite=12, amax=float('inf'))])
    r = ops.census_rows(t, [('g_c9', 'grad')])[0]
    assert r['count'] == 0 and r['nonfinite'] == 12 and r['amax'] == float('inf') and np.isnan(r['log2_ratio']) and r['low_share'] == 0.0
    assert range_trips([r], 1e-3) == [r]


class _Engine:
    def __init__(self):
        self.calls = []

    def set_policy(self, **kw):
        self.calls.append(kw)


def _rows():
    t = _table([dict(bins={3: 99}, worst=0.0), dict(bins={3: 90, 30: 10}, worst=0.1, step=256), dict(bins={1: 5}, over=1)])
    return ops.census_rows(t, [('c1', 'act'), ('u6', 'act'), ('g_c2', 'grad')])


def test_trip_rule():
    rows = _rows()
    assert [r['name'] for r in range_trips(rows, 1e-3)] == ['u6', 'g_c2']
    assert [r['name'] for r in range_trips(rows, 0.5)] == ['g_c2']                          # `over` trips whatever the share
    ok = ops.census_rows(_table([dict(bins={3: 99}, worst=5e-4)]), [('c1', 'act')])
    e = _Engine()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert handle_range_trips(ok, 1e-3, 'fallback', e) == [] and e.calls == []


def test_trip_actions():
    rows = _rows()
    e = _Engine()
    with pytest.warns(PnnpRangeWarning, match=r'act u6: low-bit share 0\.1 .* at step 256'):
        handle_range_trips(rows, 1e-3, 'warn', e)
    assert e.calls == []
    with pytest.raises(PnnpRangeError, match='grad g_c2') as ei:
        handle_range_trips(rows, 1e-3, 'raise', e)
    assert isinstance(ei.value, PnnpError) and e.calls == []
    with pytest.warns(PnnpRangeWarning, match='bf16x3'):
        handle_range_trips(rows, 1e-3, 'fallback', e)
    assert e.calls == [dict(h2=False)]
    with pytest.raises(ValueError):
        handle_range_trips(rows, 1e-3, 'ignore', e)


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        meta = [('c1', 'act'), ('g_c1', 'grad')]
        if rank == 0:
            t = _table([dict(bins={2: 100}, worst=0.0, step=0, amax=1.0), dict(bins={4: 50}, zero=3, worst=0.0, amax=2.0)])
        else:                                            # the outlier on rank 1 only
            t = _table([dict(bins={2: 60, 40: 40}, worst=0.4, step=10, amax=4.0, last=0.4), dict(bins={4: 50}, nonfinite=2, worst=0.0, amax=1.0)])
        t[1], t[2] = 2, 10
        red = ops.reduce_census_table(torch.from_numpy(t), None).numpy()
        rows = ops.census_rows(red, meta)
        e = _Engine()
        with warnings.catch_warnings(record=True):
            warnings.simplefilter('always')
            trips = handle_range_trips(rows, 1e-3, 'fallback', e)
        out.put((rank, red.tolist(), rows, [r['name'] for r in trips], e.calls))
    finally:
        dist.destroy_process_group()


def test_cross_rank_reduction_gives_every_rank_the_same_report():
    ctx = mp.get_context('spawn')
    q = ctx.SimpleQueue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict((r, rest) for r, *rest in (q.get() for _ in ps))
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    (t0, rows0, trips0, calls0), (t1, rows1, trips1, calls1) = got[0], got[1]
    assert t0 == t1 and rows0 == rows1 and trips0 == trips1 and calls0 == calls1
    c1, g = rows0
    assert c1['hist'][2] == 160 and c1['hist'][40] == 40 and c1['count'] == 200 and c1['censuses'] == 2
    assert c1['worst_share'] == pytest.approx(0.4) and c1['worst_step'] == 10 and c1['amax'] == 4.0
    assert g['zero'] == 3 and g['nonfinite'] == 2 and g['amax'] == 2.0
    assert trips0 == ['c1', 'g_c1'] and calls0 == [dict(h2=False)]


def test_c_entry_checks_arguments_without_a_gpu():
    so = os.path.join(REPO, 'pnnp_amd', 'libpnnp_hip.so')
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    f = lib.pnnp_range_census_f32
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    jobs, table = 0x10000, 0x20000                       # never dereferenced: every call below fails its checks first
    assert lib.pnnp_census_job_bytes() == ctypes.sizeof(ops.CensusJob) == 32
    lib.pnnp_census_table_words.restype = ctypes.c_int64
    assert lib.pnnp_census_table_words(3) == HDR + 3 * ROW
    assert f(jobs, 1, None, 0, None) == -1                # null table
    assert f(None, 1, table, 0, None) == -1               # null job table
    assert f(jobs, 0, table, 0, None) == -1               # no jobs
    assert f(jobs, -3, table, 0, None) == -1
    assert f(jobs, ops.CENSUS_MAX_JOBS + 1, table, 0, None) == -1
    assert f(jobs + 8, 1, table, 0, None) == -1           # misaligned job table
    assert f(jobs, 1, table + 4, 0, None) == -1           # misaligned census table
