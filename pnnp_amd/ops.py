"""Thin ctypes wrappers of the layer-level C ABI (include/pnnp_hip.h).  Tensors are CUDA
fp32; activations NHWC.  No CPU path: every function raises on CPU tensors."""
import ctypes as C
import inspect

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, require_cuda, stream

_i64 = C.c_int64

# Optional per-launch timing with HIP events on the launching stream (bench.py turns it on):
# PROFILE = [] collects (kind, algorithmic_flops, algorithmic_bytes, start_event, end_event, sub); `sub` names the kernel instantiation
# a launch class resolves to where that matters for its roofline ('bn32' / 'bn64': pnnp_h2_tile_columns), else ''.
PROFILE = None
PROFILE_KINDS = None        # None: every launch class; a set: only those (bench.py times just the dominant kernel in its timed region)


class _Timed:
    def __init__(self, kind, flops=0.0, nbytes=0.0, sub=None):
        self.rec = None
        if PROFILE is not None and (PROFILE_KINDS is None or kind in PROFILE_KINDS):
            self.rec = (kind, float(flops), float(nbytes), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True),
                        sub() if callable(sub) else (sub or ''))

    def __enter__(self):
        if self.rec is not None:
            self.rec[3].record(torch.cuda.current_stream())

    def __exit__(self, *a):
        if self.rec is not None:
            self.rec[4].record(torch.cuda.current_stream())
            PROFILE.append(self.rec)


ABI_VERSION = 9                 # the PNNP_ABI_VERSION of include/pnnp_hip.h these wrappers (and the PackJob mirror below) were written against


def _prep():
    L = lib()
    if not getattr(L, '_pnnp_sigs', False):
        got = L.pnnp_abi_version() if hasattr(L, 'pnnp_abi_version') else None
        if got != ABI_VERSION or L.pnnp_pack_job_bytes() != C.sizeof(PackJob):
            raise _lib.PnnpError(f'{_lib.LIB_PATH}: ABI version {got} / PnnpPackJob of {L.pnnp_pack_job_bytes() if got else "?"} bytes, these bindings '
                                 f'were written for version {ABI_VERSION} / {C.sizeof(PackJob)} bytes: rebuild the library (tools/build.py)')
        L.pnnp_wgrad_workspace_floats.restype = C.c_int64
        L.pnnp_wino_weight_floats.restype = C.c_int64
        L.pnnp_wino_wgrad_workspace_floats.restype = C.c_int64
        L.pnnp_x3_weight_bytes.restype = C.c_int64
        L.pnnp_x3_wgrad_workspace_floats.restype = C.c_int64
        L.pnnp_x3g_wgrad_workspace_floats.restype = C.c_int64
        L.pnnp_x3mat_bytes.restype = C.c_int64
        L.pnnp_h2_weight_bytes.restype = C.c_int64
        L.pnnp_h1_weight_bytes.restype = C.c_int64
        L.pnnp_h1_pointwise_weight_bytes.restype = C.c_int64
        L.pnnp_h2_bits_words.restype = C.c_int64
        L.pnnp_h2mat_bytes.restype = C.c_int64
        L.pnnp_h2g_wgrad_workspace_floats.restype = C.c_int64
        L.pnnp_head_bwd_workspace_floats.restype = C.c_int64
        L.pnnp_first_wgrad_workspace_floats.restype = C.c_int64
        L.pnnp_census_table_words.restype = C.c_int64
        if L.pnnp_census_job_bytes() != C.sizeof(CensusJob):
            raise _lib.PnnpError(f'{_lib.LIB_PATH}: PnnpCensusJob of {L.pnnp_census_job_bytes()} bytes, these bindings were written for '
                                 f'{C.sizeof(CensusJob)}: rebuild the library (tools/build.py)')
        L._pnnp_sigs = True
    return L


def pack_conv_weight(w, fwd, dgrad, cin_pad=None, cout_pad=None):
    co, ci, kh, kw = w.shape
    check(_prep().pnnp_pack_conv_weight_f32(ptr(w), ptr(fwd), ptr(dgrad), co, ci, kh * kw,
                                            cin_pad or ci, cout_pad or co, stream()), 'pack_conv_weight')


class PackJob(C.Structure):                      # PnnpPackJob of include/pnnp_hip.h
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('kind', C.c_int), ('T', C.c_int), ('K', C.c_int), ('N', C.c_int),
                ('sk', C.c_int64), ('sn', C.c_int64), ('st', C.c_int64), ('off', C.c_int64),
                ('flip', C.c_int), ('Kvalid', C.c_int), ('Ndst', C.c_int), ('n_off', C.c_int), ('amax', C.c_void_p)]


class PackJobs:
    """A table of weight re-pack jobs (csrc/pack_jobs.hip): filled once per model / device with the add_* builders, run once
    per optimiser step in ceil(n / 32) launches instead of one or two launches per layer.  The tensors whose pointers are
    recorded must stay alive and in place (parameters as views of the flat buffer, the persistent packed buffers)."""

    def __init__(self, cap=256):
        self.cap = cap
        self.jobs = (PackJob * cap)()
        self.n = C.c_int(0)
        self.keep = []                           # the tensors behind the recorded pointers
        # fp16x2 packs (add_h2) scale every weight tensor by its own maximum: the amax jobs form a table of their own that run() launches
        # FIRST (a pack job reads the slot its amax job filled); `wslots` holds one 4-byte slot per weight tensor
        self.amax_jobs = None
        self.n_amax = C.c_int(0)
        self.wslots = None
        self._wslot_of = {}
        self.split_weights = []                  # (weight tensor, its slot) for every weight an fp16x2 pack splits: the range census's weight jobs

    def add_conv(self, w, fwd, dgrad, cin_pad=None, cout_pad=None):
        co, ci, kh, kw = w.shape
        check(_prep().pnnp_pack_jobs_add_conv(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(fwd), ptr(dgrad), co, ci, kh * kw,
                                              cin_pad or ci, cout_pad or co), 'pack_jobs_add_conv')
        self.keep += [w, fwd, dgrad]

    def add_convt(self, w, fwd, dgrad):
        ci, co = w.shape[0], w.shape[1]
        check(_prep().pnnp_pack_jobs_add_convt(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(fwd), ptr(dgrad), ci, co), 'pack_jobs_add_convt')
        self.keep += [w, fwd, dgrad]

    def add_wino(self, w, fwd, dgrad):
        co, ci = w.shape[0], w.shape[1]
        check(_prep().pnnp_pack_jobs_add_wino(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(fwd), ptr(dgrad), co, ci), 'pack_jobs_add_wino')
        self.keep += [w, fwd, dgrad]

    def add_x3(self, w, fwd, dgrad, cin_pad=None):
        """bf16x3 packs (csrc/conv_x3s.hip) of a 3x3 Conv2d weight; fwd / dgrad: uint8 buffers of x3_weight_bytes, or None."""
        co, ci = w.shape[0], w.shape[1]
        check(_prep().pnnp_pack_jobs_add_x3(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(fwd), ptr(dgrad), co, ci,
                                            cin_pad or (ci + 15) // 16 * 16), 'pack_jobs_add_x3')
        self.keep += [w, fwd, dgrad]

    def weight_slot(self, w):
        """The amax slot (a 1-element int32 view) of weight tensor ``w``; its amax job is added on first use."""
        key = (w.data_ptr(), w.numel())
        if key not in self._wslot_of:
            if self.wslots is None:
                self.wslots = torch.zeros(self.cap, dtype=torch.int32, device=w.device)
                self.amax_jobs = (PackJob * self.cap)()
            i = len(self._wslot_of)
            slot = self.wslots[i:i + 1]
            check(_prep().pnnp_pack_jobs_add_amax(self.amax_jobs, C.byref(self.n_amax), self.cap, ptr(w), C.c_int64(w.numel()), ptr(slot)), 'pack_jobs_add_amax')
            self._wslot_of[key] = slot
            self.split_weights.append((w, slot))
            self.keep += [w]
        return self._wslot_of[key]

    def add_h2(self, w, fwd, dgrad, cin_pad=None):
        """fp16x2 packs (csrc/conv_h2s.hip) of a 3x3 Conv2d weight; fwd / dgrad: uint8 buffers of h2_weight_bytes, or None.  Returns the
        weight tensor's amax slot (what the kernels take as ``amax_w``)."""
        co, ci = w.shape[0], w.shape[1]
        slot = self.weight_slot(w)
        check(_prep().pnnp_pack_jobs_add_h2(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(fwd), ptr(dgrad), co, ci,
                                            cin_pad or (ci + 15) // 16 * 16, ptr(slot)), 'pack_jobs_add_h2')
        self.keep += [w, fwd, dgrad]
        return slot

    def add_h1(self, w, dst, cin_pad=None):
        """The fp16x1 forward pack (csrc/conv_h1s.hip) of a 3x3 Conv2d weight; dst: a uint8 buffer of h1_weight_bytes.  Returns the weight tensor's
        amax slot (what the kernels take as ``amax_w``)."""
        co, ci = w.shape[0], w.shape[1]
        slot = self.weight_slot(w)
        check(_prep().pnnp_pack_jobs_add_h1(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(dst), co, ci, cin_pad or (ci + 15) // 16 * 16, ptr(slot)),
              'pack_jobs_add_h1')
        self.keep += [w, dst]
        return slot

    def _add_pointwise(self, fam, kind, w, fwd, dgrad=None):
        """The pack jobs of a pointwise layer's weight: ``fam`` 'x3' (csrc/gemm_x3.hip) | 'h2' (csrc/gemm_h2s.hip) | 'h1' (csrc/gemm_h1s.hip), ``kind`` 'convt'
        (ConvTranspose2d(2, 2), [Cin][Cout][2][2]) | '1x1' | 's2' (stride-2 3x3).  fwd / dgrad: zero-filled uint8 buffers of x3mat_bytes / h2mat_bytes /
        h1_pointwise_weight_bytes of the GEMM's (K, N), or None; h1 is forward only and has no dgrad.  The fp16 families scale by the weight tensor's amax
        slot, which is returned (x3: None)."""
        name = f'pack_jobs_add_{fam}_{kind}'
        bufs = [fwd] if fam == 'h1' else [fwd, dgrad]
        slot = None if fam == 'x3' else self.weight_slot(w)
        check(getattr(_prep(), 'pnnp_' + name)(self.jobs, C.byref(self.n), self.cap, ptr(w), *[ptr(b) for b in bufs], w.shape[0], w.shape[1],
                                               *([] if slot is None else [ptr(slot)])), name)
        self.keep += [w] + bufs
        return slot

    def add_h2_convt(self, w, fwd, dgrad): return self._add_pointwise('h2', 'convt', w, fwd, dgrad)
    def add_h2_1x1(self, w, fwd, dgrad): return self._add_pointwise('h2', '1x1', w, fwd, dgrad)
    def add_h2_s2(self, w, fwd, dgrad): return self._add_pointwise('h2', 's2', w, fwd, dgrad)
    def add_h1_convt(self, w, fwd): return self._add_pointwise('h1', 'convt', w, fwd)
    def add_h1_1x1(self, w, fwd): return self._add_pointwise('h1', '1x1', w, fwd)
    def add_h1_s2(self, w, fwd): return self._add_pointwise('h1', 's2', w, fwd)
    def add_x3_convt(self, w, fwd, dgrad): return self._add_pointwise('x3', 'convt', w, fwd, dgrad)
    def add_x3_1x1(self, w, fwd, dgrad): return self._add_pointwise('x3', '1x1', w, fwd, dgrad)
    def add_x3_s2(self, w, fwd, dgrad): return self._add_pointwise('x3', 's2', w, fwd, dgrad)

    def add_s2_dgrad(self, w, dst):
        co, ci = w.shape[0], w.shape[1]
        check(_prep().pnnp_pack_jobs_add_conv3x3s2_dgrad(self.jobs, C.byref(self.n), self.cap, ptr(w), ptr(dst), co, ci), 'pack_jobs_add_s2_dgrad')
        self.keep += [w, dst]

    def run(self):
        if self.n_amax.value:
            self.wslots.zero_()
            check(_prep().pnnp_pack_jobs_f32(self.amax_jobs, self.n_amax.value, stream()), 'pack_jobs (amax)')
        check(_prep().pnnp_pack_jobs_f32(self.jobs, self.n.value, stream()), 'pack_jobs')



# ---- range census of the fp16x2 family (csrc/range_census.hip, include/pnnp_hip.h PNNP_CENSUS_*)
class CensusJob(C.Structure):                    # PnnpCensusJob of include/pnnp_hip.h
    _fields_ = [('x', C.c_void_p), ('n', C.c_int64), ('slot', C.c_void_p), ('row', C.c_int), ('reserved', C.c_int)]


CENSUS_BINS, CENSUS_HDR, CENSUS_ROW, CENSUS_MAX_JOBS = 48, 64, 128, 512
_C_ZERO, _C_NONFIN, _C_OVER, _C_COUNTERS, _C_WORST, _C_WSTEP, _C_LAST, _C_AMAX, _C_NCENS = 48, 49, 50, 51, 51, 52, 53, 54, 55


def census_bin_bits(k):
    """Significand bits the fp16x2 split keeps of an element k binades below its tensor's amax (bin 47: k >= 47): csrc/range_census.hip."""
    return max(0, min(22, 39 - int(k)))


def census_first_low_bin(min_bits):
    """The first bin whose elements keep fewer than ``min_bits`` bits (24 for 16 bits); 48: none."""
    return next((k for k in range(CENSUS_BINS) if census_bin_bits(k) < min_bits), CENSUS_BINS)


def _f32(bits):
    return float(np.array([int(bits) & 0xffffffff], dtype=np.uint32).view(np.float32)[0])


def census_rows(table, meta, min_bits=16):
    """The report of a census table (1-D int64 array, host): one dict per row that took part in a census since the table was reset.
    ``log2_ratio`` is the median bin (h2_range_report's log2(amax / median |x|) to within one), ``frac_small`` the share of the finite non-zero
    elements 18 or more binades down (h2_range_report's "below 2^-18 amax"), ``low_share`` the share in bins that keep fewer than ``min_bits``
    bits over all censuses, ``worst_share`` / ``worst_step`` the largest per-census share and the step it was reached at."""
    t = np.asarray(table, dtype=np.int64)
    kmin = census_first_low_bin(min_bits)
    rows = []
    for r, (name, kind) in enumerate(meta):
        w = t[CENSUS_HDR + r * CENSUS_ROW:CENSUS_HDR + (r + 1) * CENSUS_ROW]
        if len(w) < CENSUS_ROW or w[_C_NCENS] == 0:
            continue
        hist = [int(v) for v in w[:CENSUS_BINS]]
        n = sum(hist)
        med = float('nan')
        if n:
            acc = 0
            for k, v in enumerate(hist):
                acc += v
                if 2 * acc >= n:
                    med = float(k)
                    break
        rows.append(dict(name=name, kind=kind, amax=_f32(w[_C_AMAX]), log2_ratio=med, frac_small=(sum(hist[18:]) / n if n else 0.0),
                         low_share=(sum(hist[kmin:]) / n if n else 0.0), worst_share=_f32(w[_C_WORST]), worst_step=int(w[_C_WSTEP]),
                         nonfinite=int(w[_C_NONFIN]), over=int(w[_C_OVER]), zero=int(w[_C_ZERO]), count=n, censuses=int(w[_C_NCENS]), hist=hist))
    return rows


def reduce_census_table(table, group=None):
    """The census table summed over the ranks of ``group`` (counters: integer SUM; worst share, latest share, amax: MAX; the step of the worst
    share: the largest step among the ranks that hold it), so every rank reads the same report.  Returns a new tensor."""
    import torch.distributed as dist
    rows = (table.numel() - CENSUS_HDR) // CENSUS_ROW
    body = table[CENSUS_HDR:CENSUS_HDR + rows * CENSUS_ROW].view(rows, CENSUS_ROW)
    sums = torch.cat([body[:, :_C_COUNTERS], body[:, _C_NCENS:_C_NCENS + 1]], 1).contiguous()
    maxs = torch.cat([body[:, [_C_WORST, _C_LAST, _C_AMAX]], table[1:3].view(1, 2).expand(rows, 2)], 1).contiguous()
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(maxs, op=dist.ReduceOp.MAX, group=group)
    step = torch.where(body[:, _C_WORST] == maxs[:, 0], body[:, _C_WSTEP], torch.full_like(body[:, _C_WSTEP], -1)).contiguous()
    dist.all_reduce(step, op=dist.ReduceOp.MAX, group=group)
    out = table.clone()
    ob = out[CENSUS_HDR:CENSUS_HDR + rows * CENSUS_ROW].view(rows, CENSUS_ROW)
    ob[:, :_C_COUNTERS] = sums[:, :_C_COUNTERS]
    ob[:, _C_NCENS] = sums[:, _C_COUNTERS]
    ob[:, _C_WORST], ob[:, _C_LAST], ob[:, _C_AMAX] = maxs[:, 0], maxs[:, 1], maxs[:, 2]
    ob[:, _C_WSTEP] = step
    if rows:
        out[1:3] = maxs[0, 3:5]
    return out


class RangeCensus:
    """The device table of range censuses (csrc/range_census.hip) and its job tables.  ``run(pairs, step)`` counts, on the current stream and
    without synchronising, every (name, kind, tensor, amax slot) pair in one launch (+ a one-workgroup summary); rows are assigned per
    (kind, name) on first sight.  The device job table of a pair set is built once (pinned host copy, asynchronous upload) and reused while
    the same buffers come back.  ``read()`` is the one host synchronisation: the report of census_rows; ``reset()`` zeroes the table."""

    def __init__(self, device, min_bits=16, rows=256):
        self.device = torch.device(device)
        self.min_bits = int(min_bits)
        self.kmin = census_first_low_bin(self.min_bits)
        self.cap = int(rows)
        self.table = torch.zeros(int(_prep().pnnp_census_table_words(self.cap)), dtype=torch.int64, device=self.device)
        self.meta = []                           # row -> (name, kind)
        self._row = {}
        self._sets = {}
        self.reset()

    def reset(self):
        self.table.zero_()
        self.table[0] = self.kmin

    def row(self, name, kind):
        key = (kind, name)
        if key not in self._row:
            if len(self.meta) >= self.cap:
                raise _lib.PnnpError(f'range census table full ({self.cap} rows)')
            self._row[key] = len(self.meta)
            self.meta.append((name, kind))
        return self._row[key]

    def _jobs(self, pairs):
        key = tuple((kind, name, t.data_ptr(), t.numel(), s.data_ptr()) for name, kind, t, s in pairs)
        got = self._sets.get(key)
        if got is None:
            if len(pairs) > CENSUS_MAX_JOBS:
                raise _lib.PnnpError(f'range census: {len(pairs)} jobs, at most {CENSUS_MAX_JOBS} per launch')
            arr = (CensusJob * len(pairs))()
            rows = set()
            for i, (name, kind, t, s) in enumerate(pairs):
                require_cuda(t, s)
                if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 or t.numel() >= 1 << 32 or s.dtype != torch.int32:
                    raise _lib.PnnpError(f'range census: {kind} {name} must be a contiguous, 16-byte aligned float32 tensor of < 2^32 elements with an int32 slot')
                r = self.row(name, kind)
                if r in rows:
                    raise _lib.PnnpError(f'range census: {kind} {name} appears twice in one census')
                rows.add(r)
                arr[i] = CensusJob(t.data_ptr(), t.numel(), s.data_ptr(), r, 0)
            nb = C.sizeof(arr)
            host = torch.empty(nb, dtype=torch.uint8).pin_memory()
            C.memmove(host.data_ptr(), arr, nb)
            dev = torch.empty(nb, dtype=torch.uint8, device=self.device)
            dev.copy_(host, non_blocking=True)
            if len(self._sets) >= 16:
                self._sets.clear()
            got = self._sets[key] = (dev, len(pairs), host, [p[2:] for p in pairs])
        return got

    def run(self, pairs, step=0):
        if not pairs:
            return
        dev, n, _, _ = self._jobs(pairs)
        check(_prep().pnnp_range_census_f32(ptr(dev), n, ptr(self.table), C.c_longlong(int(step)), stream()), 'range_census')

    def read(self, reduce=False, group=None):
        """The report (census_rows) -- with ``reduce``, of the table summed over the ranks of ``group`` (reduce_census_table).  Synchronises."""
        t = reduce_census_table(self.table, group) if reduce else self.table
        return census_rows(t.cpu().numpy(), self.meta, self.min_bits)


def pack_convt_weight(w, fwd, dgrad):
    ci, co = w.shape[:2]
    check(_prep().pnnp_pack_convt_weight_f32(ptr(w), ptr(fwd), ptr(dgrad), ci, co, stream()), 'pack_convt_weight')


def conv_fwd(x1, x2, w_packed, bias, y, cout, taps, act, residual=None):
    require_cuda(x1, x2, w_packed, y)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv%d_fwd' % taps, 2.0 * B * H * W * cout * (C1 + C2) * taps, 4.0 * B * H * W * (C1 + C2 + cout)):
        check(_prep().pnnp_conv_fwd_f32(ptr(x1), C1, ptr(x2), C2, ptr(w_packed), ptr(bias), ptr(residual), ptr(y),
                                        B, H, W, cout, taps, act, stream()), 'conv_fwd')
    return y


def conv_bwd_data(g, w_dgrad, dx1, mask1=None, mode1=0, accum1=0, dx2=None, mask2=None, mode2=0, accum2=0, taps=9):
    require_cuda(g, w_dgrad, dx1)
    B, H, W, Cout = g.shape
    C1 = dx1.shape[3]
    C2 = dx2.shape[3] if dx2 is not None else 0
    with _Timed('conv%d_dgrad' % taps, 2.0 * B * H * W * Cout * (C1 + C2) * taps, 4.0 * B * H * W * (C1 + C2 + Cout)):
        check(_prep().pnnp_conv_bwd_data_f32(ptr(g), Cout, ptr(w_dgrad), ptr(dx1), C1, ptr(mask1), mode1, accum1,
                                             ptr(dx2), C2, ptr(mask2), mode2, accum2, B, H, W, taps, stream()), 'conv_bwd_data')


def x3_supported(K, N):
    return bool(_prep().pnnp_x3_supported(int(K), int(N)))


def x3_image_fits(H, W, cstride):
    """one [H][W][cstride] image within the 32-bit offsets of the bf16x3 forward / backward-data / pointwise kernels?"""
    return bool(_prep().pnnp_x3_image_fits(int(H), int(W), int(cstride)))


def x3_wgrad_fits(B, H, W, cstride):
    return bool(_prep().pnnp_x3_wgrad_fits(int(B), int(H), int(W), int(cstride)))


def x3_weight_bytes(K, N):
    return int(_prep().pnnp_x3_weight_bytes(int(K), int(N)))


def conv_x3_fwd(x1, x2, w_x3, bias, y, cout, act, residual=None):
    """3x3 / stride 1 / pad 1 forward on the bf16 matrix cores, fp32 operands split in three (same contract as conv_fwd, taps=9)."""
    require_cuda(x1, x2, w_x3, y)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_x3', 2.0 * B * H * W * cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + cout)):
        check(_prep().pnnp_conv3x3_x3_fwd_f32(ptr(x1), C1, ptr(x2), C2, ptr(w_x3), ptr(bias), ptr(residual), ptr(y), B, H, W, cout, act,
                                              stream()), 'conv_x3_fwd')
    return y


def conv_x3_fwd_pool(x1, x2, w_x3, bias, y, pooled, codes, cout, act):
    """conv_x3_fwd + MaxPool2d(2) of the activated output in the same kernel (pooled [B,H/2,W/2,cout], codes as maxpool_fwd)."""
    require_cuda(x1, x2, w_x3, y, pooled, codes)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_x3', 2.0 * B * H * W * cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + cout)):
        check(_prep().pnnp_conv3x3_x3_fwd_pool_f32(ptr(x1), C1, ptr(x2), C2, ptr(w_x3), ptr(bias), ptr(y), ptr(pooled), ptr(codes),
                                                   B, H, W, cout, act, stream()), 'conv_x3_fwd_pool')
    return y


def conv_x3_bwd_data(g, w_x3_dgrad, dx1, mask1=None, mode1=0, accum1=0, dx2=None, mask2=None, mode2=0, accum2=0):
    require_cuda(g, w_x3_dgrad, dx1)
    B, H, W, Cout = g.shape
    C1 = dx1.shape[3]
    C2 = dx2.shape[3] if dx2 is not None else 0
    with _Timed('conv9_dgrad_x3', 2.0 * B * H * W * Cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + Cout)):
        check(_prep().pnnp_conv3x3_x3_bwd_data_f32(ptr(g), Cout, ptr(w_x3_dgrad), ptr(dx1), C1, ptr(mask1), mode1, accum1,
                                                   ptr(dx2), C2, ptr(mask2), mode2, accum2, B, H, W, stream()), 'conv_x3_bwd_data')


def conv_x3_bwd_data_res(g, w_x3_dgrad, dx, addsrc, mask=None, mode=0):
    require_cuda(g, w_x3_dgrad, dx, addsrc)
    B, H, W, Cout = g.shape
    C1 = dx.shape[3]
    with _Timed('conv9_dgrad_x3', 2.0 * B * H * W * Cout * C1 * 9, 4.0 * B * H * W * (2 * C1 + Cout)):
        check(_prep().pnnp_conv3x3_x3_bwd_data_res_f32(ptr(g), Cout, ptr(w_x3_dgrad), ptr(dx), C1, ptr(addsrc), ptr(mask), mode,
                                                       B, H, W, stream()), 'conv_x3_bwd_data_res')


# ---- the fp16x2 ("h2") family: csrc/conv_h2s.hip, csrc/h2.h.  amax_* are 1-element int32 CUDA tensors (the slots), bits_* int32 tensors of
# h2_bits_words elements.
def h2_supported(K, N):
    return bool(_prep().pnnp_h2_supported(int(K), int(N)))


def h2_weight_bytes(K, N):
    return int(_prep().pnnp_h2_weight_bytes(int(K), int(N)))


def h2_bits_words(B, H, W, C_):
    return int(_prep().pnnp_h2_bits_words(int(B), int(H), int(W), int(C_)))


def h2_splitk(B, H, W, chunks, N):
    """K slices for a small grid (pnnp_h2_splitk): 1 = launch as usual."""
    return int(_prep().pnnp_h2_splitk(int(B), int(H), int(W), int(chunks), int(N)))


def amax(x, slot):
    """slot = max(slot, max |x|) as a kernel of its own (tensors whose producer has no fused amax)."""
    require_cuda(x, slot)
    with _Timed('amax', 0.0, 4.0 * x.numel()):
        check(_prep().pnnp_amax_f32(ptr(x), C.c_int64(x.numel()), ptr(slot), stream()), 'amax')
    return slot


def h2_tile_columns(B, H, W, N, pool=False):
    """GEMM columns per workgroup tile the fp16x2 3x3 kernel picks for this map (32: the HBM-bound instantiations; pnnp_h2_tile_columns)."""
    return int(_prep().pnnp_h2_tile_columns(int(B), int(H), int(W), int(N), int(bool(pool))))


# ---- the fp16x1 ("h1") family: csrc/conv_h1s.hip -- the h2 forward entries with one fp16 piece per operand, eval forward only (no sign bits)
def h1_supported(K, N):
    return bool(_prep().pnnp_h1_supported(int(K), int(N)))


def h1_weight_bytes(K, N):
    return int(_prep().pnnp_h1_weight_bytes(int(K), int(N)))


# ---- the 3x3 forward layers of both fp16 families, one wrapper per layer shape: ``fam`` = 'h2' | 'h1' picks the C entry and the _Timed kind
# ('conv9_fwd_h2' / 'conv9_fwd_h1'); the h2 entries alone take ``bits_y``.  The per-family names below them (conv_h2_fwd, conv_h1_fwd, ...) are what
# callers use, the engine included: what wraps or inspects ``ops.conv_h2_fwd`` (tests/test_gpu_range_census.py) sees every call and named parameters.
def _for_family(fn, fam):
    """``fn`` with its first parameter bound to ``fam``, as a plain function that reports the rest of ``fn``'s signature"""
    def bound(*a, **kw):
        return fn(fam, *a, **kw)
    sig = inspect.signature(fn)
    bound.__signature__ = sig.replace(parameters=list(sig.parameters.values())[1:])
    bound.__name__, bound.__doc__ = fn.__name__.replace('f16', fam), fn.__doc__
    return bound


def _f16_entry(fam, name, bits_y=None):
    """(the C entry ``name`` with FAM replaced, the arguments that stand for ``bits_y`` in its list); refuses sign bits for h1 before any call"""
    if fam not in ('h2', 'h1') or (fam == 'h1' and bits_y is not None):
        raise _lib.PnnpError(f'{name}: family {fam!r}' + (' writes no sign bits (bits_y)' if fam == 'h1' else ' is not an fp16 family'))
    return getattr(_prep(), name.replace('FAM', fam)), ((ptr(bits_y),) if fam == 'h2' else ())


def conv_f16_fwd(fam, x1, x2, w, amax_w, bias, y, cout, act, amax_x1, amax_x2=None, amax_y=None, *, bits_y=None, residual=None):
    """3x3 / stride 1 / pad 1 forward on the fp16 matrix cores (contract of conv_fwd, taps=9): fp32 operands split on the fly in two scaled fp16 pieces
    (h2) or rounded to one (h1)."""
    fn, bits = _f16_entry(fam, 'pnnp_conv3x3_FAM_fwd_f32', bits_y)
    require_cuda(x1, x2, w, y, amax_w, amax_x1)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_' + fam, 2.0 * B * H * W * cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + cout), sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, cout)):
        check(fn(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(residual), ptr(y), ptr(amax_y), *bits,
                 B, H, W, cout, act, stream()), f'conv_{fam}_fwd')
    return y


def conv_f16_fwd_splitk(fam, x1, x2, w, amax_w, bias, y, cout, act, amax_x1, ksplit, ws, amax_x2=None, amax_y=None, *, bits_y=None):
    """conv_f16_fwd with K cut into ``ksplit`` slices (small grids, h2_splitk): partial sums into ``ws`` (>= ksplit * y.numel() floats), one fixed-order reduce."""
    fn, bits = _f16_entry(fam, 'pnnp_conv3x3_FAM_fwd_splitk_f32', bits_y)
    require_cuda(x1, x2, w, y, amax_w, amax_x1, ws)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_' + fam, 2.0 * B * H * W * cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + cout), sub='splitk'):
        check(fn(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), *bits,
                 B, H, W, cout, act, int(ksplit), ptr(ws), _i64(ws.numel()), stream()), f'conv_{fam}_fwd_splitk')
    return y


def conv_f16_fwd_head(fam, x1, x2, w, amax_w, bias, y, cout, act, amax_x1, head_w, head_b, out, amax_x2=None, amax_y=None, *, bits_y=None, residual=None):
    """The last 3x3 layer + activation + the 1x1 head in one kernel (archs/Unet.py:93-94): ``out`` NCHW [B,4,H,W] (+ ``residual``, NCHW);
    ``y`` None: the 32-channel map is not stored (eval forward)."""
    fn, bits = _f16_entry(fam, 'pnnp_conv3x3_FAM_fwd_head_f32', bits_y)
    require_cuda(x1, x2, w, y, amax_w, amax_x1, head_w, out, residual)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_' + fam, 2.0 * B * H * W * cout * (C1 + C2) * 9 + 2.0 * B * H * W * cout * 4, 4.0 * B * H * W * (C1 + C2 + (cout if y is not None else 0) + 4), sub='bn32'):
        check(fn(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), *bits,
                 ptr(head_w), ptr(head_b), ptr(residual), ptr(out), B, H, W, cout, act, stream()), f'conv_{fam}_fwd_head')
    return out


def conv_f16_fwd_pool(fam, x1, x2, w, amax_w, bias, y, pooled, codes, cout, act, amax_x1, amax_x2=None, amax_y=None, *, bits_y=None):
    """conv_f16_fwd + MaxPool2d(2) of its output from the same kernel: ``pooled`` and the argmax / sign ``codes`` of maxpool_fwd"""
    fn, bits = _f16_entry(fam, 'pnnp_conv3x3_FAM_fwd_pool_f32', bits_y)
    require_cuda(x1, x2, w, y, pooled, codes, amax_w, amax_x1)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_' + fam, 2.0 * B * H * W * cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + 1.25 * cout) + B * H * W * cout / 4,
                sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, cout, True)):      # (+ the pooled map and its one-byte codes)
        check(fn(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(pooled), ptr(codes), ptr(amax_y), *bits,
                 B, H, W, cout, act, stream()), f'conv_{fam}_fwd_pool')
    return y


conv_h2_fwd, conv_h1_fwd = _for_family(conv_f16_fwd, 'h2'), _for_family(conv_f16_fwd, 'h1')
conv_h2_fwd_splitk, conv_h1_fwd_splitk = _for_family(conv_f16_fwd_splitk, 'h2'), _for_family(conv_f16_fwd_splitk, 'h1')
conv_h2_fwd_head, conv_h1_fwd_head = _for_family(conv_f16_fwd_head, 'h2'), _for_family(conv_f16_fwd_head, 'h1')
conv_h2_fwd_pool, conv_h1_fwd_pool = _for_family(conv_f16_fwd_pool, 'h2'), _for_family(conv_f16_fwd_pool, 'h1')


# ---- the fp16x1 layers with fp16 ACTIVATIONS ("h1a": csrc/conv_h1s.hip H1a, the pnnp_conv3x3_h1_*_et entries).  The element type of a side is the dtype of its
# tensors: torch.float16 NHWC sources are taken as they are (unscaled; no amax slot), a torch.float16 ``y`` / ``pooled`` receives float16(the float32 value the
# conv_h1_* wrapper stores).  float32 on both sides is that wrapper.  Anything else -- another dtype, x2 unlike x1, pooled unlike y -- is refused HERE.
def image_fits(H, W, cstride, elem_bytes=4):
    """one [H][W][cstride] image of ``elem_bytes``-byte elements within the 32-bit byte offsets of the matrix-core kernels?  (4: x3_image_fits)"""
    return bool(_prep().pnnp_image_fits_es(int(H), int(W), int(cstride), int(elem_bytes)))


def _h1a_types(what, x1, x2, y, *same_as_y):
    """(src_f16, dst_f16) of a launch from its tensors' dtypes; ``y`` None: a float32 destination"""
    def is16(t, role):
        if t.dtype not in (torch.float16, torch.float32):
            raise _lib.PnnpError(f'{what}: {role} is {t.dtype}: torch.float16 or torch.float32')
        return t.dtype == torch.float16
    s16 = is16(x1, 'x1')
    if x2 is not None and is16(x2, 'x2') != s16:
        raise _lib.PnnpError(f'{what}: x1 is {x1.dtype} and x2 {x2.dtype}: the K segments of a launch share one element type')
    d16 = is16(y, 'y') if y is not None else False
    for t in same_as_y:
        if t is not None and t.dtype != y.dtype:
            raise _lib.PnnpError(f'{what}: {t.dtype} beside a {y.dtype} destination')
    return int(s16), int(d16)


def _h1a_bytes(B, H, W, C1, C2, cout, s16, d16):
    return B * H * W * ((C1 + C2) * (2.0 if s16 else 4.0) + cout * (2.0 if d16 else 4.0))


def conv_h1a_fwd(x1, x2, w, amax_w, bias, y, cout, act, amax_x1=None, amax_x2=None, amax_y=None, residual=None):
    """conv_h1_fwd with the element types of ``x1`` / ``x2`` and ``y``.  ``residual`` (pnnp_conv3x3_h1_fwd_res_et): a tensor of y's shape and dtype, added to
    the float32 sum before the one rounding; offered with torch.float16 on all three sides (float32 on all three: conv_h1_fwd), no activation."""
    s16, d16 = _h1a_types('conv_h1a_fwd', x1, x2, y, residual)
    require_cuda(x1, x2, w, y, amax_w, residual)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    if residual is not None:
        if tuple(residual.shape) != tuple(y.shape):
            raise _lib.PnnpError(f'conv_h1a_fwd: the residual is {tuple(residual.shape)}, y {tuple(y.shape)}')
        with _Timed('conv9_fwd_h1a', 2.0 * B * H * W * cout * (C1 + C2) * 9, _h1a_bytes(B, H, W, C1, C2, 2 * cout, s16, d16), sub=lambda: 'res_bn%d' % h2_tile_columns(B, H, W, cout)):
            check(_prep().pnnp_conv3x3_h1_fwd_res_et(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(residual), ptr(y),
                                                     ptr(amax_y), s16, d16, d16, B, H, W, cout, act, stream()), 'conv_h1a_fwd')
        return y
    with _Timed('conv9_fwd_h1a', 2.0 * B * H * W * cout * (C1 + C2) * 9, _h1a_bytes(B, H, W, C1, C2, cout, s16, d16), sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, cout)):
        check(_prep().pnnp_conv3x3_h1_fwd_et(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), s16, d16,
                                             B, H, W, cout, act, stream()), 'conv_h1a_fwd')
    return y


def conv_h1a_fwd_splitk(x1, x2, w, amax_w, bias, y, cout, act, ksplit, ws, amax_x1=None, amax_x2=None, amax_y=None):
    """conv_h1_fwd_splitk with element types: the slabs ``ws`` stay float32, the reduce rounds once into an fp16 ``y``"""
    s16, d16 = _h1a_types('conv_h1a_fwd_splitk', x1, x2, y)
    if ws.dtype != torch.float32:
        raise _lib.PnnpError(f'conv_h1a_fwd_splitk: the slabs are float32, ws is {ws.dtype}')
    require_cuda(x1, x2, w, y, amax_w, ws)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_h1a', 2.0 * B * H * W * cout * (C1 + C2) * 9, _h1a_bytes(B, H, W, C1, C2, cout, s16, d16), sub='splitk'):
        check(_prep().pnnp_conv3x3_h1_fwd_splitk_et(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), s16, d16,
                                                    B, H, W, cout, act, int(ksplit), ptr(ws), _i64(ws.numel()), stream()), 'conv_h1a_fwd_splitk')
    return y


def conv_h1a_fwd_head(x1, x2, w, amax_w, bias, cout, act, head_w, head_b, out, amax_x1=None, amax_x2=None, residual=None):
    """conv_h1_fwd_head of an fp16 source: ``out`` float32 NCHW [B,4,H,W] (+ ``residual``), nothing else stored"""
    s16, _ = _h1a_types('conv_h1a_fwd_head', x1, x2, None)
    for t in (head_w, head_b, out, residual):
        if t is not None and t.dtype != torch.float32:
            raise _lib.PnnpError(f'conv_h1a_fwd_head: the head is float32, got {t.dtype}')
    require_cuda(x1, x2, w, amax_w, head_w, out, residual)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_h1a', 2.0 * B * H * W * cout * (C1 + C2) * 9 + 2.0 * B * H * W * cout * 4, _h1a_bytes(B, H, W, C1, C2, 0, s16, 0) + 16.0 * B * H * W, sub='bn32'):
        check(_prep().pnnp_conv3x3_h1_fwd_head_et(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(head_w), ptr(head_b),
                                                  ptr(residual), ptr(out), s16, B, H, W, cout, act, stream()), 'conv_h1a_fwd_head')
    return out


def conv_h1a_fwd_pool(x1, x2, w, amax_w, bias, y, pooled, codes, cout, act, amax_x1=None, amax_x2=None, amax_y=None):
    """conv_h1_fwd_pool with element types: ``pooled`` has the dtype of ``y``; the ``codes`` are those of the float32 map"""
    s16, d16 = _h1a_types('conv_h1a_fwd_pool', x1, x2, y, pooled)
    if codes.dtype != torch.uint8:
        raise _lib.PnnpError(f'conv_h1a_fwd_pool: the codes are bytes, got {codes.dtype}')
    require_cuda(x1, x2, w, y, pooled, codes, amax_w)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_h1a', 2.0 * B * H * W * cout * (C1 + C2) * 9, _h1a_bytes(B, H, W, C1, C2, 1.25 * cout, s16, d16) + B * H * W * cout / 4,
                sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, cout, True)):
        check(_prep().pnnp_conv3x3_h1_fwd_pool_et(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(pooled), ptr(codes),
                                                  ptr(amax_y), s16, d16, B, H, W, cout, act, stream()), 'conv_h1a_fwd_pool')
    return y


def conv_h2_bwd_data(g, amax_g, w_h2_dgrad, amax_w, dx1, mask1=None, bits1=None, mode1=0, accum1=0, amax_dx1=None,
                     dx2=None, mask2=None, bits2=None, mode2=0, accum2=0, amax_dx2=None):
    require_cuda(g, w_h2_dgrad, dx1, amax_g, amax_w)
    B, H, W, Cout = g.shape
    C1 = dx1.shape[3]
    C2 = dx2.shape[3] if dx2 is not None else 0
    with _Timed('conv9_dgrad_h2', 2.0 * B * H * W * Cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + Cout), sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, C1 + C2)):
        check(_prep().pnnp_conv3x3_h2_bwd_data_f32(ptr(g), Cout, ptr(amax_g), ptr(w_h2_dgrad), ptr(amax_w),
                                                   ptr(dx1), C1, ptr(mask1), ptr(bits1), mode1, accum1, ptr(amax_dx1),
                                                   ptr(dx2), C2, ptr(mask2), ptr(bits2), mode2, accum2, ptr(amax_dx2), B, H, W, stream()), 'conv_h2_bwd_data')


def conv_h2_bwd_data_unpool(g, amax_g, w_h2_dgrad, amax_w, col0, cols, dx, bits=None, mode=0, accum=0, amax_dx=None, gp=None, codes=None):
    """Columns [col0, col0 + C) of a backward-data pack with ``cols`` columns into ``dx`` [B,H,W,C] (the act' mask as sign bits, or none).  With ``gp`` / ``codes``
    (the pooled map's gradient and the forward pass's codes) the kernel adds the un-pooled gradient before it stores: bit-identical to the plain launch
    followed by ``maxpool_bwd(.., gp, dx, mode, 1, codes=codes, amax_gx=amax_dx)``, without that pass over the full-resolution map."""
    require_cuda(g, w_h2_dgrad, dx, amax_g, amax_w, gp, codes)
    B, H, W, Cout = g.shape
    C1 = dx.shape[3]
    nbytes = 4.0 * B * H * W * (C1 + Cout) + (1.25 * B * H * W * C1 if gp is not None else 0.0)      # (+ the pooled gradient and its one-byte codes)
    with _Timed('conv9_dgrad_h2', 2.0 * B * H * W * Cout * C1 * 9, nbytes, sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, C1)):
        check(_prep().pnnp_conv3x3_h2_bwd_data_unpool_f32(ptr(g), Cout, ptr(amax_g), ptr(w_h2_dgrad), ptr(amax_w), int(col0), int(cols), ptr(dx), C1, ptr(bits), mode,
                                                          int(accum), ptr(amax_dx), ptr(gp), gp.shape[3] if gp is not None else 0, ptr(codes), B, H, W, stream()),
              'conv_h2_bwd_data_unpool')


def conv_h2_bwd_data_res(g, amax_g, w_h2_dgrad, amax_w, dx, addsrc, mask=None, mode=0, amax_dx=None):
    require_cuda(g, w_h2_dgrad, dx, addsrc, amax_g, amax_w)
    B, H, W, Cout = g.shape
    C1 = dx.shape[3]
    with _Timed('conv9_dgrad_h2', 2.0 * B * H * W * Cout * C1 * 9, 4.0 * B * H * W * (2 * C1 + Cout), sub=lambda: 'bn%d' % h2_tile_columns(B, H, W, C1)):
        check(_prep().pnnp_conv3x3_h2_bwd_data_res_f32(ptr(g), Cout, ptr(amax_g), ptr(w_h2_dgrad), ptr(amax_w), ptr(dx), C1, ptr(addsrc), ptr(mask), mode,
                                                       ptr(amax_dx), B, H, W, stream()), 'conv_h2_bwd_data_res')


def gemm_x3_supported(K, N):
    return bool(_prep().pnnp_gemm_x3_supported(int(K), int(N)))


def x3mat_bytes(K, N):
    return int(_prep().pnnp_x3mat_bytes(int(K), int(N)))


def convt_x3_fwd(x, w_x3, bias, y, cout, amax_y=None):
    require_cuda(x, w_x3, y)
    B, H, W, Cin = x.shape
    with _Timed('convt_fwd_x3', 8.0 * B * H * W * Cin * cout, 4.0 * B * H * W * (Cin + 4 * cout)):
        check(_prep().pnnp_convt2x2_x3_fwd_amax_f32(ptr(x), Cin, ptr(w_x3), ptr(bias), ptr(y), ptr(amax_y), B, H, W, cout, stream()), 'convt_x3_fwd')
    return y


def convt_x3_bwd_data(g, w_x3_dgrad, dx, mask=None, mode=0, amax_dx=None):
    require_cuda(g, w_x3_dgrad, dx)
    B, H, W, Cin = dx.shape
    with _Timed('convt_dgrad_x3', 8.0 * B * H * W * Cin * g.shape[3], 4.0 * B * H * W * (Cin + 4 * g.shape[3])):
        check(_prep().pnnp_convt2x2_x3_bwd_data_amax_f32(ptr(g), g.shape[3], ptr(w_x3_dgrad), ptr(dx), Cin, ptr(mask), mode, ptr(amax_dx), B, H, W, stream()),
              'convt_x3_bwd_data')


def gemm_h2_supported(K, N):
    return bool(_prep().pnnp_gemm_h2_supported(int(K), int(N)))


def h2mat_bytes(K, N):
    return int(_prep().pnnp_h2mat_bytes(int(K), int(N)))


# ---- the pointwise forward layers of both fp16 families (csrc/gemm_h2s.hip, csrc/gemm_h1s.hip), as the 3x3 ones above: contracts of the _x3_ wrappers + the amax slots
def convt_f16_fwd(fam, x, amax_x, w, amax_w, bias, y, cout, amax_y=None):
    """ConvTranspose2d(2, 2) forward on the fp16 matrix cores: contract of convt_x3_fwd + the amax slots."""
    fn, _ = _f16_entry(fam, 'pnnp_convt2x2_h2_fwd_f32' if fam == 'h2' else 'pnnp_convt_h1_fwd_f32')
    require_cuda(x, w, y, amax_x, amax_w)
    B, H, W, Cin = x.shape
    with _Timed('convt_fwd_' + fam, 8.0 * B * H * W * Cin * cout, 4.0 * B * H * W * (Cin + 4 * cout)):
        check(fn(ptr(x), Cin, ptr(amax_x), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), B, H, W, cout, stream()), f'convt_{fam}_fwd')
    return y


def conv1x1_f16_fwd(fam, x1, amax_x1, x2, amax_x2, w, amax_w, bias, y, cout, act, *, residual=None, amax_y=None):
    fn, _ = _f16_entry(fam, 'pnnp_conv1x1_FAM_fwd_f32')
    require_cuda(x1, x2, w, y, amax_x1, amax_w)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv1_fwd_' + fam, 2.0 * B * H * W * cout * (C1 + C2), 4.0 * B * H * W * (C1 + C2 + cout)):
        check(fn(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(residual), ptr(y), ptr(amax_y),
                 B, H, W, cout, act, stream()), f'conv1x1_{fam}_fwd')
    return y


def conv_s2_f16_fwd(fam, x, amax_x, w, amax_w, bias, y, cout, act, amax_y=None):
    fn, _ = _f16_entry(fam, 'pnnp_conv3x3s2_h2_fwd_f32' if fam == 'h2' else 'pnnp_conv_s2_h1_fwd_f32')
    require_cuda(x, w, y, amax_x, amax_w)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_fwd_' + fam, 2.0 * B * (H // 2) * (W // 2) * cout * Cin * 9):
        check(fn(ptr(x), Cin, ptr(amax_x), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), B, H, W, cout, act, stream()), f'conv_s2_{fam}_fwd')
    return y


convt_h2_fwd, convt_h1_fwd = _for_family(convt_f16_fwd, 'h2'), _for_family(convt_f16_fwd, 'h1')

conv1x1_h2_fwd, conv1x1_h1_fwd = _for_family(conv1x1_f16_fwd, 'h2'), _for_family(conv1x1_f16_fwd, 'h1')
conv_s2_h2_fwd, conv_s2_h1_fwd = _for_family(conv_s2_f16_fwd, 'h2'), _for_family(conv_s2_f16_fwd, 'h1')


def convt_h1a_fwd(x, w, amax_w, bias, y, cout, amax_x=None, amax_y=None):
    """convt_h1_fwd with the element types of ``x`` and ``y`` (csrc/gemm_h1s.hip H1ga): both torch.float16 -- x taken as it is, y = float16(the float32 value
    convt_h1_fwd stores) -- or both float32 (that wrapper); a mixed pair is refused by the entry"""
    s16, d16 = _h1a_types('convt_h1a_fwd', x, None, y)
    require_cuda(x, w, y, amax_w)
    B, H, W, Cin = x.shape
    with _Timed('convt_fwd_h1a', 8.0 * B * H * W * Cin * cout, B * H * W * ((2.0 if s16 else 4.0) * Cin + (2.0 if d16 else 4.0) * 4 * cout)):
        check(_prep().pnnp_convt_h1_fwd_et(ptr(x), Cin, ptr(amax_x), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), s16, d16, B, H, W, cout, stream()), 'convt_h1a_fwd')
    return y


def conv_s2_h1a_fwd(x, w, amax_w, bias, y, cout, act, amax_x=None, amax_y=None):
    """conv_s2_h1_fwd with the element types of ``x`` and ``y`` (csrc/gemm_h1s.hip H1ga): both torch.float16 or both float32; a mixed pair is refused by the entry"""
    s16, d16 = _h1a_types('conv_s2_h1a_fwd', x, None, y)
    require_cuda(x, w, y, amax_w)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_fwd_h1a', 2.0 * B * (H // 2) * (W // 2) * cout * Cin * 9, B * H * W * ((2.0 if s16 else 4.0) * Cin + (2.0 if d16 else 4.0) * cout / 4)):
        check(_prep().pnnp_conv_s2_h1_fwd_et(ptr(x), Cin, ptr(amax_x), ptr(w), ptr(amax_w), ptr(bias), ptr(y), ptr(amax_y), s16, d16, B, H, W, cout, act, stream()),
              'conv_s2_h1a_fwd')
    return y


def conv1x1_h1a_fwd(x1, x2, w, amax_w, bias, y, cout, act, amax_x1=None, amax_x2=None, amax_y=None):
    """conv1x1_h1_fwd on cat([x1, x2]) with the element types of the sources and ``y``: all torch.float16 or all float32; no residual"""
    s16, d16 = _h1a_types('conv1x1_h1a_fwd', x1, x2, y)
    require_cuda(x1, x2, w, y, amax_w)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv1_fwd_h1a', 2.0 * B * H * W * cout * (C1 + C2), _h1a_bytes(B, H, W, C1, C2, cout, s16, d16)):
        check(_prep().pnnp_conv1x1_h1_fwd_et(ptr(x1), C1, ptr(amax_x1), ptr(x2), C2, ptr(amax_x2), ptr(w), ptr(amax_w), ptr(bias), ptr(None), ptr(y), ptr(amax_y), s16, d16,
                                             B, H, W, cout, act, stream()), 'conv1x1_h1a_fwd')
    return y


def convt_h2_bwd_data(g, amax_g, w_h2_dgrad, amax_w, dx, mask=None, mode=0, amax_dx=None, bits=None):
    """``bits``: the act' mask as the sign bits a 3x3 fp16x2 forward kernel stored for the layer's input map (then ``mask`` is not read)."""
    require_cuda(g, w_h2_dgrad, dx, amax_g, amax_w, bits)
    B, H, W, Cin = dx.shape
    with _Timed('convt_dgrad_h2', 8.0 * B * H * W * Cin * g.shape[3], 4.0 * B * H * W * (Cin + 4 * g.shape[3])):
        if bits is not None and mode:
            check(_prep().pnnp_convt2x2_h2_bwd_data_bits_f32(ptr(g), g.shape[3], ptr(amax_g), ptr(w_h2_dgrad), ptr(amax_w), ptr(dx), Cin, ptr(bits), mode, ptr(amax_dx),
                                                             B, H, W, stream()), 'convt_h2_bwd_data (bit masks)')
            return
        check(_prep().pnnp_convt2x2_h2_bwd_data_f32(ptr(g), g.shape[3], ptr(amax_g), ptr(w_h2_dgrad), ptr(amax_w), ptr(dx), Cin, ptr(mask), mode, ptr(amax_dx),
                                                    B, H, W, stream()), 'convt_h2_bwd_data')


def conv1x1_h2_bwd_data(g, amax_g, w_h2_dgrad, amax_w, dx1, mask1=None, mode1=0, accum1=0, amax_dx1=None, dx2=None, mask2=None, mode2=0, accum2=0):
    require_cuda(g, w_h2_dgrad, dx1, dx2, amax_g, amax_w)
    B, H, W, Cout = g.shape
    C1 = dx1.shape[3]; C2 = dx2.shape[3] if dx2 is not None else 0
    with _Timed('conv1_dgrad_h2', 2.0 * B * H * W * Cout * (C1 + C2), 4.0 * B * H * W * (C1 + C2 + Cout)):
        check(_prep().pnnp_conv1x1_h2_bwd_data_f32(ptr(g), Cout, ptr(amax_g), ptr(w_h2_dgrad), ptr(amax_w), ptr(dx1), C1, ptr(mask1), mode1, int(accum1), ptr(amax_dx1),
                                                   ptr(dx2), C2, ptr(mask2), mode2, int(accum2), B, H, W, stream()), 'conv1x1_h2_bwd_data')


def conv_s2_h2_bwd_data(g, amax_g, w_h2_s2dgrad, amax_w, dx, mask=None, mode=0, accum=0, amax_dx=None):
    require_cuda(g, w_h2_s2dgrad, dx, amax_g, amax_w)
    B, H, W, Cin = dx.shape
    with _Timed('conv9s2_dgrad_h2', 2.0 * B * (H // 2) * (W // 2) * g.shape[3] * Cin * 9):
        check(_prep().pnnp_conv3x3s2_h2_bwd_data_f32(ptr(g), g.shape[3], ptr(amax_g), ptr(w_h2_s2dgrad), ptr(amax_w), ptr(dx), Cin, ptr(mask), mode, int(accum), ptr(amax_dx),
                                                     B, H, W, stream()), 'conv_s2_h2_bwd_data')


# ---- the fp16x1 ("h1") pointwise packs: csrc/gemm_h1s.hip, one fp16 piece per operand, eval forward only
def h1_pointwise_supported(K, N):
    return bool(_prep().pnnp_h1_pointwise_supported(int(K), int(N)))


def h1_pointwise_weight_bytes(K, N):
    """Bytes of a kind-8 pack; K, N of the forward GEMM (ConvTranspose2d: Cin, 4 Cout; 1x1: Cin, Cout; stride 2: 9 Cin, Cout)."""
    return int(_prep().pnnp_h1_pointwise_weight_bytes(int(K), int(N)))


def conv1x1_x3_fwd(x1, x2, w_x3, bias, y, cout, act, residual=None):
    require_cuda(x1, x2, w_x3, y)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv1_fwd_x3', 2.0 * B * H * W * cout * (C1 + C2), 4.0 * B * H * W * (C1 + C2 + cout)):
        check(_prep().pnnp_conv1x1_x3_fwd_f32(ptr(x1), C1, ptr(x2), C2, ptr(w_x3), ptr(bias), ptr(residual), ptr(y), B, H, W, cout, act, stream()),
              'conv1x1_x3_fwd')
    return y


def conv1x1_x3_bwd_data(g, w_x3_dgrad, dx1, mask1=None, mode1=0, accum1=0, dx2=None, mask2=None, mode2=0, accum2=0):
    require_cuda(g, w_x3_dgrad, dx1)
    B, H, W, Cout = g.shape
    C1 = dx1.shape[3]
    C2 = dx2.shape[3] if dx2 is not None else 0
    with _Timed('conv1_dgrad_x3', 2.0 * B * H * W * Cout * (C1 + C2), 4.0 * B * H * W * (C1 + C2 + Cout)):
        check(_prep().pnnp_conv1x1_x3_bwd_data_f32(ptr(g), Cout, ptr(w_x3_dgrad), ptr(dx1), C1, ptr(mask1), mode1, accum1,
                                                   ptr(dx2), C2, ptr(mask2), mode2, accum2, B, H, W, stream()), 'conv1x1_x3_bwd_data')


def conv_s2_x3_fwd(x, w_x3, bias, y, cout, act=0, amax_y=None):
    require_cuda(x, w_x3, y)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_fwd_x3', 2.0 * B * (H // 2) * (W // 2) * cout * Cin * 9):
        check(_prep().pnnp_conv3x3s2_x3_fwd_amax_f32(ptr(x), Cin, ptr(w_x3), ptr(bias), ptr(y), ptr(amax_y), B, H, W, cout, act, stream()), 'conv3x3s2_x3_fwd')
    return y


def conv_s2_x3_bwd_data(g, w_x3_s2dgrad, dx, mask=None, mode=0, accum=0, amax_dx=None):
    require_cuda(g, w_x3_s2dgrad, dx)
    B, H, W, Cin = dx.shape
    with _Timed('conv9s2_dgrad_x3', 2.0 * B * (H // 2) * (W // 2) * g.shape[3] * Cin * 9):
        check(_prep().pnnp_conv3x3s2_x3_bwd_data_amax_f32(ptr(g), g.shape[3], ptr(w_x3_s2dgrad), ptr(dx), Cin, ptr(mask), mode, accum, ptr(amax_dx),
                                                          B, H, W, stream()), 'conv3x3s2_x3_bwd_data')


def x3_wgrad_supported(H, W, cout, c1, c2=0):
    return bool(_prep().pnnp_x3_wgrad_supported(int(H), int(W), int(cout), int(c1), int(c2)))


def x3_wgrad_workspace_floats(B, H, W, cout, cin):
    return int(_prep().pnnp_x3_wgrad_workspace_floats(B, H, W, cout, cin))


def conv_x3_bwd_weight(g, cout, x1, c1, x2, dW, dbias, workspace, accumulate=0):
    """dW [cout][c1+c2][3][3] (+ dbias) on the bf16 matrix cores, fp32 operands split in three (same contract as conv_bwd_weight, taps=9)."""
    require_cuda(g, x1, dW, workspace)
    B, H, W, gcs = g.shape
    c2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_wgrad_x3', 2.0 * B * H * W * cout * (c1 + c2) * 9, 4.0 * B * H * W * (gcs + x1.shape[3] + c2)):
        check(_prep().pnnp_conv3x3_x3_bwd_weight_f32(ptr(g), gcs, cout, ptr(x1), x1.shape[3], c1, ptr(x2), c2, c2, ptr(dW), ptr(dbias),
                                                     B, H, W, int(accumulate), ptr(workspace), C.c_int64(workspace.numel()), stream()),
              'conv_x3_bwd_weight')


def conv_h2_bwd_weight(g, amax_g, cout, x1, amax_x1, c1, x2, amax_x2, dW, dbias, workspace, accumulate=0):
    """dW [cout][c1+c2][3][3] (+ dbias) on the fp16 matrix cores, both operands split in two scaled pieces (contract of conv_x3_bwd_weight + slots)."""
    require_cuda(g, x1, dW, workspace, amax_g, amax_x1)
    B, H, W, gcs = g.shape
    c2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_wgrad_h2', 2.0 * B * H * W * cout * (c1 + c2) * 9, 4.0 * B * H * W * (gcs + x1.shape[3] + c2)):
        check(_prep().pnnp_conv3x3_h2_bwd_weight_f32(ptr(g), gcs, cout, ptr(amax_g), ptr(x1), x1.shape[3], c1, ptr(amax_x1), ptr(x2), c2, c2, ptr(amax_x2),
                                                     ptr(dW), ptr(dbias), B, H, W, int(accumulate), ptr(workspace), C.c_int64(workspace.numel()), stream()),
              'conv_h2_bwd_weight')


def wino_supported(K, N):
    return bool(_prep().pnnp_wino_supported(int(K), int(N)))


def pack_conv_weight_wino(w, fwd, dgrad):
    co, ci = w.shape[:2]
    check(_prep().pnnp_pack_conv_weight_wino_f32(ptr(w), ptr(fwd), ptr(dgrad), co, ci, stream()), 'pack_conv_weight_wino')


def conv_wino_fwd(x1, x2, u_fwd, bias, y, cout, act, residual=None):
    """3x3 / stride 1 / pad 1 forward through the Winograd F(2x2,3x3) kernel (same contract as conv_fwd, taps=9)."""
    require_cuda(x1, x2, u_fwd, y)
    B, H, W, C1 = x1.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_fwd_wino', 2.0 * B * H * W * cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + cout)):
        check(_prep().pnnp_conv3x3_wino_fwd_f32(ptr(x1), C1, ptr(x2), C2, ptr(u_fwd), ptr(bias), ptr(residual), ptr(y), B, H, W, cout, act,
                                                stream()), 'conv_wino_fwd')
    return y


def conv_wino_bwd_data(g, u_dgrad, dx1, mask1=None, mode1=0, accum1=0, dx2=None, mask2=None, mode2=0, accum2=0):
    require_cuda(g, u_dgrad, dx1)
    B, H, W, Cout = g.shape
    C1 = dx1.shape[3]
    C2 = dx2.shape[3] if dx2 is not None else 0
    with _Timed('conv9_dgrad_wino', 2.0 * B * H * W * Cout * (C1 + C2) * 9, 4.0 * B * H * W * (C1 + C2 + Cout)):
        check(_prep().pnnp_conv3x3_wino_bwd_data_f32(ptr(g), Cout, ptr(u_dgrad), ptr(dx1), C1, ptr(mask1), mode1, accum1,
                                                     ptr(dx2), C2, ptr(mask2), mode2, accum2, B, H, W, stream()), 'conv_wino_bwd_data')


def wino_wgrad_supported(H, W, cout, c1, c2=0):
    return bool(_prep().pnnp_wino_wgrad_supported(int(H), int(W), int(cout), int(c1), int(c2)))


def wino_wgrad_workspace_floats(B, H, W, cout, cin):
    return int(_prep().pnnp_wino_wgrad_workspace_floats(B, H, W, cout, cin))


def conv_wino_bwd_weight(g, cout, x1, c1, x2, dW, dbias, workspace, accumulate=0):
    """dW [cout][c1+c2][3][3] (+ dbias) through the Winograd backward-weight kernel (same contract as conv_bwd_weight, taps=9)."""
    require_cuda(g, x1, dW, workspace)
    B, H, W, gcs = g.shape
    c2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv9_wgrad_wino', 2.0 * B * H * W * cout * (c1 + c2) * 9, 4.0 * B * H * W * (gcs + x1.shape[3] + c2)):
        check(_prep().pnnp_conv3x3_wino_bwd_weight_f32(ptr(g), gcs, cout, ptr(x1), x1.shape[3], c1, ptr(x2), c2, c2, ptr(dW), ptr(dbias),
                                                       B, H, W, int(accumulate), ptr(workspace), C.c_int64(workspace.numel()), stream()),
              'conv_wino_bwd_weight')


def conv_wino_bwd_data_res(g, u_dgrad, dx, addsrc, mask=None, mode=0):
    """dx = (conv_bwd_data(g) + addsrc) * act'(mask) through the Winograd kernel."""
    require_cuda(g, u_dgrad, dx, addsrc)
    B, H, W, Cout = g.shape
    C1 = dx.shape[3]
    with _Timed('conv9_dgrad_wino', 2.0 * B * H * W * Cout * C1 * 9, 4.0 * B * H * W * (2 * C1 + Cout)):
        check(_prep().pnnp_conv3x3_wino_bwd_data_res_f32(ptr(g), Cout, ptr(u_dgrad), ptr(dx), C1, ptr(addsrc), ptr(mask), mode,
                                                         B, H, W, stream()), 'conv_wino_bwd_data_res')


def conv_bwd_data_res(g, w_dgrad, dx, addsrc, mask=None, mode=0, taps=9):
    """dx = (conv_bwd_data(g) + addsrc) * act'(mask): backward through an identity shortcut."""
    require_cuda(g, w_dgrad, dx, addsrc)
    B, H, W, Cout = g.shape
    C1 = dx.shape[3]
    with _Timed('conv%d_dgrad' % taps, 2.0 * B * H * W * Cout * C1 * taps, 4.0 * B * H * W * (2 * C1 + Cout)):
        check(_prep().pnnp_conv_bwd_data_res_f32(ptr(g), Cout, ptr(w_dgrad), ptr(dx), C1, ptr(addsrc), ptr(mask), mode,
                                                 B, H, W, taps, stream()), 'conv_bwd_data_res')


def wgrad_workspace_floats(B, H, W, M, N, taps):
    return int(_prep().pnnp_wgrad_workspace_floats(B, H, W, M, N, taps))


def conv_bwd_weight(g, cout, x1, c1, x2, dW, dbias, taps, ws, accumulate=0):
    """g [B,H,W,>=cout] (first ``cout`` channels used), x1 [B,H,W,>=c1], x2 [B,H,W,C2] or None."""
    require_cuda(g, x1, dW, ws)
    B, H, W, gcs = g.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv%d_wgrad' % taps, 2.0 * B * H * W * cout * (c1 + C2) * taps, 4.0 * B * H * W * (c1 + C2 + cout)):
        check(_prep().pnnp_conv_bwd_weight_f32(ptr(g), gcs, cout, ptr(x1), x1.shape[3], c1, ptr(x2), C2, C2, ptr(dW), ptr(dbias),
                                               B, H, W, taps, accumulate, ptr(ws), _i64(ws.numel()), stream()), 'conv_bwd_weight')


def convt_fwd(x, w_packed, bias, y, cout):
    require_cuda(x, w_packed, y)
    B, H, W, Cin = x.shape
    with _Timed('convt_fwd', 8.0 * B * H * W * Cin * cout, 4.0 * B * H * W * (Cin + 4 * cout)):
        check(_prep().pnnp_convt2x2_fwd_f32(ptr(x), Cin, ptr(w_packed), ptr(bias), ptr(y), B, H, W, cout, stream()), 'convt_fwd')
    return y


def convt_bwd_data(g, w_dgrad, dx, mask=None, mode=0):
    require_cuda(g, w_dgrad, dx)
    B, H, W, Cin = dx.shape
    with _Timed('convt_dgrad', 8.0 * B * H * W * Cin * g.shape[3], 4.0 * B * H * W * (Cin + 4 * g.shape[3])):
        check(_prep().pnnp_convt2x2_bwd_data_f32(ptr(g), g.shape[3], ptr(w_dgrad), ptr(dx), Cin, ptr(mask), mode, B, H, W,
                                                 stream()), 'convt_bwd_data')


def set_persistent_split(n):
    """Workgroups per CU of the persistent forward / backward-data convolution kernels (include/pnnp_hip.h: pnnp_set_persistent_split):
    1 = one per CU with a static share (default, fastest alone), 4 = quarter shares handed out by the dispatcher (safe beside a
    collective kernel that occupies CUs: tests/test_gpu_overlap.py)."""
    L = _prep()
    L.pnnp_set_persistent_split.argtypes = [C.c_int]
    L.pnnp_set_persistent_split.restype = None
    L.pnnp_set_persistent_split(int(n))


def get_persistent_split():
    return int(_prep().pnnp_get_persistent_split())


X3G_PW, X3G_CT, X3G_S2 = 0, 1, 2        # geometry kinds of csrc/wgrad_x3g.hip: Conv2d 1x1, ConvTranspose2d 2x2 s2, Conv2d 3x3 s2


def x3g_wgrad_supported(kind, M, N):
    """Does the bf16x3 backward-weight kernel of the pointwise / strided layers have a tile configuration for (M, N)?"""
    return bool(_prep().pnnp_x3g_wgrad_supported(int(kind), int(M), int(N)))


def x3g_wgrad_workspace_floats(kind, B, UH, UW, M, N):
    return int(_prep().pnnp_x3g_wgrad_workspace_floats(int(kind), int(B), int(UH), int(UW), int(M), int(N)))


def convt_x3_bwd_weight(x, g, dW, ws, accumulate=0, dbias=None):
    """convt_bwd_weight on the bf16 matrix cores (fp32 operands split in three, csrc/wgrad_x3g.hip): Cin = M, Cout = N."""
    require_cuda(x, g, dW, ws, dbias)
    B, H, W, Cin = x.shape
    with _Timed('convt_wgrad_x3', 8.0 * B * H * W * Cin * g.shape[3], 4.0 * B * H * W * (Cin + 4 * g.shape[3])):
        check(_prep().pnnp_convt2x2_x3_bwd_weight_f32(ptr(x), Cin, ptr(g), g.shape[3], ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                      ptr(ws), _i64(ws.numel()), stream()), 'convt_x3_bwd_weight')


def conv_s2_x3_bwd_weight(g, x, dW, dbias, ws, accumulate=0):
    require_cuda(g, x, dW, ws)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_wgrad_x3', 2.0 * B * (H // 2) * (W // 2) * g.shape[3] * Cin * 9):
        check(_prep().pnnp_conv3x3s2_x3_bwd_weight_f32(ptr(g), g.shape[3], ptr(x), Cin, ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                       ptr(ws), _i64(ws.numel()), stream()), 'conv3x3s2_x3_bwd_weight')


def conv1x1_x3_bwd_weight(g, cout, x1, c1, x2, dW, dbias, ws, accumulate=0):
    """conv_bwd_weight(taps=1) on the bf16 matrix cores."""
    require_cuda(g, x1, dW, ws)
    B, H, W, gcs = g.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv1_wgrad_x3', 2.0 * B * H * W * cout * (c1 + C2), 4.0 * B * H * W * (c1 + C2 + cout)):
        check(_prep().pnnp_conv1x1_x3_bwd_weight_f32(ptr(g), gcs, cout, ptr(x1), x1.shape[3], c1, ptr(x2), C2, C2, ptr(dW), ptr(dbias),
                                                     B, H, W, accumulate, ptr(ws), _i64(ws.numel()), stream()), 'conv1x1_x3_bwd_weight')


def h2g_wgrad_supported(kind, M, N):
    return bool(_prep().pnnp_h2g_wgrad_supported(int(kind), int(M), int(N)))


def h2g_wgrad_workspace_floats(kind, B, UH, UW, M, N):
    return int(_prep().pnnp_h2g_wgrad_workspace_floats(int(kind), int(B), int(UH), int(UW), int(M), int(N)))


def convt_h2_bwd_weight(x, amax_x, g, amax_g, dW, ws, accumulate=0, dbias=None):
    """convt_x3_bwd_weight on the fp16x2 scheme (csrc/wgrad_h2g.hip): same shapes and workspace, + the operands' amax slots."""
    require_cuda(x, g, dW, ws, dbias, amax_x, amax_g)
    B, H, W, Cin = x.shape
    with _Timed('convt_wgrad_h2', 8.0 * B * H * W * Cin * g.shape[3], 4.0 * B * H * W * (Cin + 4 * g.shape[3])):
        check(_prep().pnnp_convt2x2_h2_bwd_weight_f32(ptr(x), Cin, ptr(amax_x), ptr(g), g.shape[3], ptr(amax_g), ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                      ptr(ws), _i64(ws.numel()), stream()), 'convt_h2_bwd_weight')


def conv_s2_h2_bwd_weight(g, amax_g, x, amax_x, dW, dbias, ws, accumulate=0):
    require_cuda(g, x, dW, ws, amax_g, amax_x)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_wgrad_h2', 2.0 * B * (H // 2) * (W // 2) * g.shape[3] * Cin * 9):
        check(_prep().pnnp_conv3x3s2_h2_bwd_weight_f32(ptr(g), g.shape[3], ptr(amax_g), ptr(x), Cin, ptr(amax_x), ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                       ptr(ws), _i64(ws.numel()), stream()), 'conv3x3s2_h2_bwd_weight')


def conv1x1_h2_bwd_weight(g, amax_g, cout, x1, amax_x1, c1, x2, amax_x2, dW, dbias, ws, accumulate=0):
    require_cuda(g, x1, dW, ws, amax_g, amax_x1)
    B, H, W, gcs = g.shape
    C2 = x2.shape[3] if x2 is not None else 0
    with _Timed('conv1_wgrad_h2', 2.0 * B * H * W * cout * (c1 + C2), 4.0 * B * H * W * (c1 + C2 + cout)):
        check(_prep().pnnp_conv1x1_h2_bwd_weight_f32(ptr(g), gcs, cout, ptr(amax_g), ptr(x1), x1.shape[3], c1, ptr(amax_x1), ptr(x2), C2, C2, ptr(amax_x2), ptr(dW), ptr(dbias),
                                                     B, H, W, accumulate, ptr(ws), _i64(ws.numel()), stream()), 'conv1x1_h2_bwd_weight')


def convt_bwd_weight(x, g, dW, ws, accumulate=0, dbias=None):
    """dW (and dbias = the channel sums of g, gathered by the same kernel while g is staged) of ConvTranspose2d(k2, s2)."""
    require_cuda(x, g, dW, ws, dbias)
    B, H, W, Cin = x.shape
    with _Timed('convt_wgrad', 8.0 * B * H * W * Cin * g.shape[3], 4.0 * B * H * W * (Cin + 4 * g.shape[3])):
        check(_prep().pnnp_convt2x2_bwd_weight_f32(ptr(x), Cin, ptr(g), g.shape[3], ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                   ptr(ws), _i64(ws.numel()), stream()), 'convt_bwd_weight')


def conv_s2_fwd(x, w_packed, bias, y, cout, act=0):
    """Conv2d 3x3 stride 2 pad 1: x [B,H,W,Cin] -> y [B,H/2,W/2,cout]."""
    require_cuda(x, w_packed, y)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_fwd', 2.0 * B * (H // 2) * (W // 2) * cout * Cin * 9):
        check(_prep().pnnp_conv3x3s2_fwd_f32(ptr(x), Cin, ptr(w_packed), ptr(bias), ptr(y), B, H, W, cout, act, stream()),
              'conv3x3s2_fwd')
    return y


def pack_conv_s2_dgrad(w, dst):
    co, ci = w.shape[:2]
    check(_prep().pnnp_pack_conv3x3s2_dgrad_f32(ptr(w), ptr(dst), co, ci, stream()), 'pack_conv3x3s2_dgrad')


def conv_s2_bwd_data(g, w_s2dgrad, dx, mask=None, mode=0, accum=0):
    require_cuda(g, w_s2dgrad, dx)
    B, H, W, Cin = dx.shape
    with _Timed('conv9s2_dgrad', 2.0 * B * (H // 2) * (W // 2) * g.shape[3] * Cin * 9):
        check(_prep().pnnp_conv3x3s2_bwd_data_f32(ptr(g), g.shape[3], ptr(w_s2dgrad), ptr(dx), Cin, ptr(mask), mode, accum,
                                                  B, H, W, stream()), 'conv3x3s2_bwd_data')


def conv_s2_bwd_weight(g, x, dW, dbias, ws, accumulate=0):
    require_cuda(g, x, dW, ws)
    B, H, W, Cin = x.shape
    with _Timed('conv9s2_wgrad', 2.0 * B * (H // 2) * (W // 2) * g.shape[3] * Cin * 9):
        check(_prep().pnnp_conv3x3s2_bwd_weight_f32(ptr(g), g.shape[3], ptr(x), Cin, ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                    ptr(ws), _i64(ws.numel()), stream()), 'conv3x3s2_bwd_weight')


# ---- the thin ends of the networks (csrc/thin.hip): the 1x1 head and the first layer's backward-weight
def head_supported(cin, cout, npix):
    return bool(_prep().pnnp_head_supported(int(cin), int(cout), _i64(npix)))


def head_bwd_workspace_floats(cin):
    return int(_prep().pnnp_head_bwd_workspace_floats(int(cin)))


def head_fwd(x, weight, bias, out, residual=None):
    """out NCHW [B,cout,H,W] = conv1x1(x NHWC [B,H,W,>=cin]; weight [cout,cin,1,1], bias) (+ residual NCHW)."""
    require_cuda(x, weight, bias, out)
    B, H, W, xcs = x.shape
    cout, cin = weight.shape[0], weight.shape[1]
    with _Timed('head_fwd', 2.0 * B * H * W * cin * cout, 4.0 * B * H * W * (cin + cout)):
        check(_prep().pnnp_head_fwd_f32(ptr(x), xcs, cin, ptr(weight), ptr(bias), ptr(residual), ptr(out), B, H, W, cout, stream()), 'head_fwd')
    return out


def head_fwd_et(x, weight, bias, out, residual=None):
    """head_fwd with the element type of ``x``: a torch.float16 NHWC map is widened exactly in the kernel; everything else stays float32"""
    if x.dtype not in (torch.float16, torch.float32):
        raise _lib.PnnpError(f'head_fwd_et: x is {x.dtype}: torch.float16 or torch.float32')
    for t in (weight, bias, out, residual):
        if t is not None and t.dtype != torch.float32:
            raise _lib.PnnpError(f'head_fwd_et: the head is float32, got {t.dtype}')
    require_cuda(x, weight, bias, out, residual)
    B, H, W, xcs = x.shape
    cout, cin = weight.shape[0], weight.shape[1]
    s16 = int(x.dtype == torch.float16)
    with _Timed('head_fwd_et', 2.0 * B * H * W * cin * cout, B * H * W * ((2.0 if s16 else 4.0) * cin + 4.0 * cout)):
        check(_prep().pnnp_head_fwd_et(ptr(x), xcs, cin, ptr(weight), ptr(bias), ptr(residual), ptr(out), s16, B, H, W, cout, stream()), 'head_fwd_et')
    return out


def head_bwd(g, x, weight, gx, dW, dbias, ws, mode=0, accumulate=0, amax_gx=None):
    """Backward of the 1x1 head in one pass: gx [B,H,W,>=cin] = (g W) * act'(x), dW [cout,cin,1,1] and dbias (+)=.
    g [B,H,W,gcs>=4] (first cout channels), x [B,H,W,>=cin] the head's input (an activation output when mode != 0)."""
    require_cuda(g, x, weight, gx, dW, ws)
    B, H, W, gcs = g.shape
    cout, cin = weight.shape[0], weight.shape[1]
    with _Timed('head_bwd', 4.0 * B * H * W * cin * cout, 4.0 * B * H * W * (2 * cin + cout)):
        check(_prep().pnnp_head_bwd_amax_f32(ptr(g), gcs, ptr(x), x.shape[3], cin, ptr(weight), ptr(gx), gx.shape[3], mode, ptr(dW), ptr(dbias),
                                             B, H, W, cout, accumulate, ptr(ws), _i64(ws.numel()), ptr(amax_gx), stream()), 'head_bwd')


def first_wgrad_supported(cin, cout, H, W):
    return bool(_prep().pnnp_first_wgrad_supported(int(cin), int(cout), int(H), int(W)))


def first_wgrad_workspace_floats(cout):
    return int(_prep().pnnp_first_wgrad_workspace_floats(int(cout)))


def first_fwd(x, weight, bias, y, act, amax_y=None):
    """y [B,H,W,>=cout] = act(conv3x3(x [B,H,W,xcs>=4], zero in channels cin..3; weight [cout,cin,3,3]) + bias) on the streaming kernel.
    ``amax_y``: an amax slot of the fp16x2 family (max |y| is raised into it)."""
    require_cuda(x, weight, y)
    B, H, W, xcs = x.shape
    cout, cin = weight.shape[0], weight.shape[1]
    with _Timed('first_fwd', 2.0 * B * H * W * cout * cin * 9, 4.0 * B * H * W * (cin + cout)):
        check(_prep().pnnp_first_fwd_amax_f32(ptr(x), xcs, cin, ptr(weight), ptr(bias), ptr(y), y.shape[3], B, H, W, cout, act, ptr(amax_y), stream()), 'first_fwd')
    return y


def first_fwd_et(x, weight, bias, y, act, amax_y=None):
    """first_fwd with the element type of ``y``: a torch.float16 ``y`` receives float16(the float32 value first_fwd stores); ``x`` stays float32"""
    if x.dtype != torch.float32 or y.dtype not in (torch.float16, torch.float32):
        raise _lib.PnnpError(f'first_fwd_et: x float32 and y torch.float16 or float32, got {x.dtype} -> {y.dtype}')
    require_cuda(x, weight, y)
    B, H, W, xcs = x.shape
    cout, cin = weight.shape[0], weight.shape[1]
    d16 = int(y.dtype == torch.float16)
    with _Timed('first_fwd_et', 2.0 * B * H * W * cout * cin * 9, B * H * W * (4.0 * cin + (2.0 if d16 else 4.0) * cout)):
        check(_prep().pnnp_first_fwd_amax_et(ptr(x), xcs, cin, ptr(weight), ptr(bias), ptr(y), y.shape[3], B, H, W, cout, act, ptr(amax_y), d16, stream()), 'first_fwd_et')
    return y


def first_bwd_weight(g, cout, x, cin, dW, dbias, ws, accumulate=0):
    """dW [cout,cin,3,3], dbias (+)= for the first 3x3 convolution: x [B,H,W,xcs>=4] zero in channels cin..3, g [B,H,W,>=cout]."""
    require_cuda(g, x, dW, ws)
    B, H, W, gcs = g.shape
    with _Timed('first_wgrad', 2.0 * B * H * W * cout * cin * 9, 4.0 * B * H * W * (cin + cout)):
        check(_prep().pnnp_first_bwd_weight_f32(ptr(g), gcs, cout, ptr(x), x.shape[3], cin, ptr(dW), ptr(dbias), B, H, W, accumulate,
                                                ptr(ws), _i64(ws.numel()), stream()), 'first_bwd_weight')


def maxpool_fwd(x, y, codes=None):
    """MaxPool2d(2); with ``codes`` (uint8 [B,H/2,W/2,C]) it also records argmax + signs for maxpool_bwd(codes=...)."""
    require_cuda(x, y, codes)
    B, H, W, Cc = x.shape
    if codes is not None:
        check(_prep().pnnp_maxpool2_fwd_codes_f32(ptr(x), ptr(y), ptr(codes), B, H, W, Cc, stream()), 'maxpool_fwd_codes')
    else:
        check(_prep().pnnp_maxpool2_fwd_f32(ptr(x), ptr(y), B, H, W, Cc, stream()), 'maxpool_fwd')
    return y


def maxpool_fwd_f16(x, y):
    """MaxPool2d(2) of a torch.float16 NHWC map into a torch.float16 one (the fp16-storage eval forward; no codes: nothing runs backward)"""
    if x.dtype != torch.float16 or y.dtype != torch.float16:
        raise _lib.PnnpError(f'maxpool_fwd_f16: torch.float16 maps, got {x.dtype} -> {y.dtype}')
    require_cuda(x, y)
    B, H, W, Cc = x.shape
    with _Timed('maxpool_fwd_f16', 0.0, 2.5 * B * H * W * Cc):
        check(_prep().pnnp_maxpool2_fwd_f16(ptr(x), ptr(y), B, H, W, Cc, stream()), 'maxpool_fwd_f16')
    return y


def maxpool_bwd(x, gy, gx, act_mode, accumulate, codes=None, amax_gx=None):
    """gx (+)= routed(gy) * act'(x); with the forward pass's ``codes`` the full-resolution x is not read again.  ``amax_gx`` (an amax slot of
    the fp16x2 family): fused into the codes kernel, a kernel of its own behind the other."""
    require_cuda(x, gy, gx, codes)
    B, H, W, Cc = x.shape
    if codes is not None:
        check(_prep().pnnp_maxpool2_bwd_codes_amax_f32(ptr(codes), ptr(gy), ptr(gx), B, H, W, Cc, act_mode, accumulate, ptr(amax_gx), stream()), 'maxpool_bwd_codes')
    else:
        check(_prep().pnnp_maxpool2_bwd_f32(ptr(x), ptr(gy), ptr(gx), B, H, W, Cc, act_mode, accumulate, stream()), 'maxpool_bwd')
        if amax_gx is not None:
            amax(gx, amax_gx)


def nchw_to_nhwc(src, dst, cp, reflect_pad=0, amax=None):
    """NCHW -> zero-padded-channel NHWC; ``reflect_pad`` > 0: dst is the frame reflect-padded by that many pixels on every side.
    ``amax``: an amax slot of the fp16x2 family (max |element| is raised into it)."""
    require_cuda(src, dst)
    B, Cc, H, W = src.shape
    check(_prep().pnnp_nchw_to_nhwc_reflect_amax_f32(ptr(src), ptr(dst), B, Cc, H, W, cp, int(reflect_pad), ptr(amax), stream()), 'nchw_to_nhwc')
    return dst


def _tile_fn(name):
    L = _prep()
    if not hasattr(L, name):
        raise _lib.PnnpError(f'{_lib.LIB_PATH} has no {name}: rebuild the library (tools/build.py)')
    return getattr(L, name)


def tile_crop(frame, grid, t0, nt, nchw=None, nhwc=None, amax=None):
    """Tiles t0 .. t0 + nt of ``grid`` (tiles.TileGrid) out of ``frame`` [1,C,h,w] in one launch: ``nchw`` [nt,C,P,P] and / or ``nhwc``
    [nt,P,pitch,Cp] (the zero-padded-channel layout of nchw_to_nhwc; pitch = its third dimension).  ``amax``: as in nchw_to_nhwc."""
    require_cuda(frame, nchw, nhwc, amax)
    _, Cc, H, W = frame.shape
    P = grid.patch_size
    if (H, W) != (grid.h, grid.w) or not frame.is_contiguous() or frame.dtype != torch.float32:
        raise _lib.PnnpError(f'tile_crop: frame {tuple(frame.shape)} ({frame.dtype}) is not the contiguous float32 {grid.h} x {grid.w} frame of the grid')
    if nchw is not None and (tuple(nchw.shape) != (nt, Cc, P, P) or not nchw.is_contiguous()):
        raise _lib.PnnpError(f'tile_crop: nchw must be contiguous [{nt},{Cc},{P},{P}], got {tuple(nchw.shape)}')
    pitch = cp = 0
    if nhwc is not None:
        if nhwc.dim() != 4 or tuple(nhwc.shape[:2]) != (nt, P) or not nhwc.is_contiguous():
            raise _lib.PnnpError(f'tile_crop: nhwc must be contiguous [{nt},{P},pitch,Cp], got {tuple(nhwc.shape)}')
        pitch, cp = nhwc.shape[2], nhwc.shape[3]
    check(_tile_fn('pnnp_tile_crop_f32')(ptr(frame), Cc, H, W, P, grid.base, int(t0), int(nt), ptr(nchw), ptr(nhwc), pitch, cp, ptr(amax), stream()),
          'tile_crop')


def tile_merge(tiles, frame, grid, t0, nt, ratio=None, clamp=False):
    """The interiors of tiles t0 .. t0 + nt (``tiles`` [nt,C,P,P]) into ``frame`` [1,C,h,w]: only the elements those tiles own are written.
    ``ratio``: None, a float or a CUDA scalar tensor; ``clamp``: to [0, 1] after the product."""
    require_cuda(tiles, frame)
    _, Cc, H, W = frame.shape
    P = grid.patch_size
    if (H, W) != (grid.h, grid.w) or not frame.is_contiguous() or frame.dtype != torch.float32:
        raise _lib.PnnpError(f'tile_merge: frame {tuple(frame.shape)} ({frame.dtype}) is not the contiguous float32 {grid.h} x {grid.w} frame of the grid')
    if tuple(tiles.shape) != (nt, Cc, P, P) or not tiles.is_contiguous() or tiles.dtype != torch.float32:
        raise _lib.PnnpError(f'tile_merge: tiles must be contiguous float32 [{nt},{Cc},{P},{P}], got {tuple(tiles.shape)} ({tiles.dtype})')
    r_dev = None
    if torch.is_tensor(ratio) and ratio.is_cuda:                   # stays on the device: nothing here synchronises
        r_dev = ratio.reshape(-1)[:1].float().contiguous()
    r = 1.0 if (ratio is None or r_dev is not None) else float(torch.as_tensor(ratio).reshape(-1)[0])
    check(_tile_fn('pnnp_tile_merge_f32')(ptr(tiles), ptr(frame), Cc, H, W, P, grid.base, int(t0), int(nt), C.c_float(r), ptr(r_dev),
                                          int(bool(clamp)), stream()), 'tile_merge')
    return frame


def nhwc_to_nchw(src, dst, residual=None):
    require_cuda(src, dst, residual)
    B, Cc, H, W = dst.shape
    check(_prep().pnnp_nhwc_to_nchw_f32(ptr(src), ptr(residual), ptr(dst), B, Cc, H, W, src.shape[3], stream()), 'nhwc_to_nchw')
    return dst


def channel_sum(x, out, ws, accumulate=0):
    require_cuda(x, out, ws)
    Cc = x.shape[-1]
    check(_prep().pnnp_channel_sum_f32(ptr(x), ptr(out), _i64(x.numel() // Cc), Cc, accumulate, ptr(ws), stream()), 'channel_sum')


def l1_clamp_loss(pred, hr, grad_nhwc, loss_out, ws, scale=None, clamp_target=False, grad_weight=1.0):
    """``scale`` [B] (or None): the `ori` branch of the train loop, pred * ratio before the loss (trainer_SID.py:97-99).
    ``clamp_target``: clamp ``hr`` to [0,1] inside the kernel (preprocess's imgs_hr.clamp(0,1) under dst.clip, trainer_SID.py:485).
    ``grad_weight`` multiplies dL/dpred only (uneven data-parallel shards of a global batch)."""
    require_cuda(pred, hr, loss_out, ws, scale)
    B, Cc, H, W = pred.shape
    cp = grad_nhwc.shape[3] if grad_nhwc is not None else 0
    check(_prep().pnnp_l1_clamp_loss_w_f32(ptr(pred), ptr(hr), ptr(scale), ptr(grad_nhwc), ptr(loss_out), B, Cc, H, W, cp, ptr(ws),
                                           int(bool(clamp_target)), C.c_float(grad_weight), stream()), 'l1_clamp_loss')


UNET_LOSS_KEYS = ('charbonnier', 'pyramid', 'grad')
UNET_LOSS_TERMS = 5                                  # the four pyramid level means before weighting, then the Sobel term
UNET_LOSS_LEVEL_WEIGHTS = (1.0, 0.5, 0.25, 0.125)    # Pyramid_Loss(rate=0.5); their sum 1.875 divides (norm=True)


def unet_loss_options(loss):
    """A loss setting -- a mapping with the keys ``charbonnier`` (bool), ``pyramid`` (bool), ``grad`` (the weight of the Sobel edge term, >= 0)
    -- checked and completed with the defaults: ``HipTrainStep(loss=)``, `hyper.loss` of a run file.  Touches no device."""
    if not hasattr(loss, 'keys'):
        raise _lib.PnnpError(f'loss: expected a mapping with keys from {UNET_LOSS_KEYS}, got {type(loss).__name__}')
    unknown = sorted(set(loss.keys()) - set(UNET_LOSS_KEYS))
    if unknown:
        raise _lib.PnnpError(f'loss: unknown keys {unknown}; the keys are {UNET_LOSS_KEYS}')
    for k in ('charbonnier', 'pyramid'):
        if not isinstance(loss.get(k, False), (bool, np.bool_)):
            raise _lib.PnnpError(f'loss: {k} must be a bool, got {loss[k]!r}')
    grad = loss.get('grad', 0.0)
    if isinstance(grad, (bool, np.bool_)) or not isinstance(grad, (int, float, np.integer, np.floating)) or not 0.0 <= float(grad) < float('inf'):
        raise _lib.PnnpError(f'loss: grad must be a finite number >= 0, got {grad!r}')
    out = dict(charbonnier=bool(loss.get('charbonnier', False)), pyramid=bool(loss.get('pyramid', False)), grad=float(grad))
    if out['pyramid'] and out['grad'] > 0:
        raise _lib.PnnpError('loss: the Sobel edge term (grad > 0) together with the pyramid is not defined by the reference (losses/base_loss.py:80-107)')
    return out


def unet_loss_workspace_floats(B):
    fn = _tile_fn('pnnp_unet_loss_workspace_floats')
    fn.restype = C.c_int64
    return int(fn(int(B)))


def unet_loss(pred, hr, grad_nhwc, loss_out, ws, scale=None, clamp_target=False, grad_weight=1.0, clamp_pred=True, charbonnier=False,
              pyramid=False, grad=0.0, terms=None, grad_nchw=None, recon=True):
    """Unet_Loss (losses/base_loss.py:33-107) and dL/dpred in streaming passes (csrc/unet_loss.hip), beside ``l1_clamp_loss`` and with its
    semantics for ``scale``, ``clamp_target`` and ``grad_weight``.  ``clamp_pred``: True = the trainer's call site, which passes
    pred.clamp(0, 1) (trainer_SID.py:99); False = the bare module.  ``charbonnier`` / ``pyramid``: ``Unet_Loss(charbonnier)(low, high, pyramid)``;
    ``grad`` > 0 adds grad * ``grad_loss`` (the Sobel edge term), which the reference keeps commented out of ``loss()``.
    ``loss_out`` [1 + B] = [loss, sse_0 ..]; ``terms`` [5] (optional) = the level means before weighting and the Sobel term; the gradient goes to
    ``grad_nhwc`` [B,H,W,4 or 8] and / or ``grad_nchw`` [B,C,H,W] (either may be None).  ``ws``: ``unet_loss_workspace_floats(B)`` floats.
    ``recon=False``: the edge term alone.  With every option off: ``l1_clamp_loss``'s loss, SSE and gradient bit for bit.
    Refused before any launch: pyramid with H % 8 or W % 8 (deviation: the reference floors odd sizes), pyramid with grad > 0."""
    opt = unet_loss_options(dict(charbonnier=charbonnier, pyramid=pyramid, grad=grad))
    B, Cc, H, W = pred.shape
    if opt['pyramid'] and (H % 8 or W % 8):
        raise _lib.PnnpError(f'unet_loss: the pyramid needs H and W to be multiples of 8, got {H} x {W}')
    if not recon and not opt['grad'] > 0:
        raise _lib.PnnpError('unet_loss: recon=False needs grad > 0')
    require_cuda(pred, hr, loss_out, ws, scale, grad_nhwc, grad_nchw, terms)
    for name, t, shape in (('pred', pred, (B, Cc, H, W)), ('hr', hr, (B, Cc, H, W)), ('grad_nchw', grad_nchw, (B, Cc, H, W)),
                           ('grad_nhwc', grad_nhwc, (B, H, W, grad_nhwc.shape[3] if grad_nhwc is not None and grad_nhwc.dim() == 4 else -1)),
                           ('loss_out', loss_out, (1 + B,)), ('terms', terms, (UNET_LOSS_TERMS,)), ('scale', scale, (B,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.PnnpError(f'unet_loss: {name} must be contiguous float32 {shape}, got {tuple(t.shape)} ({t.dtype})')
    cp = grad_nhwc.shape[3] if grad_nhwc is not None else 0
    check(_tile_fn('pnnp_unet_loss_f32')(ptr(pred), ptr(hr), ptr(scale), ptr(grad_nhwc), ptr(grad_nchw), ptr(loss_out), ptr(terms), B, Cc, H, W, cp,
                                         ptr(ws), _i64(ws.numel()), int(bool(clamp_target)), int(bool(clamp_pred)), C.c_float(grad_weight),
                                         int(opt['charbonnier']), int(opt['pyramid']), C.c_float(opt['grad']), int(bool(recon)), stream()), 'unet_loss')


def adam_step(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    require_cuda(p, g, m, v)
    check(_prep().pnnp_adam_step_f32(ptr(p), ptr(g), ptr(m), ptr(v), _i64(p.numel()), C.c_float(lr), C.c_float(beta1),
                                     C.c_float(beta2), C.c_float(eps), int(step), C.c_float(grad_scale), stream()), 'adam_step')
