"""Dark-frame calibration of a camera's noise table on the device (csrc/calib.hip): the first step of the method, which the reference
does not ship -- its tables (``process._SPEC``, ``process._REG``) arrived ready-made.  The estimators are defined here and restated
in float64 numpy by tests/_calib_ref.py.

    DarkStack        streams a stack of dark (bias) frames, uint16 Bayer mosaics, once: exact integer sum, sum of squares and per-frame
                     row sums; from them the dark-shading map, the variance map and the black-level error
    residuals        frame - dark shading - row offset, float32
    fit_dark         one ISO: a row of the per-ISO table (``lam``, ``sigGs``, ``sigTL``, ``sigR``, their spreads, ``biassig``) and the shading
    fit_regression   several ISOs: a row of the regression table (log sigma against log K)
    row_denoise      the reference's utils/isp_algos.py:84-99 (its one calibration step, run over the dark-shading files)

``process.register_camera`` puts the results where the samplers look.  The system gain ``K`` is the caller's: photon transfer from flat
fields is not estimated here (a ``DarkStack`` over a flat stack returns the mean and variance maps it would need).

The row statistic.  The sampler draws one row offset per row of a PACKED plane (``randn(C, H, 1)``): per (sensor row, column parity) of the
mosaic.  That is the unit measured here -- ``rowsum[f][y][c]`` sums the pixels of sensor row y whose column has parity c -- so that a
calibration reproduces what ``generate_noisy_torch`` will draw.  ``row_denoise`` is the per-sensor-row view (the reference's), which
averages the two parities of a row.

Device tensors in; the per-frame statistics (a few numbers per frame and row) are brought to the host, where every table entry is float64
arithmetic from the exact integers.  There is no CPU implementation.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, isp_ops, losses
from ._lib import PnnpError

MAX_FRAMES = 32768        # 32768 * 65535 < 2^31: the int32 sum
MAX_W = 65536             # 32768 * 65535 < 2^31: the int32 row sum of one column parity
BILATERAL_D, BILATERAL_SC = 25, 10.0


def _entry(name):
    try:
        return getattr(_lib.lib(), name)
    except AttributeError:
        raise PnnpError(f'{_lib.LIB_PATH} has no {name}: an older build of the library; rebuild it') from None


def _check_hw(H, W, what):
    if int(H) != H or int(W) != W or H < 2 or W < 2 or H % 2 or W % 2:
        raise PnnpError(f'{what}: a Bayer mosaic has even sides of at least 2, got {H}x{W}')
    if W > MAX_W:
        raise PnnpError(f'{what}: the width is at most {MAX_W} (the int32 row sums), got {W}')
    return int(H), int(W)


def _check_frames(frames, H, W, what):
    """the refusals that need no device: -> the chunk as [n,H,W]"""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint16:
        raise PnnpError(f'{what}: expected a uint16 tensor, got {getattr(frames, "dtype", type(frames).__name__)}')
    if frames.dim() == 2:
        frames = frames[None]
    if frames.dim() != 3 or frames.shape[0] < 1 or (H is not None and tuple(frames.shape[1:]) != (H, W)):
        raise PnnpError(f'{what}: expected [n,H,W]' + (f' with H x W = {H}x{W}' if H is not None else '') + f', got {tuple(frames.shape)}')
    if not frames.is_contiguous():
        raise PnnpError(f'{what}: the stack must be contiguous (a strided view would be copied frame by frame; copy it yourself if you mean that)')
    return frames


class DarkStack:
    """The exact integer statistics of a stack of dark frames, streamed chunk by chunk: ``add(frames_u16)`` takes [n,H,W] (or [H,W]) uint16 on
    the device, contiguous, and may be called repeatedly; at most 32768 frames in all.

        n        frames so far
        sum      int32 [H,W]     sum_f v                        sumsq    int64 [H,W]   sum_f v^2
        rowsum   int32 [n,H,2]   sum over the columns of parity c of v, per frame and sensor row
    """

    def __init__(self, H, W, device='cuda'):
        self.H, self.W = _check_hw(H, W, 'DarkStack')
        self.device = torch.device(device)
        self.n = 0
        self._sum = self._sumsq = None
        self._rows = []

    def add(self, frames_u16):
        fr = _check_frames(frames_u16, self.H, self.W, 'DarkStack.add')
        n = fr.shape[0]
        if self.n + n > MAX_FRAMES:
            raise PnnpError(f'DarkStack.add: {self.n} + {n} frames, at most {MAX_FRAMES} in all (the int32 sum)')
        _lib.require_cuda(fr)
        if self._sum is None:
            self.device = fr.device
            self._sum = torch.zeros(self.H, self.W, dtype=torch.int32, device=fr.device)
            self._sumsq = torch.zeros(self.H, self.W, dtype=torch.int64, device=fr.device)
        elif fr.device != self._sum.device:
            raise PnnpError(f'DarkStack.add: the chunk is on {fr.device}, the stack on {self._sum.device}')
        rows = torch.empty(n, self.H, 2, dtype=torch.int32, device=fr.device)
        with torch.cuda.device(fr.device):
            _lib.check(_entry('pnnp_calib_accum_u16')(_lib.ptr(fr), n, self.H, self.W, _lib.ptr(self._sum), _lib.ptr(self._sumsq), _lib.ptr(rows),
                                                      _lib.stream()), 'calib_accum')
        self._rows.append(rows)
        self.n += n
        return self

    def _need(self, least=1):
        if self.n < least:
            raise PnnpError(f'DarkStack: {self.n} frames, this needs at least {least}')

    def _f64(self, v):
        """a divisor as a device tensor: a true IEEE division (a tensor divided by a Python scalar is multiplied by its reciprocal)"""
        return torch.tensor(float(v), dtype=torch.float64, device=self._sum.device)

    @property
    def sum(self):
        self._need()
        return self._sum

    @property
    def sumsq(self):
        self._need()
        return self._sumsq

    @property
    def rowsum(self):
        self._need()
        if len(self._rows) > 1:
            self._rows = [torch.cat(self._rows)]
        return self._rows[0]

    def dark_shading(self):
        """float32 of the float64 ``sum / n``: the map the crop kernel subtracts"""
        return (self.sum.to(torch.float64) / self._f64(self.n)).to(torch.float32)

    def var_map(self):
        """float64 [H,W]: the unbiased variance over the frames, (n sumsq - sum^2) / (n (n - 1)), the numerator in exact int64"""
        self._need(2)
        s = self._sum.to(torch.int64)
        return (self.n * self._sumsq - s * s).to(torch.float64) / self._f64(self.n * (self.n - 1))

    def plane_sums(self):
        """int64 [H,2] on the host: sum over the columns of parity c of ``sum``"""
        return self.sum.view(self.H, self.W // 2, 2).sum(dim=1, dtype=torch.int64).cpu().numpy()

    def black_level_error(self, bl):
        """float64 [4] on the host, in ``raw2bayer``'s plane order (R (0,0), G1 (0,1), B (1,1), G2 (1,0)): the planes' means of ``sum / n`` minus ``bl``"""
        ps = self.plane_sums().reshape(self.H // 2, 2, 2).sum(axis=0)                  # [row parity][column parity], exact
        cnt = float(self.n) * (self.H // 2) * (self.W // 2)
        return np.array([ps[0, 0], ps[0, 1], ps[1, 1], ps[1, 0]], np.float64) / cnt - float(bl)


def residuals(frames_u16, ds, rowoff):
    """float32 [n,H,W]: ``(float(v) - ds[y][x]) - rowoff[f][y][x & 1]``, two float32 subtractions in that order.  ``ds`` float32 [H,W],
    ``rowoff`` float32 [n,H,2], all on the device."""
    fr = _check_frames(frames_u16, None, None, 'residuals')
    n, H, W = fr.shape
    _check_hw(H, W, 'residuals')
    if n > MAX_FRAMES:
        raise PnnpError(f'residuals: at most {MAX_FRAMES} frames per call, got {n}')
    for t, shape, what in ((ds, (H, W), 'ds'), (rowoff, (n, H, 2), 'rowoff')):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise PnnpError(f'residuals: {what} must be a float32 tensor {shape}, got {getattr(t, "dtype", type(t).__name__)} {tuple(getattr(t, "shape", ()))}')
    _lib.require_cuda(fr, ds, rowoff)
    out = torch.empty(n, H, W, dtype=torch.float32, device=fr.device)
    with torch.cuda.device(fr.device):
        _lib.check(_entry('pnnp_calib_residual_u16')(_lib.ptr(fr), n, H, W, _lib.ptr(ds.contiguous()), _lib.ptr(rowoff.contiguous()), _lib.ptr(out),
                                                     _lib.stream()), 'calib_residual')
    return out


# ---------------------------------------------------------------------------- the fit (host float64)
def probabilities(nq):
    """p_k = (k + 0.5) / nq as float32: what the quantile kernel is asked for and where the theoretical quantiles are taken"""
    return ((np.arange(nq, dtype=np.float64) + 0.5) / nq).astype(np.float32)


def slope(t, q):
    """least-squares slope of q [.., nq] on the theoretical quantiles t [nq]: sum(q t0) / sum(t0^2), t0 = t - mean t"""
    t0 = t - t.mean()
    return (q * t0).sum(axis=-1) / (t0 * t0).sum()


def corr(t, q):
    """Pearson correlation of q [.., nq] with t [nq]"""
    t0 = t - t.mean()
    q0 = q - q.mean(axis=-1, keepdims=True)
    return (q0 * t0).sum(axis=-1) / np.sqrt((t0 * t0).sum() * (q0 * q0).sum(axis=-1))


def _spread(x):
    return float(np.std(x, ddof=1)) if len(x) > 1 else 0.0


def fit_dark(frames, iso, K, wp, bl, nq=1000, lam_grid=None, darkshading=None):
    """One ISO's row of the noise table from a stack of dark frames.

    ``frames``: a uint16 device tensor [N,H,W], or a list of such chunks (it is walked twice).  ``K`` is the system gain at this ISO (the
    caller's), ``wp`` / ``bl`` the white and black level.  ``darkshading``: a float32 [H,W] map measured elsewhere; without it the map comes
    from this stack (N >= 2) and every variance is corrected by c = N / (N - 1) for the mean that was subtracted.  With it c = 1 and N = 1 works.

    All of it in DN.  With the exact integers ``sum``, ``rowsum`` of the stack, on the host in float64:
        rowoff[f][y][c] = rowsum[f][y][c] / (W/2) - (sum over the columns of parity c of sum[y][x]) / (N W/2)
                          (a given map: minus the float64 mean of its row and parity) -- PER SENSOR ROW AND COLUMN PARITY, i.e. per row of a
                          packed plane, the unit the sampler draws (see the module docstring); the kernel gets its float32
        res             = (v - ds) - rowoff, float32 (``residuals``)
        v_res[f]        = mean(res[f]^2) - mean(res[f])^2, reduced in float64 on the device
        v_row[f]        = the unbiased variance of rowoff[f] over its 2H values
        sigR_f          = sqrt(max(c v_row[f] - c v_res[f] / (W/2), 0)): a row mean still holds the read noise of its W/2 pixels
        m_f             = mean rowoff[f];  biassig = std_f(m_f, ddof=1)
        q[f]            = the quantiles of res[f] at p_k = (k + 0.5) / nq (float32), linear interpolation: the exact multi-rank select of
                          ``losses.quantile`` gives the two order statistics and the weight of every p_k, and the host interpolates with
                          ``torch.lerp`` -- CPU ``torch.quantile(res[f], p)`` bit for bit (the kernel's own interpolation is within an ulp of it)
        lam             = the first maximiser over ``lam_grid`` (default linspace(-0.3, 0.3, 121)) of mean_f corr(tukeylambda.ppf(p, lam), q[f])
        sigGs_f         = sqrt(c) slope(norm.ppf(p), q[f]);  sigTL_f = sqrt(c) slope(tukeylambda.ppf(p, lam), q[f])
    and each table entry is the mean over the frames, its ``*sig`` the ddof=1 standard deviation over the frames (0 for one frame).

    Returns the table row (Kmax = K, lam, sigGs, sigGssig, sigTL, sigTLsig, sigR, sigRsig, bias = 0, biassig, q = 1 / (wp + 1), wp, bl)
    plus ``iso``, ``n_frames``, ``darkshading`` (float32, device), ``black_level_error`` (float64 [4]), the per-frame arrays ``sigGs_f``,
    ``sigTL_f``, ``sigR_f``, ``m_f``, ``v_res``, ``v_row``, ``quantiles`` [N,nq], ``rowoff`` [N,H,2] and the curve ``lam_grid`` / ``lam_corr``."""
    from scipy import stats
    chunks = [frames] if torch.is_tensor(frames) else list(frames)
    if not chunks:
        raise PnnpError('fit_dark: no frames')
    first = _check_frames(chunks[0], None, None, 'fit_dark')
    H, W = first.shape[1:]
    chunks = [_check_frames(c, H, W, 'fit_dark') for c in chunks]
    if int(nq) != nq or nq < 2:
        raise PnnpError(f'fit_dark: nq must be an integer of at least 2, got {nq}')
    lam_grid = np.linspace(-0.3, 0.3, 121) if lam_grid is None else np.asarray(lam_grid, np.float64).reshape(-1)
    if lam_grid.size < 1:
        raise PnnpError('fit_dark: an empty lam_grid')
    if darkshading is not None and (not torch.is_tensor(darkshading) or darkshading.dtype != torch.float32 or tuple(darkshading.shape) != (H, W)):
        raise PnnpError(f'fit_dark: darkshading must be a float32 tensor [{H},{W}]')

    stack = DarkStack(H, W)
    for c in chunks:
        stack.add(c)
    N = stack.n
    if darkshading is None:
        if N < 2:
            raise PnnpError('fit_dark: a dark shading taken from the stack itself needs at least 2 frames')
        ds, corr_c = stack.dark_shading(), N / (N - 1)
        base = stack.plane_sums().astype(np.float64) / (N * (W // 2))
    else:
        _lib.require_cuda(darkshading)
        ds, corr_c = darkshading.contiguous(), 1.0
        base = ds.cpu().numpy().astype(np.float64).reshape(H, W // 2, 2).sum(axis=1) / (W // 2)
    rowoff = stack.rowsum.cpu().numpy().astype(np.float64) / (W // 2) - base[None]          # [N,H,2]
    rowoff32 = torch.from_numpy(rowoff.astype(np.float32)).to(ds.device)
    v_row = rowoff.reshape(N, -1).var(axis=1, ddof=1)
    m_f = rowoff.reshape(N, -1).mean(axis=1)

    p32 = probabilities(int(nq))
    p_dev = torch.from_numpy(p32).to(ds.device)
    v_res, lo, hi, f0 = [], [], [], 0
    for c in chunks:
        n = c.shape[0]
        res = residuals(c, ds, rowoff32[f0:f0 + n]).reshape(n, -1)
        for f in range(n):
            r = res[f].to(torch.float64)
            v_res.append((r * r).mean() - r.mean() ** 2)
        _, arg, w = losses.quantile_with_state(res, p_dev)                                 # arg [2,n,nq]: where s[lo] and s[hi] lie in the row
        lo.append(torch.gather(res, 1, arg[0].long()))
        hi.append(torch.gather(res, 1, arg[1].long()))
        f0 += n
        del res
    v_res = torch.stack(v_res).cpu().numpy()
    q = torch.lerp(torch.cat(lo).cpu(), torch.cat(hi).cpu(), w.cpu()[None]).numpy().astype(np.float64)      # [N,nq]

    p = p32.astype(np.float64)
    lam_corr = np.array([corr(stats.tukeylambda.ppf(p, lam), q).mean() for lam in lam_grid])
    lam = float(lam_grid[int(np.argmax(lam_corr))])
    sigGs_f = np.sqrt(corr_c) * slope(stats.norm.ppf(p), q)
    sigTL_f = np.sqrt(corr_c) * slope(stats.tukeylambda.ppf(p, lam), q)
    sigR_f = np.sqrt(np.maximum(corr_c * v_row - corr_c * v_res / (W // 2), 0.0))
    return {'Kmax': K, 'lam': lam, 'sigGs': float(sigGs_f.mean()), 'sigGssig': _spread(sigGs_f), 'sigTL': float(sigTL_f.mean()),
            'sigTLsig': _spread(sigTL_f), 'sigR': float(sigR_f.mean()), 'sigRsig': _spread(sigR_f), 'bias': 0, 'biassig': _spread(m_f),
            'q': 1.0 / (wp + 1), 'wp': wp, 'bl': bl,
            'iso': iso, 'n_frames': N, 'darkshading': ds, 'black_level_error': stack.black_level_error(bl),
            'sigGs_f': sigGs_f, 'sigTL_f': sigTL_f, 'sigR_f': sigR_f, 'm_f': m_f, 'v_res': v_res, 'v_row': v_row, 'quantiles': q,
            'rowoff': rowoff, 'lam_grid': lam_grid, 'lam_corr': lam_corr}


def fit_regression(per_iso):
    """A row of the regression table from at least 2 calibrated ISOs (``per_iso``: {iso: row of fit_dark}).  For X in TL, R, Gs the least
    squares line of log sigX on log K gives ``sigXk`` (slope), ``sigXb`` (intercept) and ``sigXsig``, the residuals' standard deviation
    sqrt(sum r^2 / max(n - 2, 1)).  ``Kmin`` / ``Kmax`` are the smallest and largest log K (the table stores log K in both), ``lam`` the
    mean; ``q``, ``wp``, ``bl`` are the rows' (they must agree)."""
    rows = list(per_iso.values())
    if len(rows) < 2:
        raise PnnpError(f'fit_regression: a line needs at least 2 ISOs, got {len(rows)}')
    for k in ('q', 'wp', 'bl'):
        if len({float(r[k]) for r in rows}) != 1:
            raise PnnpError(f'fit_regression: the ISOs disagree on {k}')
    K = np.array([float(r['Kmax']) for r in rows], np.float64)
    if not (K > 0).all() or len(set(K.tolist())) < 2:
        raise PnnpError('fit_regression: the gains must be positive and not all equal')
    x = np.log(K)
    x0 = x - x.mean()
    out = {'Kmin': float(x.min()), 'Kmax': float(x.max()), 'lam': float(np.mean([float(r['lam']) for r in rows])),
           'q': rows[0]['q'], 'wp': rows[0]['wp'], 'bl': rows[0]['bl']}
    for X in ('TL', 'R', 'Gs'):
        s = np.array([float(r['sig' + X]) for r in rows], np.float64)
        if not (s > 0).all():
            raise PnnpError(f'fit_regression: sig{X} must be positive at every ISO (its logarithm is fitted), got {s.tolist()}')
        y = np.log(s)
        k = float((x0 * (y - y.mean())).sum() / (x0 * x0).sum())
        b = float(y.mean() - k * x.mean())
        r = y - (k * x + b)
        out.update({f'sig{X}k': k, f'sig{X}b': b, f'sig{X}sig': float(np.sqrt((r * r).sum() / max(len(rows) - 2, 1)))})
    return out


# ---------------------------------------------------------------------------- row_denoise
def bilateral_1d(m, iso):
    """The 1-D bilateral filter that include/pnnp_hip.h defines (the stand-in for cv2.bilateralFilter on a 1 x n row): window 25, border
    REPLICATE, sigmaColor 10, sigmaSpace 1 + iso / 200, float64 on the host, the terms added in the order k = -12 .. 12."""
    m = np.asarray(m, np.float64)
    n, r = m.size, BILATERAL_D // 2
    ss = 1.0 + iso / 200.0
    num, den = np.zeros(n), np.zeros(n)
    for k in range(-r, r + 1):
        v = m[np.clip(np.arange(n) + k, 0, n - 1)]
        w = np.exp(-(k * k) / (2.0 * ss * ss)) * np.exp(-((v - m) ** 2) / (2.0 * BILATERAL_SC * BILATERAL_SC))
        num += w * v
        den += w
    return num / den


def row_denoise(data, iso):
    """utils/isp_algos.py:84-99 on a map that is already loaded (the reference runs it over its dark-shading files): ``bayer2rows``, the mean
    of every row of the two row planes (float64 sums: csrc/calib.hip), the 1-D bilateral filter of each plane's means, every row minus
    (mean - filtered), ``rows2bayer``.  float32 [H,W] in (a tensor, or numpy -> numpy out), float64 out as in the reference.  This is
    the per-sensor-row view: a row's mean runs over both column parities."""
    x, host = isp_ops._to_dev(data)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise PnnpError(f'row_denoise: expected a float32 map [H,W], got {x.dtype} {tuple(x.shape)}')
    H, W = x.shape
    if H < 2 or W < 1 or H % 2:
        raise PnnpError(f'row_denoise: the map needs an even number of rows, got {H}x{W}')
    rows = isp_ops.bayer2rows(x)                                                         # [2,H/2,W]
    means = torch.empty(H, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_entry('pnnp_calib_rowmean_f32')(_lib.ptr(rows), H, W, _lib.ptr(means), _lib.stream()), 'calib_rowmean')
    m = means.cpu().numpy().reshape(2, H // 2)
    diff = np.stack([m[i] - bilateral_1d(m[i], iso) for i in range(2)])
    out = rows.to(torch.float64) - torch.from_numpy(diff).to(x.device)[:, :, None]
    out = isp_ops.rows2bayer(out)
    return out.cpu().numpy() if host else out
