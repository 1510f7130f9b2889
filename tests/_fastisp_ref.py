"""The numpy restatement of the full-resolution render (csrc/demosaic.hip): the reference's FastISP (utils/isp_ops.py:134-158) with the
edge-aware demosaic that include/pnnp_hip.h defines in place of cv2.cvtColor(COLOR_BAYER_BG2RGB_EA).  tests/test_host_fastisp.py pins it
to the real function's outputs (tests/golden/fastisp.npz, recorded with this demosaic in the stubbed cv2) and to hand-written values.

    front    float32: S = (R wb0 | G1 / G2 | B wb2) interleaved RGGB; clip [0,1]; * 16383; truncate to uint16; a NaN gives 0
    demosaic integer, on the uint16 mosaic (``demosaic_ea``)
    tail     float64: D / 16383; np.sum(img * ccm, axis=-1); clip [0,1]; ** (1 / 2.2)

All return numpy arrays."""
import numpy as np

SONY_CCM64 = np.array([[1.9712269, -0.6789218, -0.29230508],                    # utils/isp_ops.py:151-153, the float64 default
                       [-0.29104823, 1.748401, -0.45735288],
                       [0.02051281, -0.5380369, 1.5175241]])


def demosaic_ea(mosaic):
    """uint16 [H,W] or [B,H,W] (RGGB, H and W even, >= 4) -> uint16 [..,H,W,3] in R, G, B order"""
    S = np.asarray(mosaic)
    assert S.dtype == np.uint16 and S.ndim in (2, 3)
    if S.ndim == 3:
        return np.stack([demosaic_ea(s) for s in S])
    H, W = S.shape
    assert H >= 4 and W >= 4 and H % 2 == 0 and W % 2 == 0
    s = S.astype(np.int64)
    c = s[1:-1, 1:-1]
    u, d, l, r = s[:-2, 1:-1], s[2:, 1:-1], s[1:-1, :-2], s[1:-1, 2:]
    hz, vt = (l + r + 1) >> 1, (u + d + 1) >> 1
    diag = (s[:-2, :-2] + s[:-2, 2:] + s[2:, :-2] + s[2:, 2:] + 2) >> 2
    g_at_colour = np.where(np.abs(l - r) > np.abs(u - d), vt, hz)                # a tie takes the horizontal pair
    yy, xx = np.mgrid[1:H - 1, 1:W - 1]
    even_row, colour = (yy & 1) == 0, ((yy ^ xx) & 1) == 0                        # colour: an R site (even, even) or a B site (odd, odd)
    R = np.where(colour, np.where(even_row, c, diag), np.where(even_row, hz, vt))
    G = np.where(colour, g_at_colour, c)
    B = np.where(colour, np.where(even_row, diag, c), np.where(even_row, vt, hz))
    inner = np.stack([R, G, B], axis=-1)
    iy = np.clip(np.arange(H), 1, H - 2) - 1
    ix = np.clip(np.arange(W), 1, W - 2) - 1
    return inner[iy][:, ix].astype(np.uint16)                                    # border: the nearest interior pixel's RGB


def front(x, wb=None):
    """float32 [4,h,w] planes R, G1, B, G2; wb None (gains 2) or an array whose entries 0 and 2 are taken as float32 -> uint16 [2h,2w]"""
    x = np.asarray(x, np.float32)
    _, h, w = x.shape
    g0 = np.float32(2 if wb is None else np.asarray(wb, np.float32).reshape(-1)[0])
    g2 = np.float32(2 if wb is None else np.asarray(wb, np.float32).reshape(-1)[2])
    raw = np.zeros((2 * h, 2 * w), np.float32)
    raw[0::2, 0::2] = x[0] * g0
    raw[0::2, 1::2] = x[1]
    raw[1::2, 1::2] = x[2] * g2
    raw[1::2, 0::2] = x[3]
    raw = np.clip(raw, 0, 1) * np.float32(16383)
    return np.where(np.isnan(raw), np.float32(0), raw).astype(np.uint16)


def tail(D, ccm=None):
    """uint16 [H,W,3] -> float64 [H,W,3]; ccm None (the float64 default) or [3,3], taken as given (a float32 matrix is widened)"""
    img = np.asarray(D) / 16383
    ccm = SONY_CCM64 if ccm is None else np.asarray(ccm)
    img = np.sum(img[:, :, None, :] * ccm[None, None, :, :], axis=-1)
    return np.clip(img, 0, 1) ** (1 / 2.2)


def fastisp(x, wb=None, ccm=None):
    """-> float64 [2h,2w,3], the real FastISP's result when its cv2.cvtColor is ``demosaic_ea``"""
    return tail(demosaic_ea(front(x, wb)), ccm)


def levels(out64):
    """floor(255 v) as uint8"""
    return np.floor(255 * np.asarray(out64, np.float64)).astype(np.uint8)
