"""numpy restatement of the noise-model score the kernels of csrc/noise_score.hip implement: integer key counts + the key -> bin table +
the reference's rules (utils/kld_div.py:163-200, trainer_NF_SID.py:165-172).  tests/test_host_kld.py pins it to the reference's own outputs
(tests/golden/kld.npz); tests/test_gpu_kld.py compares the device with it."""
import numpy as np


def counts_and_kl(p, q, lut, nbins, bl=512, wp=16383):
    """(counts_p, counts_q, flags, (kl_fwd, kl_inv, kl_sym), abs_terms) of flat float32 DN arrays; the inputs are not modified."""
    p = np.asarray(p, np.float32).reshape(-1); q = np.asarray(q, np.float32).reshape(-1)
    n = p.size
    has_nan, has_neg = bool(np.isnan(p).any()), bool((p < 0).any())
    shift = has_neg and not has_nan                          # min(p) < 0 under numpy's NaN-propagating min
    out = []
    for x in (p, q):
        with np.errstate(invalid='ignore'):
            v = x + np.float32(bl) if shift else x
            v = np.clip(np.rint(v), np.float32(0), np.float32(wp))
        ok = ~np.isnan(v)
        raw = np.bincount(v[ok].astype(np.int64), minlength=wp + 1)
        c = np.zeros(nbins, np.int64)
        m = lut >= 0
        np.add.at(c, lut[m], raw[m])
        out.append(c)
    cp, cq = out
    yp, yq = cp / n, cq / n
    idx = (cp > 0) & (cq > 0)
    a, b = yp[idx], yq[idx]
    tf, ti = a * (np.log(a) - np.log(b)), b * (np.log(b) - np.log(a))
    fwd, inv = float(np.sum(tf)), float(np.sum(ti))
    return cp, cq, (1 if has_neg else 0) | (2 if has_nan else 0), (fwd, inv, (fwd + inv) / 2.0), (float(np.abs(tf).sum()), float(np.abs(ti).sum()))


def pair_dn(clean, real, sampled_noise, bl, wp):
    """trainer_NF_SID.py:166-170 on float32 numpy arrays of one crop: (p, q, output)."""
    inputs = np.asarray(clean, np.float32).clip(0, 1)
    output = np.asarray(sampled_noise, np.float32) + inputs
    target = np.asarray(real, np.float32)
    s = np.float32(wp - bl)
    with np.errstate(invalid='ignore'):
        p = np.round((target - inputs).flatten() * s)
        q = np.round((output - inputs).flatten() * s)
    return p, q, output
