"""numpy restatement of what the kernels of csrc/hist_kl.hip do: the bin of every sample by guess-and-correct (with the arange hint) or by
the branch-free binary search (without), counts, then y = counts / n and the KLs in the kernel's summation order.  tests/test_host_kl_data.py
pins it to the reference's own outputs (tests/golden/kl_data.npz) and to np.histogram; tests/test_gpu_kl_data.py compares the device with it."""
import numpy as np

THREADS, WAVES = 1024, 16


def default_edges(left_edge=0.0, right_edge=1.0, n_bins=1000):
    bw = (right_edge - left_edge) / n_bins
    return np.arange(left_edge, right_edge + bw, bw)


def hint_of(e):
    """What the host passes for edges that came from arange: (e0, nb / (e[nb] - e0))."""
    return float(e[0]), float((len(e) - 1) / (e[-1] - e[0]))


def bins_of(x, e, hint=None):
    """int64 bin of every sample (-1: in no bin), as the count kernel finds it."""
    v = np.asarray(x).reshape(-1).astype(np.float64)            # exact for float32
    e = np.asarray(e, np.float64)
    nb = len(e) - 1
    with np.errstate(invalid='ignore'):
        ok = (v >= e[0]) & (v <= e[nb])                         # a NaN fails both
    w = v[ok]
    if hint is not None and hint[1] > 0:
        with np.errstate(over='ignore', invalid='ignore'):
            t = (w - hint[0]) * hint[1]
        g = np.where(~(t < nb - 1), nb - 1, np.where(t < nb - 1, t, 0).astype(np.int64))
        while True:                                             # down while e[g] > x
            m = (g > 0) & (e[g] > w)
            if not m.any():
                break
            g[m] -= 1
        while True:                                             # up while e[g + 1] <= x
            m = (g < nb - 1) & (e[np.minimum(g + 1, nb - 1)] <= w)
            if not m.any():
                break
            g[m] += 1
    else:
        top = 1
        while 2 * top <= nb - 1:
            top *= 2
        g = np.zeros(w.shape, np.int64)
        s = top
        while s > 0:
            c = g + s
            m = (c < nb) & (e[np.minimum(c, nb - 1)] <= w)
            g[m] = c[m]
            s >>= 1
    out = np.full(v.shape, -1, np.int64)
    out[ok] = g
    return out


def counts_of(x, e, hint=None):
    b = bins_of(x, e, hint)
    return np.bincount(b[b >= 0], minlength=len(e) - 1).astype(np.int64)


def _kernel_sum(terms):
    """The finishing workgroup's order: thread t adds bins t, t + 1024, ...; a wave's 64 partial sums meet in an xor butterfly (32 .. 1);
    thread 0 adds the 16 waves in order."""
    nb = len(terms)
    part = np.zeros(THREADS, np.float64)
    for i0 in range(0, nb, THREADS):
        chunk = terms[i0:i0 + THREADS]
        part[:len(chunk)] += chunk
    a = part.reshape(WAVES, 64)
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lane ^ s]
    total = a[0, 0]
    for w in range(1, WAVES):
        total = total + a[w, 0]
    return float(total)


def kl_of(cp, cq, n_p, n_q):
    """((fwd, inv, sym), (sum |fwd terms|, sum |inv terms|)) of two count vectors."""
    yp, yq = cp / float(n_p), cq / float(n_q)
    both = (cp > 0) & (cq > 0)
    lp, lq = np.log(np.where(both, yp, 1.0)), np.log(np.where(both, yq, 1.0))
    tf, ti = np.where(both, yp * (lp - lq), 0.0), np.where(both, yq * (lq - lp), 0.0)
    fwd, inv = _kernel_sum(tf), _kernel_sum(ti)
    return (fwd, inv, (fwd + inv) / 2.0), (float(np.abs(tf).sum()), float(np.abs(ti).sum()))


def counts_and_kl(p, q, e, hint=None):
    """(counts_p, counts_q, (kl_fwd, kl_inv, kl_sym), abs_terms); the inputs are not modified."""
    cp, cq = counts_of(p, e, hint), counts_of(q, e, hint)
    kl, ab = kl_of(cp, cq, np.asarray(p).size, np.asarray(q).size)
    return cp, cq, kl, ab


def range_edges(p, q, wp):
    """utils/kld_div.py:165-169, :181-183 with bl=None: the scalars stay in the data's dtype."""
    p, q = np.asarray(p), np.asarray(q)
    left_edge, right_edge = min(p.min(), q.min()), max(p.max(), q.max())
    data_range = right_edge - left_edge
    bin_width = data_range / wp
    return np.arange(left_edge, right_edge + bin_width, bin_width)


def load_case(g, name):
    """(p, q, edges, arange-made?) of a histogram case of kl_data.npz."""
    pn, qn = (str(s) for s in g[name + '_pq'])
    given = name + '_e' in g.files
    return g['data_' + pn], g['data_' + qn], (g[name + '_e'] if given else default_edges()), not given


def load_range_case(g, name):
    pn, qn = (str(s) for s in g[name + '_pq'])
    return g['data_' + pn], g['data_' + qn], int(g[name + '_wp'])


CASES = ['default', 'nf', 'edge32', 'edge64', 'special', 'allout', 'halfout', 'repeat', 'onebin', 'twobin', 'unequal', 'default64']
RANGE_CASES = ['range16383', 'range1000', 'range255', 'range1000s', 'range255n', 'range1000w', 'range255w', 'range64', 'range64s']
EDGE_VALUE_CASES = ['edge32', 'edge64', 'special', 'repeat']
