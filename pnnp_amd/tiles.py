"""A frame as overlapping tiles and back, under the reference's names (SynBase_Dataset.eval_crop / eval_merge,
data_process/syn_datasets.py:109-159), executed by the two gather kernels of csrc/tiles.hip.

The reference reflect-pads the frame by ``d = base // 2``, cuts ``nh x nw`` tiles of ``patch_size`` at stride
``l = patch_size - base`` (the last tile row / column snapped to the end of the padded frame), runs the network per tile and writes
every tile's ``l x l`` interior back: body tiles first, then the edge strips, then the corner, so later writes win.  ``TileGrid`` holds
both rules in closed form; the kernels evaluate them per element, so neither the padded frame nor (on the engines' path) an NCHW tile
batch is ever materialised, and every frame pixel is written exactly once by the tile that owns it.
"""
import numpy as np
import torch

from . import ops
from ._lib import PnnpError


class TileGrid:
    """The tile geometry of an ``h x w`` frame: ``d = base // 2``, ``l = patch_size - base``, ``nh = h // l + 1``, ``nw = w // l + 1``,
    ``T = nh * nw`` tiles in the order ``i * nw + j``.

    Crop: tile row ``i``, local row ``r`` reads padded row ``i * l + r`` (``h - l + r`` for the last tile row); padded coordinate ``p``
    is frame row ``reflect(p - d)`` (index -k -> k, h-1+k -> h-1-k).  Merge: frame row ``y`` belongs to the last tile row when
    ``y >= h - l`` (local row ``d + y - (h - l)``), else to tile row ``y // l`` (local row ``d + y % l``).  Columns alike.

    Refused with PnnpError: ``base`` odd, ``<= 0`` or ``>= patch_size``; ``h < l`` or ``w < l`` (the reference dies there with a shape
    error); ``d >= h`` or ``d >= w`` (the reflection is undefined); with ``network=True`` also ``patch_size % 16 != 0``."""

    def __init__(self, h, w, patch_size, base=64, network=False):
        h, w, P, base = int(h), int(w), int(patch_size), int(base)
        if base <= 0 or base % 2 or base >= P:
            raise PnnpError(f'tiles: base must be even, positive and below patch_size, got base {base}, patch_size {P}')
        if network and P % 16:
            raise PnnpError(f'tiles: the networks need patch_size % 16 == 0, got {P}')
        d, l = base // 2, P - base
        if h < l or w < l:
            raise PnnpError(f'tiles: frame {h} x {w} is smaller than a tile interior (patch_size - base = {l})')
        if d >= h or d >= w:
            raise PnnpError(f'tiles: border base // 2 = {d} does not fit the reflection of a {h} x {w} frame')
        self.h, self.w, self.patch_size, self.base, self.d, self.l = h, w, P, base, d, l
        self.nh, self.nw = h // l + 1, w // l + 1
        self.T = self.nh * self.nw

    def key(self):
        return self.h, self.w, self.patch_size, self.base

    def chunks(self, tile_batch=None):
        """[(t0, nt)]: range(T) in runs of at most ``tile_batch`` tiles (None: one run)"""
        tb = self.T if tile_batch is None else int(tile_batch)
        if tb < 1:
            raise PnnpError(f'tiles: tile_batch must be positive, got {tile_batch}')
        return [(t0, min(tb, self.T - t0)) for t0 in range(0, self.T, tb)]

    # ---- the two rules per axis (numpy; the kernels compute the same per element)
    def _src(self, n, size):
        """[n_tiles, P]: the frame index every (tile, local) position of one axis reads"""
        P, l, d = self.patch_size, self.l, self.d
        start = np.where(np.arange(n) < n - 1, np.arange(n) * l, size - l)
        q = start[:, None] + np.arange(P)[None, :] - d
        q = np.where(q < 0, -q, q)
        return np.where(q >= size, 2 * size - 2 - q, q)

    def _owner(self, n, size):
        """([size] owner tile, [size] local position in it) of every frame index of one axis"""
        l, d = self.l, self.d
        y = np.arange(size)
        last = y >= size - l
        return np.where(last, n - 1, y // l), np.where(last, d + y - (size - l), d + y % l)

    def crop_index(self):
        """int64 [T, P, P]: the flat index ``y * w + x`` of the frame pixel every tile pixel reads"""
        ys, xs = self._src(self.nh, self.h), self._src(self.nw, self.w)
        idx = ys[:, None, :, None] * self.w + xs[None, :, None, :]
        return idx.reshape(self.T, self.patch_size, self.patch_size)

    def merge_index(self):
        """int64 [h, w]: the flat index ``(t * P + r) * P + c`` of the tile pixel every frame pixel takes"""
        P = self.patch_size
        (ti, r), (tj, c) = self._owner(self.nh, self.h), self._owner(self.nw, self.w)
        return ((ti[:, None] * self.nw + tj[None, :]) * P + r[:, None]) * P + c[None, :]

    def owned(self, t0, nt):
        """bool [h, w]: the frame pixels whose owner is one of the tiles t0 .. t0 + nt"""
        t = self.merge_index() // (self.patch_size * self.patch_size)
        return (t >= t0) & (t < t0 + nt)


def _frame(data, what):
    if not torch.is_tensor(data) or not data.is_cuda:
        raise PnnpError(f'{what} needs a CUDA tensor (pnnp_amd has no CPU path)')
    if data.dim() != 4 or data.shape[0] != 1:
        raise PnnpError(f'{what} expects one frame [1,C,h,w], got {tuple(data.shape)}')
    return data.contiguous().float()


def eval_crop(data, patch_size, base=64):
    """syn_datasets.py:109-134: CUDA float32 [1,C,h,w] -> [T,C,P,P], one launch, no padded copy."""
    x = _frame(data, 'eval_crop')
    grid = TileGrid(x.shape[2], x.shape[3], patch_size, base)
    out = torch.empty((grid.T, x.shape[1], grid.patch_size, grid.patch_size), dtype=torch.float32, device=x.device)
    ops.tile_crop(x, grid, 0, grid.T, nchw=out)
    return out


def eval_merge(croped_data, h, w, base=64, ratio=None, clamp=False):
    """syn_datasets.py:136-159: CUDA float32 [T,C,P,P] -> [1,C,h,w].  ``ratio`` (a float or a CUDA scalar tensor) and ``clamp`` fuse
    ``(frame * ratio).clamp(0, 1)`` into the store (a NaN stays a NaN, as in torch.clamp)."""
    if not torch.is_tensor(croped_data) or not croped_data.is_cuda:
        raise PnnpError('eval_merge needs a CUDA tensor (pnnp_amd has no CPU path)')
    if croped_data.dim() != 4 or croped_data.shape[2] != croped_data.shape[3]:
        raise PnnpError(f'eval_merge expects square tiles [T,C,P,P], got {tuple(croped_data.shape)}')
    t = croped_data.contiguous().float()
    grid = TileGrid(h, w, t.shape[2], base)
    if t.shape[0] != grid.T:
        raise PnnpError(f'eval_merge: a {h} x {w} frame has {grid.nh} x {grid.nw} = {grid.T} tiles of {grid.patch_size}, got {t.shape[0]}')
    out = torch.empty((1, t.shape[1], grid.h, grid.w), dtype=torch.float32, device=t.device)
    ops.tile_merge(t, out, grid, 0, grid.T, ratio=ratio, clamp=clamp)
    return out
