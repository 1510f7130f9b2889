#!/usr/bin/env python3
"""Generate tests/golden/tiles.npz + tiles.json by running the REAL reference: SynBase_Dataset.eval_crop / eval_merge
(data_process/syn_datasets.py:109-159), the overlapping-tile split of a frame and its inverse.

Runs only where the reference is available (see make_golden.py, whose import stubs it uses); stores data only.

    python tests/golden/make_golden_tiles.py

Both functions are called UNBOUND on a stand-in ``self`` (args = {'patch_size': P}, h, w, c), as make_golden_mix.py calls ``preprocess``.
Both are pure gathers, so the fixtures are INDEX MAPS, not images:

    <tag>_crop   int32 [T, c, P, P]   eval_crop of the frame that holds arange(c*h*w): which frame element every tile element reads
    <tag>_merge  int32 [1, c, h, w]   eval_merge of the tile batch that holds arange(T*c*P*P): which tile element every frame element takes

Per case the generator asserts merge(crop(x)) == x before it writes anything; the case the reference cannot run (h < patch_size - base)
is recorded in the json with the exception it raised.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

# (h, w, P, base, c): see the table in DESIGN.md section 7b, row f12
CASES = [
    (80, 150, 48, 16, 4),      # general: 3 x 5 tiles, body, both strips and the corner
    (64, 96, 48, 16, 4),       # h and w exact multiples of l: the last row / column duplicates a body tile, the winner matters
    (32, 32, 48, 16, 4),       # h == l, the smallest legal frame: 2 x 2 tiles, all snapped to the end
    (33, 47, 48, 16, 4),       # odd sizes, one pixel past l
    (40, 200, 64, 32, 4),      # another base, 2 x 7 grid
    (33, 47, 48, 16, 8),       # nframes = 2: 8 channels
    (31, 40, 48, 16, 4),       # h < l: the reference raises
]


def main():
    import_reference()
    import torch
    ds = sys.modules['data_process.syn_datasets'].SynBase_Dataset
    out, meta = {}, []
    for h, w, P, base, c in CASES:
        tag = f'h{h}w{w}p{P}b{base}c{c}'
        me = types.SimpleNamespace(args={'patch_size': P}, h=h, w=w, c=c)
        frame = torch.arange(c * h * w, dtype=torch.float64).view(1, c, h, w)
        l = P - base
        nh, nw = h // l + 1, w // l + 1
        try:
            crop = ds.eval_crop(me, frame, base=base)
        except Exception as e:                                    # noqa: BLE001  (whatever the reference dies with is the record)
            meta.append(dict(tag=tag, h=h, w=w, P=P, base=base, c=c, raises=True, error=type(e).__name__))
            continue
        T = nh * nw
        assert tuple(crop.shape) == (T, c, P, P)
        tiles = torch.arange(T * c * P * P, dtype=torch.float64).view(T, c, P, P)
        merge = ds.eval_merge(me, tiles, base=base)
        assert tuple(merge.shape) == (1, c, h, w)
        assert torch.equal(ds.eval_merge(me, crop, base=base), frame), tag        # the split is lossless
        out[tag + '_crop'] = crop.numpy().astype(np.int32)
        out[tag + '_merge'] = merge.numpy().astype(np.int32)
        meta.append(dict(tag=tag, h=h, w=w, P=P, base=base, c=c, raises=False, nh=nh, nw=nw))
    assert sum(m['raises'] for m in meta) == 1 and meta[-1]['raises']
    np.savez_compressed(os.path.join(HERE, 'tiles.npz'), **out)
    json.dump(dict(cases=meta), open(os.path.join(HERE, 'tiles.json'), 'w'), indent=1)
    print('tile fixtures written:', os.path.getsize(os.path.join(HERE, 'tiles.npz')), 'bytes')


if __name__ == '__main__':
    main()
