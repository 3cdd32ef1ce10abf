"""Golden vector sets stored as several .npz parts so that no stored file exceeds PART_BYTES of array data: ``<stem>.npz``,
``<stem>.1.npz``, ``<stem>.2.npz``, ...  ``save`` packs the arrays first-fit by decreasing size; ``load`` merges the parts
back into one {key: array} dict, the same arrays a single ``np.load`` of the unsplit file returned."""
import os

import numpy as np

PART_BYTES = 960_000


def save(directory, stem, arrays):
    parts = []
    for k in sorted(arrays, key=lambda k: (-np.asarray(arrays[k]).nbytes, k)):
        n = np.asarray(arrays[k]).nbytes
        for p in parts:
            if p[0] + n <= PART_BYTES:
                p[0] += n
                p[1][k] = arrays[k]
                break
        else:
            parts.append([n, {k: arrays[k]}])
    for i, (_, part) in enumerate(parts):
        np.savez_compressed(os.path.join(directory, stem + (f".{i}" if i else "") + ".npz"), **part)


def load(directory, stem):
    out = dict(np.load(os.path.join(directory, stem + ".npz")))
    i = 1
    while os.path.exists(os.path.join(directory, f"{stem}.{i}.npz")):
        out.update(np.load(os.path.join(directory, f"{stem}.{i}.npz")))
        i += 1
    return out
