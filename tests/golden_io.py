"""Golden vectors spread over several .npz files, none larger than a committed file may be: arrays that are too
large for one file are cut along their first axis into pieces 'key#0', 'key#1', ... and put together again on load."""
import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PIECE = 400_000   # bytes of one piece of a cut array
LIMIT = 1_000_000  # uncompressed bytes of one file (compression only shrinks it): below 1 MiB


def save_split(stem, arrays):
    """write {key: ndarray} to golden/<stem>_NN.npz, replacing every earlier file of that stem"""
    for old in glob.glob(os.path.join(GOLD, stem + "_[0-9][0-9].npz")):
        os.remove(old)
    pieces = []
    for k, v in arrays.items():
        v = np.asarray(v)
        if v.nbytes <= PIECE or v.ndim == 0:
            pieces.append((k, v))
            continue
        rows = max(1, PIECE // (v.nbytes // v.shape[0]))
        for n, lo in enumerate(range(0, v.shape[0], rows)):
            pieces.append((f"{k}#{n}", v[lo:lo + rows]))
    files, cur, size = [], {}, 0
    for k, v in pieces:
        assert v.nbytes <= LIMIT, k
        if cur and size + v.nbytes > LIMIT:
            files.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    files.append(cur)
    for n, f in enumerate(files):
        np.savez_compressed(os.path.join(GOLD, "%s_%02d.npz" % (stem, n)), **f)
    return len(files)


def load_split(stem):
    flat = {}
    paths = sorted(glob.glob(os.path.join(GOLD, stem + "_[0-9][0-9].npz")))
    assert paths, stem
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                flat[k] = z[k]
    out, cut = {}, {}
    for k, v in flat.items():
        if "#" in k:
            base, n = k.split("#")
            cut.setdefault(base, {})[int(n)] = v
        else:
            out[k] = v
    for base, parts in cut.items():
        out[base] = np.concatenate([parts[n] for n in range(len(parts))], axis=0)
    return out
