"""A fixture archive too large for one committed file, stored as a directory of numbered .npz shards
(00.npz, 01.npz, ...), each below SHARD_BYTES.  An array larger than a shard is split along its first axis
into pieces named "<name>#<i>", which load() joins again.  Arrays keep their order."""
import glob
import os

import numpy as np

SHARD_BYTES = 896 * 1024          # raw bytes per shard: compressed, with the archive's headers, well under 1 MiB
_ENTRY_BYTES = 512                # per array: .npy header and zip entry


def _pieces(name, a):
    if a.nbytes + _ENTRY_BYTES <= SHARD_BYTES:
        return [(name, a)]
    n = -(-a.nbytes // (SHARD_BYTES - _ENTRY_BYTES))
    assert a.ndim and a.shape[0] >= n, (name, a.shape)
    return [(f"{name}#{i}", p) for i, p in enumerate(np.array_split(a, n, axis=0))]


def save(path, arrays):
    """Write {name: array} to the directory `path` as shards, replacing any shards already there."""
    os.makedirs(path, exist_ok=True)
    for f in glob.glob(os.path.join(path, "*.npz")):
        os.remove(f)
    shards, cur, size = [], {}, 0
    for name, a in arrays.items():
        for key, p in _pieces(name, np.asarray(a)):
            if cur and size + p.nbytes + _ENTRY_BYTES > SHARD_BYTES:
                shards.append(cur)
                cur, size = {}, 0
            cur[key] = p
            size += p.nbytes + _ENTRY_BYTES
    if cur:
        shards.append(cur)
    for i, s in enumerate(shards):
        np.savez_compressed(os.path.join(path, f"{i:02d}.npz"), **s)
    return len(shards)


def load(path):
    """{name: array} of the shards under the directory `path`, in the order they were saved."""
    files = sorted(glob.glob(os.path.join(path, "*.npz")))
    if not files:
        raise FileNotFoundError(f"no shards under {path}")
    out, parts = {}, {}
    for f in files:
        with np.load(f) as z:
            for key in z.files:
                name, sep, _ = key.rpartition("#")
                if sep:
                    parts.setdefault(name, []).append(z[key])
                    out.setdefault(name, None)
                else:
                    out[key] = z[key]
    for name, ps in parts.items():
        out[name] = np.concatenate(ps, axis=0)
    return out
