"""Golden arrays as several small archives, ``<stem>.part00.npz``, ``<stem>.part01.npz``, ...: no committed file may
exceed 1 MiB, and the three large fixture sets hold 1.5 - 3 MB of (compressed) arrays.  The generators write with
``save``, ``tests/conftest.py`` reads with ``load``; a name lives in exactly one part."""
import glob
import io
import os
import zipfile

import numpy as np

PART_LIMIT = 900_000      # bytes of compressed members per part (the archive's own directory adds a few per cent)


def save(stem, arrays, limit=PART_LIMIT):
  """Write `arrays` (name -> array, kept in this order) as ``<stem>.partNN.npz`` and drop parts of an earlier run.
  Parts are cut by the members' compressed sizes, taken from one archive of everything made in memory."""
  for old in glob.glob(stem + ".part*.npz"):
    os.remove(old)
  whole = io.BytesIO()
  np.savez_compressed(whole, **arrays)
  sizes = {i.filename[:-len(".npy")]: i.compress_size + 2 * len(i.filename) + 128 for i in zipfile.ZipFile(whole).infolist()}
  groups, size = [{}], 0
  for name, arr in arrays.items():
    if groups[-1] and size + sizes[name] > limit:
      groups.append({})
      size = 0
    groups[-1][name] = arr
    size += sizes[name]
  paths = []
  for k, group in enumerate(groups):
    paths.append(f"{stem}.part{k:02d}.npz")
    np.savez_compressed(paths[-1], **group)
  return paths


def load(stem):
  """name -> array over every part of `stem`."""
  paths = sorted(glob.glob(stem + ".part*.npz"))
  if not paths:
    raise FileNotFoundError(stem + ".part*.npz")
  out = {}
  for path in paths:
    with np.load(path) as part:
      for name in part.files:
        assert name not in out, (name, path)
        out[name] = part[name]
  return out
