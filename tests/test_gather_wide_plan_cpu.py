"""Boxes of up to 64 x 256 (the wide gather kernel's, tnh_gemm_gather_wide.hip): the chunk plan the kernel's own index
functions produce on the host (tnh_gemm_gather_plan, no device needed) covers the BN x K image exactly once and reads
the elements NumPy's strides name."""
import ctypes

import numpy as np
import pytest

from tensornetwork_amd import _lib, hip_backend


@pytest.mark.parametrize("shape,k_axes,want_bn", [
    ((16,) * 5, [1, 3], 64),                   # innermost axis free
    ((16,) * 5, [1, 4], 64),                   # innermost axis contracted
    ((12, 16, 12, 16, 12), [1, 3], 48),
])
def test_wide_box_plan_covers_the_image_once_at_numpy_offsets(shape, k_axes, want_bn):
  desc, bn, nl = hip_backend._gather_descriptor(shape, k_axes, max_box_k=256)      # pylint: disable=protected-access
  free = [i for i in range(len(shape)) if i not in k_axes]
  k = int(np.prod([shape[i] for i in k_axes]))
  assert (bn, k, desc.kl_ext) == (want_bn, 256, 1) and nl == int(np.prod([shape[i] for i in free]))
  nch, nt = bn * k // 4, nl // bn
  off, row, col = (np.zeros(nch, np.int32) for _ in range(3))
  base = np.zeros(nt, np.int64)
  p32, p64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
  rc = _lib.load_library().tnh_gemm_gather_plan(ctypes.byref(desc), k, nl, int(np.prod(shape)), off.ctypes.data_as(p32),
                                                row.ctypes.data_as(p32), col.ctypes.data_as(p32), nch,
                                                base.ctypes.data_as(p64), nt)
  assert rc == bn, (rc, _lib.last_error())
  # element offsets of the matrix [free tuples (natural order)][contracted tuples (memory order)], from NumPy's strides
  x = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
  want = np.transpose(x, free + sorted(k_axes)).reshape(nl, k)
  i = np.arange(4)[None, :]                    # a chunk's four elements: along k (innermost axis contracted) or the rows
  kin = bool(desc.k_mask & 1)
  rows, cols = (row[:, None] + 0 * i, col[:, None] + i) if kin else (row[:, None] + i, col[:, None] + 0 * i)
  hits = np.zeros((bn, k), np.int64)
  np.add.at(hits, (rows, cols), 1)
  assert hits.min() == 1 and hits.max() == 1
  for t in (0, 1, nt - 1):
    got = np.empty((bn, k), np.int64)
    got[rows, cols] = base[t] + off[:, None] + i
    np.testing.assert_array_equal(got, want[t * bn:(t + 1) * bn])
