"""The output descriptor of tnh_gemm_gather_scatter as Python builds it (hip_backend._scatter_descriptor): element
(tile, box row r, small row c) of the product lands where NumPy's transpose puts it.  No GPU, no library call."""
import numpy as np
import pytest

from tensornetwork_amd import hip_backend


def _mixed_radix(n, exts, steps):
  """offsets of 0 ... n-1 written in the mixed radix `exts` (innermost first) with `steps` elements per index"""
  rem, off = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
  for ext, step in zip(exts, steps):
    off += (rem % ext) * step
    rem //= ext
  return off


# (long shape, contracted axes, small operand's free shape, destination as a permutation of [long's free axes...,
#  small's free axes...], BN, contiguous run of the destination in elements)
@pytest.mark.parametrize("shape,k_axes,small,dest,want_bn,want_run", [
    ((16, 12, 16, 12, 16), [1, 3], (6, 12), (0, 3, 1, 2, 4), 64, 12),       # interleaved, innermost: a small axis
    ((12, 16, 12, 16, 12), [0, 3], (6, 12), (3, 0, 1, 4, 2), 48, 12),       # innermost: the box's innermost free digit
    ((16, 12, 16, 16, 12), [1, 4], (12, 12), (3, 0, 4, 1, 2), 64, 64),      # innermost digit contracted, axes 2, 3 one digit
])
def test_scatter_descriptor_lands_where_numpy_transposes(shape, k_axes, small, dest, want_bn, want_run):
  free = [i for i in range(len(shape)) if i not in k_axes]
  natural = tuple(shape[i] for i in free) + tuple(small)
  strides = hip_backend._row_major_strides(tuple(natural[p] for p in dest))      # pylint: disable=protected-access
  stride_of = {p: st for p, st in zip(dest, strides)}                            # natural result axis -> destination stride
  out_strides = [0] * len(shape)
  for j, ax in enumerate(free):
    out_strides[ax] = stride_of[j]
  small_pos = sorted(range(len(free), len(natural)), key=dest.index)             # small axes in destination order
  got = hip_backend._scatter_descriptor(shape, k_axes, out_strides, [natural[p] for p in small_pos],      # pylint: disable=protected-access
                                        [stride_of[p] for p in small_pos])
  desc, out, bn, run = got
  assert (bn, run) == (want_bn, want_run)
  nl, ms = int(np.prod([shape[i] for i in free])), int(np.prod(small))
  assert out.c_elems == nl * ms
  box = [d for d in range(desc.nd) if not (desc.k_mask >> d) & 1]
  row_off = _mixed_radix(bn, [desc.ext[d] for d in box], [out.omult[d] for d in box])
  col_off = _mixed_radix(ms, list(out.sext)[:out.ns], list(out.sstride)[:out.ns])
  tile_off = _mixed_radix(nl // bn, list(desc.text)[:desc.nt], list(out.otstride)[:desc.nt])
  offsets = ((tile_off[:, None] + row_off[None, :]).reshape(nl)[:, None] + col_off[None, :])
  # row n of the product = the n-th free tuple of the long tensor (natural order); column c = row c of the small
  # operand, whose free axes are in destination order
  x = np.arange(nl * ms, dtype=np.int64).reshape(natural)
  rows_cols = np.transpose(x, list(range(len(free))) + small_pos).reshape(nl, ms)
  landed = np.empty(nl * ms, np.int64)
  landed[offsets.ravel()] = rows_cols.ravel()
  np.testing.assert_array_equal(landed.reshape([natural[p] for p in dest]), np.transpose(x, dest))


def test_scatter_descriptor_refuses_a_split_merged_digit():
  """axes 2 and 3 of the long tensor are one digit of the gather plan: a destination that pulls them apart has no
  descriptor (the caller's fallback runs)"""
  shape, k_axes = (16, 12, 16, 16, 12), [1, 4]
  # destination [axis 2, small 0, axis 3, axis 0, small 1]
  strides = hip_backend._row_major_strides((16, 12, 16, 16, 12))      # pylint: disable=protected-access
  out_strides = [strides[3], 0, strides[0], strides[2], 0]
  assert hip_backend._scatter_descriptor(shape, k_axes, out_strides, [12, 12], [strides[1], strides[4]]) is None      # pylint: disable=protected-access
