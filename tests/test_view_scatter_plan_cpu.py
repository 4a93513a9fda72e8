"""The destination descriptor of tnh_gemm_view_scatter as Python builds it (hip_backend._cview_descriptor): which
operand becomes the kernel's N side, the merged digits, the run, and the addresses, enumerated, against np.transpose."""
import numpy as np
import pytest

from tensornetwork_amd import _lib, hip_backend

# (a's shape, a's contracted axes, b's shape, b's contracted axes, result_order, a read in place, b read in place,
#  expected: a is the N side, run, digits (extent, stride) of m and of n innermost first) -- None: no descriptor
_CASES = [
    # both in place, interleaved, b's last free axis innermost: nothing merges
    ((16, 16, 16, 128), [3], (12, 16, 16, 128), [3], (0, 3, 1, 4, 2, 5), True, True,
     (False, 16, [(16, 16), (16, 256 * 16), (16, 16 * 12 * 4096)], [(16, 1), (16, 256), (12, 65536)])),
    # a's last free axis innermost: roles swapped; b's axes 1, 2 stay adjacent in the destination and merge
    ((12, 12, 12, 64), [3], (5, 12, 12, 64), [3], (3, 0, 1, 4, 5, 2), True, True,
     (True, 12, [(144, 12), (5, 144 * 1728)], [(12, 1), (144, 144 * 12)])),
    # a takes a K1 pass (contracted axes in the middle): its rows follow the destination, all of them chain
    ((16, 4, 16, 32, 16), [1, 3], (12, 4, 256, 32), [1, 3], (3, 4, 1, 0, 2), False, True,
     (True, 4096, [(3072, 4096)], [(4096, 1)])),
    # the same order with a read in place: its innermost-in-destination axis is not its last row axis
    ((16, 4, 16, 32, 16), [1, 3], (12, 4, 256, 32), [1, 3], (3, 4, 1, 2, 0), True, True, None),
    # a run of 6: no multiple of 4
    ((16, 16, 128), [2], (12, 16, 6, 128), [3], (0, 2, 3, 1, 4), True, True, None),
]


_V = _lib.OperandView
_K1024 = _V(1024, 1024, 0, 1024, 1, 0)                  # rows of 1024 contiguous contraction indices
# (A = M side view, rows, B = N side view, rows, K, the entry has a loop): the forms of the chi = 32 MERA layer
_LOOPS = [
    (_K1024, 1024, _K1024, 1 << 20, 1024, True),
    (_V(1024, 1, 32768, 32, 1024, 32768), 1 << 20, _K1024, 1024, 1024, False),        # k-major operand on the M side
    (_K1024, 1024, _V(1024, 1, 1048576, 1024, 1024, 0), 1 << 20, 1024, True),         # k-major N side, one run of 1024
    (_V(32, 32, 32768, 32, 1, 1024), 1024, _V(1024, 1, 32768, 32, 1024, 32768), 1 << 20, 1024, False),   # ... runs of 32
    (_V(32, 32, 32768, 32, 1, 1024), 1 << 20, _K1024, 1024, 1024, True),              # two-level rows, half-K-tile walk
    (_V(1 << 20, 1 << 12, 0, 1 << 12, 1, 0), 1 << 20, _K1024, 1024, 1 << 12, True),   # 8 GiB operand, ascending rows
    (_V(1024, 1 << 24, 0, 1 << 12, 1, 0), 1024, _K1024, 1024, 1 << 12, False),        # a tile's rows span 4 GiB
    (_V(8, 1 << 12, -(1 << 15), 1 << 12, 1, 0), 1 << 19, _K1024, 1024, 1 << 12, False),      # descending outer rows
]


@pytest.mark.parametrize("case", _LOOPS, ids=[str(i) for i in range(len(_LOOPS))])
def test_plan_refuses_what_the_entry_refuses(case):
  va, m, vb, n, k, want = case
  assert hip_backend._view_scatter_loop(va, m, vb, n, k) == want      # pylint: disable=protected-access


def test_tail_split_rule():
  """the D = 12 network's 81 x 7 tiles with 324 K-tiles are split by tnh_gemm_view; short K or one wave of tiles are not"""
  split = hip_backend._view_tail_split      # pylint: disable=protected-access
  assert split(20736, 1728, 20736, 256) and not split(20736, 20736, 1728, 256) and not split(4096, 4096, 8192, 256)


@pytest.mark.parametrize("case", _CASES, ids=[str(i) for i in range(len(_CASES))])
def test_cview_descriptor(case):
  shape_a, axes_a, shape_b, axes_b, order, keep_a, keep_b, want = case
  ext_a = [n for i, n in enumerate(shape_a) if i not in axes_a]
  ext_b = [n for i, n in enumerate(shape_b) if i not in axes_b]
  plan = hip_backend._cview_descriptor(ext_a, ext_b, order, keep_a, keep_b)      # pylint: disable=protected-access
  if want is None:
    assert plan is None
    return
  desc, n_is_a, rows_a, rows_b, run, shape = plan
  m_digits = [(desc.mext[d], desc.mstride[d]) for d in range(desc.nm)]
  n_digits = [(desc.next[d], desc.nstride[d]) for d in range(desc.nn)]
  assert (n_is_a, run, m_digits, n_digits) == want and desc.run == run
  assert shape == tuple((ext_a + ext_b)[p] for p in order) and desc.c_elems == np.prod(shape)

  def offsets(digits):
    off = np.zeros(1, dtype=np.int64)
    for ext, stride in digits:                   # innermost first: each digit becomes the new leading axis
      off = (np.arange(ext, dtype=np.int64)[:, None] * stride + off[None, :]).reshape(-1)
    return off

  got = offsets(m_digits)[:, None] + offsets(n_digits)[None, :]
  # address of every element of the natural result [a's free axes..., b's free axes...] in the transposed destination
  where = np.transpose(np.arange(desc.c_elems, dtype=np.int64).reshape(shape), np.argsort(order))
  na = len(ext_a)
  where = np.transpose(where, list(rows_a) + [na + i for i in rows_b]).reshape(int(np.prod(ext_a)), -1)
  np.testing.assert_array_equal(got, where.T if n_is_a else where)
