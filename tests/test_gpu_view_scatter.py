"""The 256 x 256 view GEMM with a scattered epilogue (tnh_gemm_view_scatter): `tensordot_planned(..., result_order=...)`
writes a large product straight in the order asked for -- one GEMM launch, no K1 pass over the result -- against float64
on the rounded inputs, and bit for bit against transpose(tensordot(...))."""
import ctypes
import functools

import numpy as np
import pytest

import tensornetwork_amd as ta
from tensornetwork_amd import _lib, hip_backend
from oracle import numpy_oracle as orc
from cases import assert_half_gemm_close

pytestmark = pytest.mark.gpu

_A16 = ((16, 16, 16, 128), [3])                 # 4096 rows (16 tiles), read in place
_B16 = ((12, 16, 16, 128), [3])                 # 3072 rows (12 tiles): 192 tiles, all full
_NT, _NN = "bf16_view_nt_256x256x64_pp_scatter_", "bf16_view_nn_256x256x64_pp_scatter_"
# (a, b, result_order over [a's free axes..., b's free axes...], K1 passes over operands, kernel, run elements)
_CASES = [
    (_A16, _B16, (0, 3, 1, 4, 2, 5), 0, _NT + "v16", 16),           # both in place, interleaved, b's last axis innermost
    # extents of 12: 8-byte stores; M = 1728 and N = 8640 end in ragged tiles (7 x 34)
    (((12, 12, 12, 128), [3]), ((5, 12, 12, 12, 128), [4]), (3, 0, 4, 1, 5, 2, 6), 0, _NT + "v8", 12),
    (_A16, _B16, (3, 0, 4, 1, 5, 2), 0, _NT + "v16", 16),           # a's last axis innermost: operand roles swapped
    # a's contracted axes sit in the middle: ONE K1 pass, into destination order (a1, a0, a2) -- its three axes chain;
    # b is a two-level view with contraction runs of 32 (the half-K-tile walk) and becomes the kernel's A
    (((16, 4, 16, 32, 16), [1, 3]), ((12, 4, 256, 32), [1, 3]), (3, 4, 1, 0, 2), 1, _NT + "v16", 4096),
    (_A16, ((128, 12, 16, 16), [0]), (0, 3, 1, 4, 2, 5), 0, _NN + "v16", 16),       # k-major b: the whole-K-tile loop
    # 16 x 17 tiles on 256 workgroups: the persistent loop, the next tile's loads under the stores
    (((16, 16, 16, 192), [3]), ((17, 16, 16, 192), [3]), (0, 3, 1, 4, 2, 5), 0, _NT + "v16", 16),
    (_A16, ((5, 6, 12, 12, 128), [4]), (0, 3, 1, 4, 5, 2, 6), 0, _NT + "v8", 12),
]
_PARAMS = [pytest.param(dtype, i, id=f"{name}-{i}") for dtype, name in ((ta.bfloat16, "bf16"), (np.float16, "f16"))
           for i in range(len(_CASES))]


@functools.lru_cache(maxsize=2)
def _operands(a, b, is_bf16):
  """rounded inputs and their float64 product [a's free axes..., b's free axes...]"""
  (shape_a, axes_a), (shape_b, axes_b) = a, b
  rng = np.random.default_rng(len(shape_b) * 100 + shape_b[0])
  x = rng.standard_normal(shape_a).astype(np.float32) / 8
  y = rng.standard_normal(shape_b).astype(np.float32) / 8
  x, y = (orc.round_bf16(x), orc.round_bf16(y)) if is_bf16 else (x.astype(np.float16), y.astype(np.float16))
  return x, y, np.tensordot(x.astype(np.float64), y.astype(np.float64), [axes_a, axes_b])


def _freeze(case):
  return tuple((shape, tuple(axes)) for shape, axes in case[:2])


def _run(hip, args, order):
  """(result of the planned call, kernel, scatter launches, K1 launches) with the threshold out of the way"""
  keep = hip.view_scatter_min_run_bytes
  hip.view_scatter_min_run_bytes = 8
  try:
    before = (hip.view_scatter_launches, hip.permute_launches)
    got = hip.tensordot_planned(*args, result_order=list(order))[0]
    kernel = hip.lib.tnh_gemm_last_kernel().decode()
    return got, kernel, hip.view_scatter_launches - before[0], hip.permute_launches - before[1]
  finally:
    hip.view_scatter_min_run_bytes = keep


@pytest.mark.parametrize("dtype,i", _PARAMS)
def test_view_gemm_writes_the_consumers_order(hip, dtype, i):
  case = _CASES[i]
  is_bf16 = dtype is ta.bfloat16
  x, y, ref = _operands(*_freeze(case), is_bf16)
  to = hip.to_bfloat16 if is_bf16 else hip.convert_to_tensor
  args = (to(x), to(y), [case[0][1], case[1][1]])
  keep = hip.view_scatter_min_run_bytes
  hip.view_scatter_min_run_bytes = 8
  try:
    assert hip.scatter_run_bytes(*args, list(case[2])) == 2 * case[5]
  finally:
    hip.view_scatter_min_run_bytes = keep
  got, kernel, launches, passes = _run(hip, args, case[2])
  assert launches == 1, _lib.last_error()
  assert passes == case[3] and kernel == case[4]
  classic = hip.transpose(hip.tensordot(*args), case[2])
  g = np.asarray(got)
  assert_half_gemm_close(g, np.transpose(ref, case[2]), "bf16" if is_bf16 else "f16")
  np.testing.assert_array_equal(g, np.asarray(classic))


def test_destination_beyond_2_31_elements(hip):
  """49152 x 49152 (2.4e9 elements): the first and the last slab of the destination, bit for bit against the fallback
  (there is no float64 product at this size): 64-bit offsets"""
  a = hip.device_random((48, 32, 32, 128), ta.bfloat16, seed=1)
  b = hip.device_random((48, 32, 32, 128), ta.bfloat16, seed=2)
  order = (0, 3, 1, 4, 2, 5)
  got, kernel, launches, _ = _run(hip, (a, b, [[3], [3]]), order)
  assert launches == 1 and kernel == _NT + "v16", _lib.last_error()
  slabs = [np.asarray(got[i, i]) for i in (0, 47)]
  del got
  classic = hip.transpose(hip.tensordot(a, b, [[3], [3]]), order)
  for i, slab in zip((0, 47), slabs):
    assert np.any(slab)
    np.testing.assert_array_equal(slab, np.asarray(classic[i, i]))


def test_refused_order_takes_the_fallback(hip):
  """innermost destination axis = a non-last free axis of an operand read in place: no scatter launch, same values"""
  x, y, ref = _operands(*_freeze(_CASES[0]), True)
  order = (0, 3, 2, 5, 4, 1)
  got, _, launches, _ = _run(hip, (hip.to_bfloat16(x), hip.to_bfloat16(y), [[3], [3]]), order)
  assert launches == 0
  assert_half_gemm_close(np.asarray(got), np.transpose(ref, order), "bf16")


def _c_entry(hip, n_is_a, spoil=None):
  """tnh_gemm_view_scatter called directly on 4096 x 128 and 3072 x 128 operands; `n_is_a`: the descriptor of the order
  whose innermost axis is a's, WITHOUT swapping the operands (m and n of the descriptor exchanged to keep M and N)"""
  desc = hip_backend._cview_descriptor((16, 16, 16), (12, 16, 16), (3, 0, 4, 1, 5, 2) if n_is_a else (0, 3, 1, 4, 2, 5),      # pylint: disable=protected-access
                                       True, True)[0]
  if n_is_a:
    desc = _lib.CViewDesc(desc.nn, desc.nm, desc.next, desc.mext, desc.nstride, desc.mstride, desc.run, desc.c_elems)
  else:
    desc = _lib.CViewDesc.from_buffer_copy(desc)
  if spoil is not None:
    spoil(desc)
  a = ta.DeviceTensor.empty((4096, 128), _lib.BF16)
  b = ta.DeviceTensor.empty((3072, 128), _lib.BF16)
  c = ta.DeviceTensor.empty((4096 * 3072,), _lib.BF16)
  va, vb = _lib.OperandView(4096, 128, 0, 128, 1, 0), _lib.OperandView(3072, 128, 0, 128, 1, 0)
  return hip.lib.tnh_gemm_view_scatter(_lib.BF16, 4096, 3072, 128, ctypes.c_void_p(a.ptr), ctypes.byref(va),
                                       ctypes.c_void_p(b.ptr), ctypes.byref(vb), ctypes.c_void_p(c.ptr), ctypes.byref(desc))


def test_c_entry_rejects_a_destination_that_is_no_bijection(hip):
  def spoil(desc):
    desc.mstride[1] = desc.mstride[0]      # two digits of m on top of each other
  assert _c_entry(hip, False, spoil) == _lib.ERR_INVALID, _lib.last_error()


def test_c_entry_refuses_an_innermost_axis_on_the_m_side_without_a_launch(hip):
  before = hip.lib.tnh_gemm_last_kernel()
  assert _c_entry(hip, True) == _lib.ERR_UNSUPPORTED, _lib.last_error()
  assert hip.lib.tnh_gemm_last_kernel() == before
