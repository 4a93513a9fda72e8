"""The gather GEMM with a scattered epilogue (tnh_gemm_gather_scatter.hip): `tensordot_planned(..., result_order=...)`
writes the product straight in the order asked for -- one launch, no K1 pass over the long operand or the result --
against float64 on the rounded inputs, and bit for bit against transpose(tensordot(...))."""
import ctypes
import functools

import numpy as np
import pytest

import tensornetwork_amd as ta
from tensornetwork_amd import _lib, hip_backend
from oracle import numpy_oracle as orc
from cases import assert_half_gemm_close

pytestmark = pytest.mark.gpu

_S144 = ((12, 12, 12, 12), [1, 3])                  # Ms = 144 (free axes 0, 2), K = 144
_L64 = ((16, 12, 16, 12, 16), [1, 3])               # free axes 0, 2, 4; box = axis 4 x 4 of axis 2, innermost digit free
_L64K = ((16, 12, 16, 16, 12), [1, 4])              # free axes 0, 2, 3 (2, 3 one digit); innermost digit contracted
_S72 = ((6, 12, 12, 16), [1, 3])                    # Ms = 72: the image is padded to 80 rows; K = 192
_L48 = ((12, 16, 12, 16, 12), [0, 3])               # free axes 1, 2, 4; box = axis 4 x 4 of axis 2: BN = 48
# 1856 tiles in two tile digits (4 x 464) on a grid of 512 workgroups (two per CU): workgroups run three or four tiles,
# so both prefetch buffers are filled by an unclamped request and consumed, and the count does not divide by the grid
_BIG = ((29, 16, 12, 16, 12, 16), [2, 4])
# (small, long, destination as a permutation of [small's free axes..., long's free axes...], operand orders (True: small
#  first), kernel)
_CASES = [
    (_S144, _L64, (3, 2, 4, 0, 1), (True, False), "64xS_v16"),       # small axes innermost: runs of 144
    (_S144, _L64, (2, 0, 3, 4, 1), (True, False), "64xS_v8"),        # interleaved, run 12: 8-byte stores
    (_S144, _L64, (0, 2, 1, 3, 4), (True, False), "Sx64_v16"),       # the box's innermost free digit innermost: run 64
    (_S144, _L64, (3, 0, 2, 1, 4), (True,), "Sx64_v16"),             # interleaved, run 16
    (_S144, _L64K, (3, 4, 2, 0, 1), (True, False), "64xS_v16"),
    (_S144, _L64K, (0, 2, 1, 3, 4), (True,), "Sx64_v16"),
    (_S72, _L48, (4, 2, 3, 0, 1), (True, False), "48xS_v16"),        # run 72
    (_S72, _L48, (1, 0, 2, 3, 4), (True,), "Sx48_v16"),              # run 48
    (_S72, _L48, (0, 2, 3, 1, 4), (False,), "Sx48_v8"),              # run 12
    (((16, 5, 6, 8), [1, 3]), ((64, 5, 16, 16, 8), [1, 4]), (2, 3, 4, 0, 1), (True,), "64xS_v16"),      # K = 40: k padding
    (_S144, _BIG, (4, 2, 3, 0, 5, 1), (True, False), "64xS_v8"),     # persistent loop: see _BIG
    (_S144, _BIG, (0, 4, 2, 3, 1, 5), (True,), "Sx64_v16"),
]
_PARAMS = [pytest.param(dtype, i, first, id=f"{name}-{i}-{'Sx' if first else 'xS'}")
           for dtype, name in ((ta.bfloat16, "bf16"), (np.float16, "f16"))
           for i, case in enumerate(_CASES) for first in case[3]]


@functools.lru_cache(maxsize=2)
def _operands(small, long_, is_bf16):
  """rounded inputs and their float64 product [small's free axes..., long's free axes...]"""
  (shape_s, axes_s), (shape_l, axes_l) = small, long_
  rng = np.random.default_rng(len(shape_l) * 100 + shape_s[0])
  s = rng.standard_normal(shape_s).astype(np.float32) / 8
  l = rng.standard_normal(shape_l).astype(np.float32) / 8
  s, l = (orc.round_bf16(s), orc.round_bf16(l)) if is_bf16 else (s.astype(np.float16), l.astype(np.float16))
  return s, l, np.tensordot(s.astype(np.float64), l.astype(np.float64), [axes_s, axes_l])


def _freeze(case):
  return tuple((shape, tuple(axes)) for shape, axes in case[:2])


def _call(hip, case, small_first, is_bf16, dest):
  """(arguments of tensordot, result_order for `dest`) with either operand first"""
  (_, axes_s), (_, axes_l) = case[:2]
  s, l, _ = _operands(*_freeze(case), is_bf16)
  ds, dl = (hip.to_bfloat16(s), hip.to_bfloat16(l)) if is_bf16 else (hip.convert_to_tensor(s), hip.convert_to_tensor(l))
  ns = s.ndim - len(axes_s)
  if small_first:
    return (ds, dl, [axes_s, axes_l]), list(dest)
  natural = list(range(ns, len(dest))) + list(range(ns))       # the long operand's axes come first
  return (dl, ds, [axes_l, axes_s]), [natural.index(p) for p in dest]


@pytest.mark.parametrize("dtype,i,small_first", _PARAMS)
def test_scatter_gather_writes_the_consumers_order(hip, dtype, i, small_first):
  case = _CASES[i]
  is_bf16 = dtype is ta.bfloat16
  ref = np.transpose(_operands(*_freeze(case), is_bf16)[2], case[2])
  args, order = _call(hip, case, small_first, is_bf16, case[2])
  keep = hip.gather_min_rows
  hip.gather_min_rows = 1024
  try:
    before = (hip.gather_scatter_launches, hip.gather_launches, hip.permute_launches)
    got = hip.tensordot_planned(*args, result_order=order)[0]
    kernel = hip.lib.tnh_gemm_last_kernel().decode()
    assert hip.gather_scatter_launches - before[0] == 1, _lib.last_error()
    assert hip.gather_launches == before[1] and hip.permute_launches - before[2] == 1      # the small operand's
    assert kernel == "bf16_gather_scatter_" + case[4]
    classic = hip.transpose(hip.tensordot(*args), order)
  finally:
    hip.gather_min_rows = keep
  g = np.asarray(got)
  assert_half_gemm_close(g, ref, "bf16" if is_bf16 else "f16")
  np.testing.assert_array_equal(g, np.asarray(classic))


def test_refused_order_takes_the_fallback(hip):
  """innermost destination axis = a long digit outside the box: no scatter launch, same values"""
  case = (_S144, _L64, (0, 3, 1, 4, 2))
  ref = np.transpose(_operands(*_freeze(case), True)[2], case[2])
  args, order = _call(hip, case, True, True, case[2])
  keep = hip.gather_min_rows
  hip.gather_min_rows = 1024
  try:
    before = hip.gather_scatter_launches
    got = hip.tensordot_planned(*args, result_order=order)[0]
    assert hip.gather_scatter_launches == before
  finally:
    hip.gather_min_rows = keep
  assert_half_gemm_close(np.asarray(got), ref, "bf16")


def _c_entry(hip, dest_shape, long_pos, small_pos, spoil=None):
  """tnh_gemm_gather_scatter called directly on (_S144, _L64) with the destination `dest_shape`, in which the long
  tensor's free axes 0, 2, 4 are the axes `long_pos` and the small operand's the axes `small_pos`"""
  shape_l, axes_l = _L64
  strides = hip_backend._row_major_strides(dest_shape)      # pylint: disable=protected-access
  out_strides = [strides[long_pos[0]], 0, strides[long_pos[1]], 0, strides[long_pos[2]]]
  desc, out, _, _ = hip_backend._scatter_descriptor(shape_l, axes_l, out_strides, [12, 12],      # pylint: disable=protected-access
                                                    [strides[p] for p in small_pos])
  out = _lib.ScatterDesc.from_buffer_copy(out)
  if spoil is not None:
    spoil(out)
  s = ta.DeviceTensor.empty((144, 144), _lib.BF16)
  l = ta.DeviceTensor.empty(shape_l, _lib.BF16)
  c = ta.DeviceTensor.empty((4096 * 144,), _lib.BF16)
  return hip.lib.tnh_gemm_gather_scatter(_lib.BF16, 144, 144, 4096, ctypes.c_void_p(s.ptr), 144, ctypes.c_void_p(l.ptr),
                                         l.size, ctypes.byref(desc), ctypes.c_void_p(c.ptr), ctypes.byref(out))


def test_c_entry_rejects_a_destination_that_is_no_bijection(hip):
  def spoil(out):
    out.sstride[1] = 24                # rows of the small operand 24 apart: half of the destination is written twice
  assert _c_entry(hip, (16, 16, 16, 12, 12), (0, 1, 2), (3, 4), spoil) == _lib.ERR_INVALID, _lib.last_error()


def test_c_entry_refuses_an_innermost_tile_digit_without_a_launch(hip):
  """destination [small axes, long axes 2, 4, 0]: its innermost axis is a digit of the tile number"""
  before = hip.lib.tnh_gemm_last_kernel()
  assert _c_entry(hip, (12, 12, 16, 16, 16), (4, 2, 3), (0, 1)) == _lib.ERR_UNSUPPORTED, _lib.last_error()
  assert hip.lib.tnh_gemm_last_kernel() == before
