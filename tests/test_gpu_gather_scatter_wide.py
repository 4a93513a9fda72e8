"""The wide gather GEMM with a scattered epilogue (tnh_gemm_gather_scatter_wide.hip): `tensordot_planned(...,
result_order=...)` for small operands of 193 ... 256 free tuples -- one launch, no K1 pass over the long operand or the
result -- against float64 on the rounded inputs, and bit for bit against transpose(tensordot(...)) where that call runs
the wide gather kernel (the view GEMM of trailing contracted axes sums k in another order)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import tensornetwork_amd as ta
from tensornetwork_amd import _lib, hip_backend
from cases import assert_half_gemm_close
from test_gpu_gather_scatter import _call, _freeze, _operands

pytestmark = pytest.mark.gpu

_S256 = ((16, 16, 16, 16), [1, 3])                  # Ms = K = 256: LDS exactly 160 KB, the tables lie under the first image
_S208 = ((13, 16, 16, 16), [1, 3])                  # 13 fragments: the waves own 4, 3, 3, 3
_S200 = ((10, 16, 20, 16), [1, 3])                  # image padded to 208 rows; innermost free axis 20: 8-byte stores
_L64 = ((16,) * 5, [1, 3])                          # free axes 0, 2, 4; box = axis 4 x 4 of axis 2, innermost digit free
_L64K = ((16,) * 5, [1, 4])                         # free axes 0, 2, 3 (2, 3 one digit); innermost digit contracted
_K200 = (((16, 10, 16, 20), [1, 3]), ((16, 10, 16, 20, 16), [1, 3]))      # K = 200: Kp = 224, three chunks of k padding
_K40 = (((16, 5, 16, 8), [1, 3]), ((64, 5, 16, 16, 8), [1, 4]))
_S48, _L48 = ((16, 12, 16, 16), [1, 3]), ((12, 16, 12, 16, 12), [0, 3])     # BN = 48: box = axis 4 x 4 of axis 2, K = 192
# 832 tiles in two tile digits (4 x 208) on one workgroup per CU: workgroups run three or four tiles, so both prefetch
# buffers are filled by an unclamped request and consumed, and the count does not divide by the grid
_BIG = ((13, 16, 16, 16, 16, 16), [2, 4])
# (small, long, destination as a permutation of [small's free axes..., long's free axes...], operand orders (True: small
#  first), kernel)
_CASES = [
    (_S256, _L64, (3, 2, 4, 0, 1), (True, False), "64xS_v16"),       # small axes innermost: runs of 256
    (_S256, _L64, (0, 2, 1, 3, 4), (True, False), "Sx64_v16"),       # the box's innermost free digit innermost: run 64
    (_S256, _L64K, (2, 0, 3, 4, 1), (True,), "64xS_v16"),            # interleaved, run 16
    (_S256, _L64K, (0, 2, 1, 3, 4), (True,), "Sx64_v16"),
    (_S208, _L64, (3, 2, 4, 0, 1), (True, False), "64xS_v16"),
    (_S208, _L64, (3, 0, 2, 1, 4), (True,), "Sx64_v16"),             # interleaved, run 16
    (_S200, _L64K, (2, 0, 3, 4, 1), (True, False), "64xS_v8"),       # run 20
    (_S200, _L64K, (0, 2, 1, 3, 4), (False,), "Sx64_v16"),
    (*_K200, (3, 2, 4, 0, 1), (True,), "64xS_v16"),
    (*_K200, (0, 2, 1, 3, 4), (False,), "Sx64_v16"),
    (*_K40, (2, 3, 4, 0, 1), (True,), "64xS_v16"),
    (_S48, _L48, (4, 2, 3, 0, 1), (True, False), "48xS_v16"),
    (_S48, _L48, (1, 0, 2, 3, 4), (True,), "Sx48_v16"),              # 96-byte plain staging rows, run 48
    (_S48, _L48, (0, 2, 3, 1, 4), (False,), "Sx48_v8"),              # run 12
    (_S256, _BIG, (4, 2, 3, 0, 5, 1), (True, False), "64xS_v16"),    # persistent loop: see _BIG
    (_S256, _BIG, (0, 4, 2, 3, 1, 5), (True,), "Sx64_v16"),
]
_PARAMS = [pytest.param(dtype, i, first, id=f"{name}-{i}-{'Sx' if first else 'xS'}")
           for dtype, name in ((ta.bfloat16, "bf16"), (np.float16, "f16"))
           for i, case in enumerate(_CASES) for first in case[3]]


def _run(hip, args, order):
  """(scattered result, its kernel, scatter / gather / permute launches it took, classic result, its GEMM kernel)"""
  keep = (hip.gather_min_rows, hip.gather_max_small)
  hip.gather_min_rows, hip.gather_max_small = 1024, 256
  try:
    before = (hip.gather_scatter_launches, hip.gather_launches, hip.permute_launches)
    got = hip.tensordot_planned(*args, result_order=order)[0]
    kernel = hip.lib.tnh_gemm_last_kernel().decode()
    counts = tuple(x - y for x, y in zip((hip.gather_scatter_launches, hip.gather_launches, hip.permute_launches), before))
    natural = hip.tensordot(*args)
    return got, kernel, counts, hip.transpose(natural, order), hip.lib.tnh_gemm_last_kernel().decode()
  finally:
    hip.gather_min_rows, hip.gather_max_small = keep


@pytest.mark.parametrize("dtype,i,small_first", _PARAMS)
def test_wide_scatter_gather_writes_the_consumers_order(hip, dtype, i, small_first):
  case = _CASES[i]
  is_bf16 = dtype is ta.bfloat16
  ref = np.transpose(_operands(*_freeze(case), is_bf16)[2], case[2])
  got, kernel, counts, classic, classic_kernel = _run(hip, *_call(hip, case, small_first, is_bf16, case[2]))
  assert counts == (1, 0, 1), (counts, _lib.last_error())      # one scatter launch, the small operand's permute
  assert kernel == "bf16_gather_scatter_wide_" + case[4]
  g = np.asarray(got)
  assert_half_gemm_close(g, ref, "bf16" if is_bf16 else "f16")
  if classic_kernel.startswith("bf16_gather_wide_"):
    np.testing.assert_array_equal(g, np.asarray(classic))


def test_refused_order_takes_the_fallback(hip):
  """innermost destination axis = a long digit outside the box: no scatter launch, same values"""
  case = (_S256, _L64, (0, 3, 1, 4, 2))
  ref = np.transpose(_operands(*_freeze(case), True)[2], case[2])
  got, _, counts, _, _ = _run(hip, *_call(hip, case, True, True, case[2]))
  assert counts[0] == 0
  assert_half_gemm_close(np.asarray(got), ref, "bf16")


def _c_entry(hip, dest_shape, long_pos, small_pos, spoil=None):
  """tnh_gemm_gather_scatter called directly on (_S256, _L64) with the destination `dest_shape`, in which the long
  tensor's free axes 0, 2, 4 are the axes `long_pos` and the small operand's the axes `small_pos`; (status, whether
  tnh_gemm_last_kernel changed)"""
  shape_l, axes_l = _L64
  strides = hip_backend._row_major_strides(dest_shape)      # pylint: disable=protected-access
  out_strides = [strides[long_pos[0]], 0, strides[long_pos[1]], 0, strides[long_pos[2]]]
  desc, out, _, _ = hip_backend._scatter_descriptor(shape_l, axes_l, out_strides, [16, 16],      # pylint: disable=protected-access
                                                    [strides[p] for p in small_pos], 256)
  out = _lib.ScatterDesc.from_buffer_copy(out)
  if spoil is not None:
    spoil(out)
  s, l = ta.DeviceTensor.empty((256, 256), _lib.BF16), ta.DeviceTensor.empty(shape_l, _lib.BF16)
  c = ta.DeviceTensor.empty((4096 * 256,), _lib.BF16)
  before = hip.lib.tnh_gemm_last_kernel()
  status = hip.lib.tnh_gemm_gather_scatter(_lib.BF16, 256, 256, 4096, ctypes.c_void_p(s.ptr), 256, ctypes.c_void_p(l.ptr),
                                           l.size, ctypes.byref(desc), ctypes.c_void_p(c.ptr), ctypes.byref(out))
  return status, hip.lib.tnh_gemm_last_kernel() != before


_GOOD = ((16, 16, 16, 16, 16), (0, 1, 2), (3, 4))      # destination [long axes 0, 2, 4, small axes]


def test_c_entry_at_256_rows(hip):
  """a spoiled sstride (half of the destination written twice) is invalid; an innermost tile digit (destination [small
  axes, long axes 2, 4, 0]) and the library's knobs turned off are unsupported, nothing launched"""
  assert _c_entry(hip, *_GOOD, lambda out: out.sstride.__setitem__(1, 32))[0] == _lib.ERR_INVALID, _lib.last_error()
  assert _c_entry(hip, (16, 16, 16, 16, 16), (4, 2, 3), (0, 1)) == (_lib.ERR_UNSUPPORTED, False), _lib.last_error()
  assert _c_entry(hip, *_GOOD) == (_lib.OK, True), _lib.last_error()
  code = ("import sys; sys.path.insert(1, '..')\n"
          "import tensornetwork_amd as ta, test_gpu_gather_scatter_wide as t\n"
          "assert t._c_entry(ta.get_hip_backend(), *t._GOOD) == (ta._lib.ERR_UNSUPPORTED, False)")
  for knob in ("TNH_GATHER_SCATTER", "TNH_GATHER_WIDE"):
    proc = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(__file__), env={**os.environ, knob: "0"},
                          capture_output=True, text=True, timeout=300, check=False)
    assert proc.returncode == 0, (knob, proc.stderr[-2000:])


def test_destination_of_2_to_the_31_elements(hip):
  """Ms = 256, K = 8, Nl = 2^23: destination offsets past 2^31 bytes and up to 2^31 elements.  The first and the last
  slab along the destination's outermost axis, bit for bit against the same slabs of the classic result."""
  s = hip.to_bfloat16(np.random.default_rng(7).standard_normal((16, 8, 16)).astype(np.float32) / 8)
  long_ = hip.device_random((128, 8, 256, 256), dtype=ta.bfloat16, seed=5, normal=True, a=0.0, b=0.125)
  got, kernel, counts, classic, classic_kernel = _run(hip, (s, long_, [[1], [1]]), [2, 0, 3, 4, 1])
  assert counts == (1, 0, 1) and kernel == "bf16_gather_scatter_wide_64xS_v16", _lib.last_error()
  assert classic_kernel == "bf16_gather_wide_Sx64" and got.shape == (128, 16, 256, 256, 16)
  for lead in ((0,), (127,)):
    np.testing.assert_array_equal(np.asarray(got[lead]), np.asarray(classic[lead]))
