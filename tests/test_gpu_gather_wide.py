"""The wide gather GEMM (tnh_gemm_gather_wide.hip): small operands of 193 ... 256 free tuples against ONE box of up to
256 contracted indices of a long tensor that is read where it lies, against float64 on the rounded inputs."""
import ctypes
import functools

import numpy as np
import pytest

import tensornetwork_amd as ta
from tensornetwork_amd import _lib, hip_backend
from oracle import numpy_oracle as orc

pytestmark = pytest.mark.gpu

# (shape_small, shape_long, axes_small, axes_long, orders of the operands (True: small first), BN)
_CASES = [
    ((16, 16, 16, 16), (16,) * 5, [1, 3], [1, 3], (True, False), 64),     # innermost axis free, Ms = K = 256: all 160 KB
    ((16, 16, 16, 16), (16,) * 5, [1, 3], [1, 4], (True, False), 64),     # innermost axis contracted
    ((16, 16, 16, 16), (16,) * 5, [1, 3], [0, 1], (True,), 64),           # k-major
    ((16, 16, 16, 16), (12, 16, 12, 16, 12), [1, 3], [1, 3], (True, False), 48),
    ((10, 16, 20, 16), (16,) * 5, [1, 3], [1, 4], (True, False), 64),     # Ms = 200: msp = 208, zero rows in the image
    ((10, 16, 25, 16), (16,) * 5, [1, 3], [1, 3], (True,), 64),           # Ms = 250, not a multiple of 8
    ((16, 14, 16, 16), (16, 14, 16, 16, 16), [1, 3], [1, 3], (True,), 64),     # K = 224: k-padding columns
    ((16, 5, 16, 8), (64, 5, 16, 16, 8), [1, 3], [1, 4], (True, False), 64),   # K = 40
    # 53 248 rows = 832 tiles on 256 workgroups: the persistent loop, both prefetch buffers and an uneven tail
    ((16, 16, 16, 16), (13, 16, 16, 16, 16, 16), [1, 3], [2, 4], (True, False), 64),
]
_PARAMS = [pytest.param(dtype, i, first, id=f"{name}-{i}-{'Sx' if first else 'xS'}")
           for dtype, name in ((ta.bfloat16, "bf16"), (np.float16, "f16"))
           for i, case in enumerate(_CASES) for first in case[4]]


@functools.lru_cache(maxsize=1)
def _operands(i, is_bf16):
  """rounded inputs of case i and their float64 product [small's free axes..., long's free axes...]"""
  shape_s, shape_l, axes_s, axes_l = _CASES[i][:4]
  rng = np.random.default_rng(900 + i)
  s = rng.standard_normal(shape_s).astype(np.float32) / 8
  l = rng.standard_normal(shape_l).astype(np.float32) / 8
  s, l = (orc.round_bf16(s), orc.round_bf16(l)) if is_bf16 else (s.astype(np.float16), l.astype(np.float16))
  return s, l, np.tensordot(s.astype(np.float64), l.astype(np.float64), [axes_s, axes_l])


def _dev(hip, x, is_bf16):
  return hip.to_bfloat16(x) if is_bf16 else hip.convert_to_tensor(x)


@pytest.mark.parametrize("dtype,i,small_first", _PARAMS)
def test_wide_gather_reads_the_long_operand_in_place(hip, dtype, i, small_first):
  """ONE tnh_gemm_gather launch of the wide kernel, no K1 pass over the long operand; values against float64, and the
  classic lowering (permute + tile kernels) of the same call against the same bound."""
  axes_s, axes_l, bn = _CASES[i][2], _CASES[i][3], _CASES[i][5]
  is_bf16 = dtype is ta.bfloat16
  s, l, ref = _operands(i, is_bf16)
  if not small_first:
    ref = np.moveaxis(ref, (0, 1), (-2, -1))
  ds, dl = _dev(hip, s, is_bf16), _dev(hip, l, is_bf16)
  args = (ds, dl, [axes_s, axes_l]) if small_first else (dl, ds, [axes_l, axes_s])
  keep = (hip.gather_gemm, hip.gather_min_rows, hip.gather_max_small)
  hip.gather_min_rows, hip.gather_max_small = 1024, 256
  try:
    hip.gather_gemm = True
    before = (hip.gather_launches, hip.permute_launches)
    got = hip.tensordot(*args)
    kernel = hip.lib.tnh_gemm_last_kernel().decode()
    assert hip.gather_launches - before[0] == 1, _lib.last_error()
    assert hip.permute_launches - before[1] <= 1          # the small operand at most
    assert kernel == (f"bf16_gather_wide_Sx{bn}" if small_first else f"bf16_gather_wide_{bn}xS")
    hip.gather_gemm = False
    classic = hip.tensordot(*args)
  finally:
    hip.gather_gemm, hip.gather_min_rows, hip.gather_max_small = keep
  g, c = np.asarray(got), np.asarray(classic)
  assert g.shape == ref.shape
  np.testing.assert_allclose(g, ref, rtol=2.0**-8, atol=2e-3)
  np.testing.assert_allclose(c, ref, rtol=2.0**-8, atol=2e-3)


def test_wide_gather_on_a_tensor_of_2_to_the_32_elements(hip):
  """Bond D = 16 at full size, 256 x 16 777 216 x 256: box origins and output rows past 2^31 elements.  The first and
  the last block of the result (leading free indices 0,0,0 and 15,15,15) against float64 on the same block of the input."""
  s = orc.round_bf16(np.random.default_rng(990).standard_normal((16,) * 4).astype(np.float32) / 8)
  long_ = hip.device_random((16,) * 8, dtype=ta.bfloat16, seed=5, normal=True, a=0.0, b=0.125)
  keep = (hip.gather_gemm, hip.gather_max_small)
  hip.gather_gemm, hip.gather_max_small = True, 256
  try:
    got, _, _, swapped = hip.tensordot_planned(hip.to_bfloat16(s), long_, [[1, 3], [4, 7]], None, None, allow_swap=True)
  finally:
    hip.gather_gemm, hip.gather_max_small = keep
  assert swapped and hip.lib.tnh_gemm_last_kernel().decode() == "bf16_gather_wide_64xS"
  assert got.shape == (16,) * 8
  for lead in ((0, 0, 0), (15, 15, 15)):
    block = np.asarray(long_[lead]).astype(np.float64)                 # axes 3 ... 7 of the long tensor
    ref = np.tensordot(block, s.astype(np.float64), [[1, 4], [1, 3]])
    np.testing.assert_allclose(np.asarray(got[lead]), ref, rtol=2.0**-8, atol=2e-3)


def test_wide_gather_c_abi_range_and_64_bit_output_rows(hip):
  """Ms = K = 256 is inside the C entry point's range, Ms = 257 and a box of 264 indices are refused without a launch,
  and the C[Ms, Nl] form takes rows that lie 2^22 + 8 elements apart (Ms x ldc >= 2^30: 64-bit row addresses)."""
  s, l, ref = _operands(0, True)
  desc, bn, rows = hip_backend._gather_descriptor(l.shape, [1, 3], max_box_k=256)      # pylint: disable=protected-access
  assert (bn, rows) == (64, 4096)
  dl = hip.to_bfloat16(l)
  ds = hip.to_bfloat16(np.ascontiguousarray(s.transpose(0, 2, 1, 3)).reshape(256, 256))
  ldc = 2**22 + 8
  out = ta.DeviceTensor.empty((256 * ldc,), _lib.BF16)      # ~2 GB, only 256 x 4096 of it written

  def call(ms=256, k=256):
    return hip.lib.tnh_gemm_gather(_lib.BF16, ms, k, rows, ctypes.c_void_p(ds.ptr), k, ctypes.c_void_p(dl.ptr), l.size,
                                   ctypes.byref(desc), ctypes.c_void_p(out.ptr), ldc, 1)

  assert call(ms=257) == _lib.ERR_UNSUPPORTED
  assert call(k=264) == _lib.ERR_UNSUPPORTED
  assert call() == _lib.OK, _lib.last_error()
  assert hip.lib.tnh_gemm_last_kernel().decode() == "bf16_gather_wide_Sx64"
  got = np.asarray(hip._dense(out.as_rows(256, rows, ldc)))      # pylint: disable=protected-access
  np.testing.assert_allclose(got, ref.reshape(256, rows), rtol=2.0**-8, atol=2e-3)
