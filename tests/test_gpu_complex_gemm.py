"""complex64 / complex128 GEMM on the matrix cores (tnh_gemm_complex.hip: mfma_c64_* / mfma_c128_*) against
np.matmul in complex128 on the same rounded inputs.  Tolerance: the rule of test_gemm_all_layouts_ragged
(assert_gemm(scale_k=True)) -- rtol = T sqrt(K), atol = T K with T = 3e-6 (complex64) / 1e-14 (complex128)."""
import ctypes

import numpy as np
import pytest

from tensornetwork_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {np.complex64: 3e-6, np.complex128: 1e-14}
PREFIX = {np.complex64: "mfma_c64", np.complex128: "mfma_c128"}
DTYPES = [np.complex64, np.complex128]


def _operands(dtype, a_shape, b_shape, ta_=0, tb_=0):
  """Operands whose re / im parts are four independent draws (a swapped plane or a wrong sign cannot cancel), as stored
  ([..., K, M] with ta_, [..., N, K] with tb_), and the complex128 product of the rounded values."""
  rng = np.random.default_rng(sum(a_shape) + 7 * sum(b_shape))
  a = (rng.standard_normal(a_shape) + 1j * rng.uniform(-2.0, 1.0, a_shape)).astype(dtype)
  b = (rng.uniform(-1.0, 3.0, b_shape) + 1j * rng.standard_normal(b_shape)).astype(dtype)
  ea = np.swapaxes(a, -1, -2) if ta_ else a
  eb = np.swapaxes(b, -1, -2) if tb_ else b
  return a, b, np.matmul(ea.astype(np.complex128), eb.astype(np.complex128))


def _close(out, ref, dtype, k):
  np.testing.assert_allclose(out, ref, rtol=TOL[dtype] * np.sqrt(k), atol=TOL[dtype] * k)


@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 15, 5), (64, 257, 33), (130, 70, 129), (257, 129, 40)])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("ta_,tb_", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_native_tensordot_every_layout_and_tile(hip, monkeypatch, dtype, ta_, tb_, tile, shape):
  m, n, k = shape
  a, b, ref = _operands(dtype, (k, m) if ta_ else (m, k), (n, k) if tb_ else (k, n), ta_, tb_)
  monkeypatch.setattr(hip, "complex_lowering", "native")
  _lib.check(hip.lib.tnh_gemm_set_variant(f"auto:z{tile}".encode()))
  try:
    out = hip.tensordot(hip.convert_to_tensor(a), hip.convert_to_tensor(b), [[0 if ta_ else 1], [1 if tb_ else 0]])
    name = hip.lib.tnh_gemm_last_kernel().decode()
  finally:
    _lib.check(hip.lib.tnh_gemm_set_variant(b"auto"))
  assert name.startswith(PREFIX[dtype]), name
  _close(np.asarray(out), ref, dtype, k)


@pytest.mark.parametrize("a_shape,b_shape", [((5, 40, 56), (5, 56, 24)), ((3, 130, 33), (3, 33, 70)),
                                             ((3, 130, 33), (33, 70))])
@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_matmul_default_settings(hip, dtype, a_shape, b_shape):
  a, b, ref = _operands(dtype, a_shape, b_shape)
  da, db = hip.convert_to_tensor(a), hip.convert_to_tensor(b)
  out = np.asarray(hip.matmul(da, db))
  name = hip.lib.tnh_gemm_last_kernel().decode()
  assert name.startswith(PREFIX[dtype]), name
  _close(out, ref, dtype, a_shape[-1])
  _lib.check(hip.lib.tnh_gemm_set_variant(b"valu"))
  try:
    valu = np.asarray(hip.matmul(da, db))
    assert hip.lib.tnh_gemm_last_kernel().decode() == "valu_64x64x16"
  finally:
    _lib.check(hip.lib.tnh_gemm_set_variant(b"auto"))
  _close(valu, ref, dtype, a_shape[-1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_ex_alpha_beta(hip, dtype):
  m, n, k = 130, 70, 33
  a, b, ab = _operands(dtype, (m, k), (k, n))
  c0 = (np.linspace(-1.0, 1.0, m * n).reshape(m, n) - 0.5j * np.linspace(0.0, 2.0, m * n).reshape(m, n)).astype(dtype)
  da, db, dc = hip.convert_to_tensor(a), hip.convert_to_tensor(b), hip.convert_to_tensor(c0)
  code = da.code
  ptr = lambda t: ctypes.c_void_p(t.ptr)
  _lib.check(hip.lib.tnh_gemm_ex(code, code, 0, 0, m, n, k, ptr(da), k, ptr(db), n, ptr(dc), n, 1, 0, 0, m * n,
                                 0.5, 2.0), "tnh_gemm_ex")
  assert hip.lib.tnh_gemm_last_kernel().decode().startswith(PREFIX[dtype])
  ref = 0.5 * ab + 2.0 * c0.astype(np.complex128)
  _close(np.asarray(dc), ref, dtype, k)
