"""Native complex64 / complex128 Householder QR (tnh_qr on interleaved data, HipBackend.complex_qr = "native") against
np.linalg.qr in complex128, phase-fixed to a non-negative diagonal.  Tolerances are those of cases.check_qr_case."""
import ctypes

import numpy as np
import pytest

from cases import assert_close, tol
from tensornetwork_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [np.complex64, np.complex128]
# smallest shapes reaching: 1 x 1, thin, wide, one full panel, a second panel of width 1 (odd complex64 pitch), two
# full panels, wide with several panels, the tall form with a narrow second panel (heights 600, 568: two K slices, no
# remainder), three tall panels with four K slices each (1100 = 4 * 275, 1068, 1036: no remainder).  Then the two that
# leave a remainder slice in W = V^H C (slices of mj / 256 rows each): a tall panel of 531 = 2 * 265 + 1 rows feeding
# a one-workgroup panel of 499, and panels of 1101 = 4 * 275 + 1, 1069 = 4 * 267 + 1 and 1037 = 4 * 259 + 1 rows at an
# odd pitch (complex64 rows of the trailing block 8-byte aligned only)
SHAPES = [(1, 1), (5, 3), (3, 5), (33, 32), (40, 33), (70, 64), (64, 96), (600, 40), (1100, 70), (531, 40), (1101, 71)]
EDGE_SHAPES = [(40, 33), (600, 40)]


def _random(shape, dtype, seed=0):
  rng = np.random.default_rng(seed)
  return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def _check(a, q, r, elementwise=True):
  q, r = np.asarray(q), np.asarray(r)
  m, n = a.shape
  k = min(m, n)
  assert q.shape == (m, k) and r.shape == (k, n) and q.dtype == a.dtype and r.dtype == a.dtype
  scale = float(np.max(np.abs(a))) + 1e-30
  np.testing.assert_allclose(q @ r, a, rtol=0, atol=10 * tol(a.dtype, scale)["atol"])
  np.testing.assert_allclose(q.conj().T @ q, np.eye(k), rtol=0, atol=10 * tol(a.dtype)["atol"])
  assert np.array_equal(r, np.triu(r))
  if elementwise:
    q_ref, r_ref = np.linalg.qr(a.astype(np.complex128))
    d = np.diagonal(r_ref)
    ph = np.where(d == 0, 1.0, d / np.where(d == 0, 1.0, np.abs(d)))
    assert_close(r, (ph.conj()[:, None] * r_ref).astype(a.dtype), scale=scale * np.sqrt(m))
    assert_close(q, (q_ref * ph).astype(a.dtype), scale=10.0)


@pytest.fixture
def native(hip, monkeypatch):
  monkeypatch.setattr(hip, "complex_qr", "native")
  return hip


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_native_qr_matches_lapack(native, shape, dtype):
  a = _random(shape, dtype)
  q, r = native.qr(native.convert_to_tensor(a), 1)
  assert native.last_qr_path == "native complex"
  _check(a, q, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_phase_only_columns(native, shape, dtype):
  a = np.triu(_random(shape, dtype, seed=1))        # xnorm == 0, Im alpha != 0 in every column
  q, r = native.qr(native.convert_to_tensor(a), 1)
  _check(a, q, r)
  d = np.diagonal(np.asarray(r))
  assert np.all(d.imag == 0)
  assert_close(d.real, np.abs(np.diagonal(a)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_rank_deficient(native, shape, dtype):
  a = _random(shape, dtype, seed=2)
  a[:, 7] = a[:, 2]
  a[:, 11] = 0
  q, r = native.qr(native.convert_to_tensor(a), 1)
  _check(a, q, r, elementwise=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_zero_matrix(native, shape, dtype):
  q, r = native.qr(native.convert_to_tensor(np.zeros(shape, dtype)), 1)
  assert np.array_equal(np.asarray(q), np.eye(*shape, dtype=dtype)[:, :min(shape)])
  assert np.array_equal(np.asarray(r), np.zeros((min(shape), shape[1]), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_rq(native, shape, dtype):
  a = _random(shape[::-1], dtype, seed=3)           # rq factors the conjugate transpose: (n, m) -> a tall QR
  r, q = native.rq(native.convert_to_tensor(a), 1)
  assert native.last_qr_path == "native complex"
  _check(a.conj().T, np.asarray(q).conj().T, np.asarray(r).conj().T)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_workgroup_form_agrees_with_tall_form(native, monkeypatch, dtype):
  a = _random((600, 40), dtype, seed=4)
  q_tall, r_tall = (np.asarray(x) for x in native.qr(native.convert_to_tensor(a), 1))
  monkeypatch.setenv("TNH_QR_TALL", "0")
  q, r = native.qr(native.convert_to_tensor(a), 1)
  _check(a, q, r)
  assert_close(r, r_tall, scale=float(np.max(np.abs(a))) * np.sqrt(600))
  assert_close(q, q_tall, scale=10.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_captured_qr_replays_bit_for_bit(native, shape, dtype):
  a = native.convert_to_tensor(_random(shape, dtype, seed=5))
  q, r = (np.asarray(x) for x in native.qr(a, 1))
  graph = native.capture(lambda t: native.qr(t, 1), a)
  try:
    for _ in range(3):
      gq, gr = graph.launch()
      assert np.array_equal(np.asarray(gq), q) and np.array_equal(np.asarray(gr), r)
  finally:
    graph.close()


def test_work_bytes_accepts_complex(hip):
  nbytes = ctypes.c_size_t(0)
  assert hip.lib.tnh_qr_work_bytes(_lib.C128, 40, 33, ctypes.byref(nbytes)) == _lib.OK
  assert nbytes.value >= 40 * 33 * 16
