"""complex64 / complex128 SVD on the block-Jacobi path (tnh_svd_block_complex.hip) and the basis completion of
exactly rank-deficient complex inputs, against np.linalg.svd of the input in complex128.  Tolerances: complex64 as
test_complex_svd_larger_vs_oracle, complex128 as the float64 row of test_svd_graded_and_rank_deficient_block_path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (singular values / s_1, orthonormality, product: absolute for complex64, / s_1 for complex128)
TOL = {np.complex64: (2e-5, 2e-4, 2e-3), np.complex128: (1e-12, 1e-11, 1e-11)}
DTYPES = [np.complex64, np.complex128]


def _gauss(rng, shape):
  return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _check(hip, x, k):
  """All min(m, n) values, U^H U = 1, Vh Vh^H = 1, U diag(s) Vh = rank-k truncation of the reference."""
  stol, otol, ptol = TOL[x.dtype.type]
  u, s, vh, rest = hip.svd(hip.convert_to_tensor(x), 1, max_singular_values=k)
  uo, so, vo = np.linalg.svd(x.astype(np.complex128), full_matrices=False)
  k = len(so) if k is None else k
  s_all = np.real(np.concatenate([np.asarray(s), np.asarray(rest)])).astype(np.float64)
  um, vm = np.asarray(u).astype(np.complex128), np.asarray(vh).astype(np.complex128)
  assert um.shape == (x.shape[0], k) and vm.shape == (k, x.shape[1]) and s_all.shape == so.shape
  assert np.abs(s_all - so).max() <= stol * so[0]
  assert np.abs(um.conj().T @ um - np.eye(k)).max() <= otol
  assert np.abs(vm @ vm.conj().T - np.eye(k)).max() <= otol
  ref = (uo[:, :k] * so[:k]) @ vo[:k]
  assert np.abs((um * s_all[:k]) @ vm - ref).max() <= ptol * (1.0 if x.dtype == np.complex64 else so[0])
  return s_all


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,k", [((65, 70), None), ((96, 200), 24), ((200, 96), None), ((160, 160), 40),
                                     ((257, 260), 64), ((128, 128), "graded")])
def test_block_path_vs_lapack(hip, monkeypatch, dtype, shape, k):
  """First block-path size (rows padded 65 -> 128, ragged Q), wide and transposed entry, 8 and 12 blocks (the band
  path, which would take 257 x 260, switched off), and a graded spectrum 2^-j."""
  monkeypatch.setattr(hip, "svd_band", False, raising=False)
  rng = np.random.default_rng(shape[0] * 7 + shape[1])
  x = _gauss(rng, shape)
  if k == "graded":
    qu, _ = np.linalg.qr(x)
    qv, _ = np.linalg.qr(_gauss(rng, shape))
    x, k = (qu * 2.0 ** -np.arange(shape[0])) @ qv.conj().T, None
  _check(hip, x.astype(dtype), k)
  assert hip.last_svd_path == "jacobi"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["rank40_96x80", "rank10_40x48", "dup_rows_130x70", "zero_padded_96x80",
                                  "zero_padded_40x48"])
def test_rank_deficient_complex_gets_a_complete_basis(hip, monkeypatch, dtype, kind):
  """Exact rank deficiency (block path and the 2-row path): U and Vh orthonormal INCLUDING the completed vectors,
  zeros in s where LAPACK has them, reconstruction.  The zero-padded inputs (a DMRG split of a padded tensor) leave
  exactly zero rows on both paths: NotImplementedError before the completion existed; the duplicated rows did not
  converge."""
  monkeypatch.setattr(hip, "svd_band", False, raising=False)
  rng = np.random.default_rng(len(kind))
  if kind == "rank40_96x80":
    x = _gauss(rng, (96, 40)) @ _gauss(rng, (40, 80))
  elif kind == "rank10_40x48":
    x = _gauss(rng, (40, 10)) @ _gauss(rng, (10, 48))
  elif kind.startswith("zero_padded"):
    m, n = (96, 80) if kind.endswith("96x80") else (40, 48)
    x = np.zeros((m, n), dtype=np.complex128)
    x[:m // 2, :n // 2] = _gauss(rng, (m // 2, n // 2))
  else:
    x = np.repeat(_gauss(rng, (65, 70)), 2, axis=0)
  _check(hip, x.astype(dtype), None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_block_path_and_two_row_kernel_agree(hip, monkeypatch, dtype):
  """The 2-row kernel (TNH_SVD_BLOCK=0) is the on-device second opinion: both meet LAPACK and each other."""
  monkeypatch.setattr(hip, "svd_band", False, raising=False)
  x = _gauss(np.random.default_rng(12), (128, 96)).astype(dtype)
  monkeypatch.delenv("TNH_SVD_BLOCK", raising=False)
  s_block = _check(hip, x, None)
  monkeypatch.setenv("TNH_SVD_BLOCK", "0")
  s_rows = _check(hip, x, None)
  assert np.abs(s_block - s_rows).max() <= TOL[dtype][0] * s_block[0]
