"""`HipBackend.complex_lowering` on the emulated C ABI: which launches a planned complex tensordot makes."""
import numpy as np
import pytest

from emu_tnh import emulated_backend


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("lowering", ["native", "embedded"])
def test_complex_tensordot_with_a_k_major_a(lowering, tb):
  m, n, k = 96, 64, 48
  rng = np.random.default_rng(3)
  a = (rng.standard_normal((k, m)) + 1j * rng.standard_normal((k, m))).astype(np.complex64)
  b_shape = (n, k) if tb else (k, n)
  b = (rng.standard_normal(b_shape) - 1j * rng.standard_normal(b_shape)).astype(np.complex64)
  with emulated_backend() as be:
    if lowering == "native":
      be.complex_lowering = "native"
    da, db = be.convert_to_tensor(a), be.convert_to_tensor(b)
    del be.lib.calls[:]
    out = np.asarray(be.tensordot(da, db, [[0], [1 if tb else 0]]))
    calls = list(be.lib.calls)
  if lowering == "native":      # ONE complex GEMM on the operands where they lie: no transpose of A, no expansion of B
    assert calls == [("gemm", 1, tb, m, n, k, 1)]
  else:                         # A brought to row-major, then the real M x 2N x 2K product
    assert calls[-1] == ("gemm", 0, 0, m, 2 * n, 2 * k, 1)
    assert calls[0][0] == "permute"
  np.testing.assert_allclose(out, np.tensordot(a, b, [[0], [1 if tb else 0]]), rtol=1e-4, atol=1e-4)


def test_unknown_complex_lowering_is_an_error():
  with emulated_backend() as be:
    be.complex_lowering = "planar"
    x = be.convert_to_tensor(np.ones((8, 8), np.complex64))
    with pytest.raises(ValueError, match="complex_lowering"):
      be.tensordot(x, x, [[1], [0]])
