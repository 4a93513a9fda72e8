"""HipBackend.complex_qr on the emulated library: the default and the rejection of unknown values."""
import numpy as np
import pytest

from cases import assert_close
from emu_tnh import emulated_backend


def test_default_is_embedded_and_matches_lapack_in_the_non_negative_gauge():
  rng = np.random.default_rng(0)
  a = rng.standard_normal((9, 5)) + 1j * rng.standard_normal((9, 5))
  with emulated_backend() as be:
    assert be.complex_qr == "embedded"
    q, r = be.qr(be.convert_to_tensor(a), 1)
    assert be.last_qr_path == "embedded complex"
    q, r = np.asarray(q), np.asarray(r)
  q_ref, r_ref = np.linalg.qr(a)
  ph = np.diagonal(r_ref) / np.abs(np.diagonal(r_ref))
  assert_close(r, ph.conj()[:, None] * r_ref, scale=3.0 * float(np.max(np.abs(a))))
  assert_close(q, q_ref * ph, scale=10.0)


def test_unknown_value_raises():
  with emulated_backend() as be:
    be.complex_qr = "planar"
    with pytest.raises(ValueError, match="complex_qr"):
      be.qr(be.convert_to_tensor(np.ones((3, 2), np.complex128)), 1)
