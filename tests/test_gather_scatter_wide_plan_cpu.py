"""The output descriptor of the wide form of tnh_gemm_gather_scatter (hip_backend._scatter_descriptor with the wide
kernel's box bound of 256 contracted indices): the bond D = 16 product, Ms = K = 256, lands where NumPy's transpose puts
it -- the check of test_gather_scatter_plan_cpu, run with that bound.  No GPU, no library call."""
import functools

import pytest

from tensornetwork_amd import hip_backend
import test_gather_scatter_plan_cpu as narrow

_SHAPE, _K_AXES = (16,) * 5, [1, 3]


# destination as a permutation of [long's free axes 0, 2, 4, small's two free axes]
@pytest.mark.parametrize("dest,want_run", [
    ((0, 3, 1, 2, 4), 16),      # innermost: the small operand's innermost free axis
    ((3, 0, 4, 1, 2), 64),      # innermost: the box (axis 4 x 4 of axis 2)
])
def test_wide_scatter_descriptor_lands_where_numpy_transposes(monkeypatch, dest, want_run):
  wide = functools.partial(hip_backend._scatter_descriptor, max_box_k=256)      # pylint: disable=protected-access
  monkeypatch.setattr(hip_backend, "_scatter_descriptor", wide)
  narrow.test_scatter_descriptor_lands_where_numpy_transposes(_SHAPE, _K_AXES, (16, 16), dest, 64, want_run)


def test_narrow_bound_still_refuses_256_contracted_indices():
  strides = hip_backend._row_major_strides((16,) * 5)      # pylint: disable=protected-access
  out_strides = [strides[0], 0, strides[1], 0, strides[2]]
  assert hip_backend._scatter_descriptor(_SHAPE, _K_AXES, out_strides, [16, 16], strides[3:]) is None      # pylint: disable=protected-access
  assert hip_backend._scatter_descriptor(_SHAPE, _K_AXES, out_strides, [16, 16], strides[3:], 256) is not None      # pylint: disable=protected-access
