"""pytest configuration: markers, import paths and the golden-fixture loader."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
  if p not in sys.path:
    sys.path.insert(0, p)


def _golden_parts():
  """tests/golden/npz_parts.py (the fixture sets are stored as several archives of under 1 MiB each)."""
  import importlib.util
  spec = importlib.util.spec_from_file_location("npz_parts", os.path.join(HERE, "golden", "npz_parts.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def pytest_configure(config):
  config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


class Golden:
  """tests/golden/golden.part*.npz + cases.json (made by tests/golden/make_golden.py)."""

  def __init__(self):
    self.arrays = _golden_parts().load(os.path.join(HERE, "golden", "golden"))
    with open(os.path.join(HERE, "golden", "cases.json")) as f:
      self.cases = json.load(f)

  def __getitem__(self, name):
    return self.arrays[name]


@pytest.fixture(scope="session")
def golden():
  return Golden()


class GoldenLinalg(Golden):
  """tests/golden/golden_linalg.part*.npz + cases_linalg.json (made by make_golden_linalg.py)."""

  def __init__(self):  # pylint: disable=super-init-not-called
    self.arrays = _golden_parts().load(os.path.join(HERE, "golden", "golden_linalg"))
    with open(os.path.join(HERE, "golden", "cases_linalg.json")) as f:
      self.cases = json.load(f)


@pytest.fixture(scope="session")
def golden_linalg():
  return GoldenLinalg()


class GoldenComplex(Golden):
  """tests/golden/golden_complex.part*.npz + cases_complex.json (made by make_golden_complex.py)."""

  def __init__(self):  # pylint: disable=super-init-not-called
    self.arrays = _golden_parts().load(os.path.join(HERE, "golden", "golden_complex"))
    with open(os.path.join(HERE, "golden", "cases_complex.json")) as f:
      self.cases = json.load(f)


@pytest.fixture(scope="session")
def golden_complex():
  return GoldenComplex()


@pytest.fixture(scope="session")
def hip():
  """The hip backend bound to cuda:0 -- fails loudly if libtnhip or the GPU is missing."""
  import tensornetwork_amd as ta
  be = ta.get_hip_backend()
  be.lib  # initialise: raises HipRuntimeError without a gfx950 device  # pylint: disable=pointless-statement
  return be
