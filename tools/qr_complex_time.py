"""HipBackend.qr on complex Gaussian inputs, complex_qr = "native" against "embedded": the two settings alternate call by
call on the same device tensor; device events around each call, 3 warm-ups then 9 timed calls per setting; median / min
/ max in ms, one JSON line per (dtype, shape), the largest element-wise difference of the two R factors, and the shader
clock sampled from sysfs (tensornetwork_amd.telemetry) while that shape's calls run.

  python tools/qr_complex_time.py [TAG]
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import tensornetwork_amd as ta  # pylint: disable=wrong-import-position
from tensornetwork_amd import _lib, telemetry  # pylint: disable=wrong-import-position

SHAPES = [(512, 256), (1024, 1024), (2048, 512), (4096, 1024), (1024, 4096)]
WARMUP, REPEATS = 3, 9


def main():
  hip = ta.get_hip_backend()
  tag = sys.argv[1] if len(sys.argv) > 1 else ""
  tel = telemetry.Telemetry(hip.lib)
  for dtype in (np.complex64, np.complex128):
    for shape in SHAPES:
      rng = np.random.default_rng(shape[0] + shape[1])
      x = hip.convert_to_tensor((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype))
      times = {"native": [], "embedded": []}
      r = {}
      with telemetry.Sampler(tel, period=0.005, skip_fraction=0.0) as clock:   # shader clock while the calls run
        for _ in range(WARMUP + REPEATS):
          for mode in ("native", "embedded"):
            hip.complex_qr = mode
            start = _lib.Event().record()
            _, r[mode] = hip.qr(x, 1)
            stop = _lib.Event().record()
            stop.synchronize()
            times[mode].append(start.elapsed_ms(stop))
      clk = clock.summary()
      row = {"lib": tag, "dtype": np.dtype(dtype).name, "m": shape[0], "n": shape[1],
             "sclk_mean_mhz": clk["sclk_mean_mhz"], "sclk_min_mhz": clk["sclk_min_mhz"],
             "max_abs_diff_r": float(np.max(np.abs(np.asarray(r["native"]) - np.asarray(r["embedded"]))))}
      for mode, ts in times.items():
        ts = sorted(ts[WARMUP:])
        row[mode] = {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}
      row["native_over_embedded"] = round(row["native"]["median_ms"] / row["embedded"]["median_ms"], 3)
      print(json.dumps(row), flush=True)
  hip.complex_qr = "embedded"


if __name__ == "__main__":
  main()
