"""HipBackend.svd on complex Gaussian inputs, all values kept: median / min / max of 9 timed calls after 3 warm-ups."""
import os, sys, time, json
import numpy as np
sys.path.insert(0, os.getcwd())
import tensornetwork_amd as ta
hip = ta.get_hip_backend()
hip.svd_band = False
tag = sys.argv[1]
for dtype in (np.complex64, np.complex128):
  for n in (96, 128, 192, 256, 384):
    rng = np.random.default_rng(n)
    x = hip.convert_to_tensor((rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))).astype(dtype))
    ts = []
    for i in range(12):
      t0 = time.perf_counter()
      u, s, vh, rest = hip.svd(x, 1)
      np.asarray(vh); np.asarray(u)
      ts.append(time.perf_counter() - t0)
    ts = sorted(ts[3:])
    print(json.dumps({"lib": tag, "dtype": np.dtype(dtype).name, "n": n, "sweeps": hip.last_svd_sweeps,
                      "median_ms": round(ts[4] * 1e3, 3), "min_ms": round(ts[0] * 1e3, 3), "max_ms": round(ts[-1] * 1e3, 3)}), flush=True)
