"""Native complex GEMM (mfma_c64_* / mfma_c128_*) against what it replaces, on the GPU, as two markdown tables:
  (a) batched `matmul`: native against the VALU kernel (`tnh_gemm_set_variant("valu")`);
  (b) 2-D `tensordot` at MPS-step shapes M = 2D, N = K = D in the four storage layouts: `complex_lowering = "native"`
      against "embedded" (tnh_complex_expand + ONE real GEMM, plus a transpose of a k-major A).
Each cell: the two columns called alternately after warm-up, `--inner` calls between two HIP events on the library
stream, median and [min, max] over `--reps` windows in microseconds per call.  `diff`: the largest difference between
the two columns' results on two slices (the first and the last 8 rows), relative to the largest value there.
  python tools/complex_gemm_ab.py [--reps 15] [--inner 10] [--out profiles/complex_native.md]"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tensornetwork_amd as ta
from tensornetwork_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
be = ta.get_hip_backend()
rng = np.random.default_rng(11)
lines = []


def emit(line):
  print(line, flush=True)
  lines.append(line)


def operand(shape, dtype):
  return be.convert_to_tensor((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype))


def window(fn):
  start = _lib.Event().record()
  for _ in range(args.inner):
    out = fn()
  stop = _lib.Event().record()
  stop.synchronize()
  return start.elapsed_ms(stop) * 1e3 / args.inner, out


def ab(fx, fy):
  """Alternating windows of the two callables: (cell x, cell y, diff, kernel x, kernel y)."""
  names = []
  for fn in (fx, fy):
    for _ in range(3):
      fn()
    names.append(be.lib.tnh_gemm_last_kernel().decode())
  _lib.sync()
  tx, ty = [], []
  for _ in range(args.reps):
    t, ox = window(fx)
    tx.append(t)
    t, oy = window(fy)
    ty.append(t)
  ox, oy = np.asarray(ox), np.asarray(oy)
  ox, oy = ox.reshape(-1, ox.shape[-1]), oy.reshape(-1, oy.shape[-1])
  diff = max(float(np.abs(ox[s] - oy[s]).max() / np.abs(oy[s]).max()) for s in (slice(0, 8), slice(-8, None)))
  cell = lambda t: f"{statistics.median(t):.1f} [{min(t):.1f}, {max(t):.1f}]"
  return cell(tx), cell(ty), diff, names[0], names[1]


def with_variant(variant, fn):
  def run():
    _lib.check(be.lib.tnh_gemm_set_variant(variant))
    try:
      return fn()
    finally:
      _lib.check(be.lib.tnh_gemm_set_variant(b"auto"))
  return run


def with_lowering(value, fn):
  def run():
    be.complex_lowering = value
    try:
      return fn()
    finally:
      be.complex_lowering = "embedded"
  return run


emit("## (a) batched matmul: native against the VALU kernel (us per call: median [min, max])\n")
emit("| dtype | batch x (M, N, K) | native | valu | speed-up | diff | native kernel |")
emit("|---|---|---|---|---|---|---|")
for dtype in (np.complex64, np.complex128):
  for batch, m, n, k in ((64, 128, 128, 128), (4096, 16, 16, 16), (16, 1024, 512, 512)):
    a, b = operand((batch, m, k), dtype), operand((batch, k, n), dtype)
    mm = lambda a=a, b=b: be.matmul(a, b)
    x, y, diff, kx, _ = ab(mm, with_variant(b"valu", mm))
    emit(f"| {np.dtype(dtype).name} | {batch} x ({m}, {n}, {k}) | {x} | {y} | "
         f"{float(y.split()[0]) / float(x.split()[0]):.2f} | {diff:.1e} | {kx} |")

emit("\n## (b) tensordot, M = 2D, N = K = D: complex_lowering native against embedded (us per call)\n")
emit("| dtype | D | A, B stored | native | embedded | speed-up | diff | native kernel | embedded GEMM |")
emit("|---|---|---|---|---|---|---|---|---|")
for dtype in (np.complex64, np.complex128):
  for D in (64, 128, 256, 512, 1024):
    m, n, k = 2 * D, D, D
    for ta_, tb_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
      a, b = operand((k, m) if ta_ else (m, k), dtype), operand((n, k) if tb_ else (k, n), dtype)
      td = lambda a=a, b=b, ta_=ta_, tb_=tb_: be.tensordot(a, b, [[0 if ta_ else 1], [1 if tb_ else 0]])
      x, y, diff, kx, ky = ab(with_lowering("native", td), with_lowering("embedded", td))
      emit(f"| {np.dtype(dtype).name} | {D} | {'KM' if ta_ else 'MK'}, {'NK' if tb_ else 'KN'} | {x} | {y} | "
           f"{float(y.split()[0]) / float(x.split()[0]):.2f} | {diff:.1e} | {kx} | {ky} |")

if args.out:
  with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
